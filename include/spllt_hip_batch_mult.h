/*
 * spllt_hip_batch_mult.h -- factor products and Gaussian sampling for every member of a batch: the batch
 * twins of spllt_hip_factor_mult, spllt_hip_white_noise_dev and spllt_hip_sample of spllt_hip.h.
 *
 * WHY A HEADER OF ITS OWN.  The recorded table of the entry ladder (tests/capi_ladder.py and the two files
 * under tests/golden/) has one row per entry point of spllt_hip.h that takes a handle, and it is recorded
 * from the library of the commit BEFORE a change of the boundary.  This family was added without
 * regenerating that table, so it is declared here, bound by a table of its own (spllt_amd/_lib.py,
 * _BATCH_MULT) and checked by a ladder of its own (tests/test_batch_mult_cpu.py, tests/test_batch_mult_gpu.py),
 * whose expected codes are the recorded rows of the siblings spllt_hip_solve_batch / spllt_hip_solve_batch_dev.
 * When the table is next regenerated these declarations are to be folded into the batch section of
 * spllt_hip.h, with their rows in tests/capi_ladder.py and their prototypes in _lib._HIP, and this file goes.
 *
 * The header is self-contained; the handle is the fkeep of spllt_iface.h, the error codes are its
 * SPLLT_ERROR_* values (PARAMETER -10, NOT_POSDEF -20, HIP -30, UNIMPLEMENTED -98, ALLOCATION -1).
 */
#ifndef SPLLT_HIP_BATCH_MULT_H
#define SPLLT_HIP_BATCH_MULT_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- batched factor products and sampling (single GPU) ----------------------------
 * For every member b of the LAST batch (spllt_hip_factor_batch) the factor L_b is applied instead of
 * inverted, and draws from N(mean_b, A_b) or N(mean_b, A_b^-1) are made from it.  There is no nbatch argument:
 * like spllt_hip_solve_batch every call works on ALL members of the last batch (spllt_hip_batch_status
 * returns their number).  Vector q of member b is at x[(b*nvec + q)*ldx .. + n), ldx >= n; nothing else is
 * read or written.
 *
 * A product has no dependency chain: a direction is two kernel launches whatever the elimination tree looks
 * like, and every launch carries all members, so the number of launches does not depend on nbatch.  The
 * kernels are those of spllt_hip_factor_mult applied to the members' arenas (a member's arena has the
 * layout of spllt_hip_get_factor): every product runs on the fp64 matrix cores, no sum is an atomic add, and
 * for vector q every sum runs in an order fixed by the pattern alone.  The same factor bits and vector bits
 * give the same result bits -- whatever nvec, q's place among the vectors, the other members' vectors, the
 * entry point (host, device, pivot order) or the block width -- and they are the bits
 * spllt_hip_factor_mult gives on a single handle that holds the same factor bits.
 *
 * Storage is taken from the handle's device pool on the first call: the tables of the products (shared
 * with spllt_hip_factor_mult and the reproducible solve when those are resident), two workspaces of
 * nbatch * 32 * n doubles and a scratch of nbatch * 32 * max(frows, bsize) doubles (the RsolveTables of
 * DESIGN.md); when that does not fit, all of it for blocks of 16 vectors, with the same bits per vector.
 * When that does not fit either the call returns SPLLT_ERROR_ALLOCATION, keeps nothing half-allocated, and
 * the batch, spllt_hip_solve_batch and the single factorization stay usable.  The storage stays until
 * spllt_hip_release_factor_mult_batch, spllt_hip_release_batch or spllt_deallocate_fkeep and is taken
 * again when a later batch brings a larger nbatch.  All work is ordered on spllt_hip_engine_stream and
 * finished when a call returns.
 *
 * A member that is not positive definite: its vectors of a product are left bit-identical (as
 * spllt_hip_solve_batch leaves them), its noise rows and its samples are NaN (they are outputs, like
 * spllt_hip_log_det_batch); the call returns SPLLT_ERROR_NOT_POSDEF and the other members are served.
 *
 * Errors, the rungs of spllt_hip_solve_batch(_dev) in the same order: null handle or pointer, negative
 * count, ldx < n, bad job or kind, stream_step not 0 or 1, 0 < ldmean < n, no batch yet ->
 * SPLLT_ERROR_PARAMETER; a handle after spllt_hip_set_partition with nranks > 1 ->
 * SPLLT_ERROR_UNIMPLEMENTED; no device -> SPLLT_ERROR_HIP.  Messages: spllt_hip_last_error.  nvec = 0,
 * nsamp = 0 and an empty batch are no-ops that return 0. */
/* x_b <- P^T L_b L_b^T P x_b (job 0, = A_b x_b to rounding), P^T L_b x_b (job 1) or L_b^T P x_b (job 2): the
 * jobs of spllt_hip_factor_mult.  spllt_hip_factor_mult_batch(job) undoes spllt_hip_solve_batch(job) and
 * the other way round.  pivot_order as spllt_hip_factor_mult_dev: non-zero = the vectors are in pivot
 * order on both sides and no permutation is applied.  The host entry point stages its vectors in groups
 * of at most 32 per member. */
int spllt_hip_factor_mult_batch(void *fkeep, int nvec, double *x_host, int64_t ldx, int job);
int spllt_hip_factor_mult_batch_dev(void *fkeep, int nvec, double *x_dev, int64_t ldx, int job, int pivot_order);
/* The standard normals of the batched samplers, in PIVOT order: z[(b*nsamp + q)*ldz + p], ldz >= n.  Entry
 * (pivot position p, member b, sample s = first_sample + q) is the one Philox4x32-10 block with counter
 * (p, stream0 + b*stream_step, s low word, s high word) and key (seed low word, seed high word), turned
 * into ONE normal by Box-Muller on its two 53-bit uniforms: the generator of spllt_hip_white_noise_dev,
 * whose counter word 1 is 0 -- stream 0 is bit for bit that noise.  stream_step 0 gives every member
 * the same noise (common random numbers, for comparing members), 1 gives every member a stream of its
 * own; stream0 keeps the streams of an ensemble apart that is split over several batches.  An entry is a
 * function of (seed, p, stream, s) alone. */
int spllt_hip_white_noise_batch_dev(void *fkeep, int nsamp, double *z_dev, int64_t ldz, uint64_t seed,
                                    uint64_t first_sample, uint32_t stream0, int stream_step);
/* nsamp draws per member, sample q of member b at x[(b*nsamp + q)*ldx .. + n), user order:
 *   kind 1 (covariance): x = mean_b + P^T L_b z_b    ~ N(mean_b, A_b), through the batched product; it repeats
 *                        bit for bit
 *   kind 0 (precision):  x = mean_b + P^T L_b^-T z_b ~ N(mean_b, A_b^-1), through the backward sweep of
 *                        spllt_hip_solve_batch_dev; it repeats to rounding only, as that solve does
 * with z_b the noise above.  mean: NULL = none; ldmean = 0: ONE mean of n doubles (user order) shared by all
 * members; ldmean >= n: member b's mean at mean + b*ldmean.  The mean is added on the device, by one fp64
 * add per entry.  mean of spllt_hip_sample_batch_dev is a device pointer. */
int spllt_hip_sample_batch(void *fkeep, int nsamp, double *x_host, int64_t ldx, int kind, uint64_t seed,
                           uint64_t first_sample, uint32_t stream0, int stream_step, const double *mean_host,
                           int64_t ldmean);
int spllt_hip_sample_batch_dev(void *fkeep, int nsamp, double *x_dev, int64_t ldx, int kind, uint64_t seed,
                               uint64_t first_sample, uint32_t stream0, int stream_step, const double *mean_dev,
                               int64_t ldmean);
/* give the workspaces, the scratch and (when no one else holds them) the tables back; the next call takes
 * them again.  Return codes as spllt_hip_release_batch. */
int spllt_hip_release_factor_mult_batch(void *fkeep);

#ifdef __cplusplus
}
#endif
#endif
