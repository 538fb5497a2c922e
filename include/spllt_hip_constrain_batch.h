/*
 * spllt_hip_constrain_batch.h -- hard linear constraints C x = e for the members of the LAST batch: conditioned
 * solves, samples and marginal variances of every member in each launch (spllt_amd/csrc/constrain_batch.hip,
 * DESIGN.md section 26).  The batch twin of spllt_hip_constrain.h.
 *
 * WHY A HEADER OF ITS OWN.  As spllt_hip_constrain.h: the recorded table of the entry ladder (tests/capi_ladder.py and
 * the two files under tests/golden/) has one row per entry point of spllt_hip.h and is recorded from the library of
 * the commit BEFORE a change of the boundary.  This family was added without regenerating that table, so it is
 * declared here, bound by a table of its own (spllt_amd/_lib.py, _CONSTRAIN_BATCH) and checked by a ladder of its own
 * (tests/constrain_batch_ladder.py), whose expected codes are the recorded rows of the siblings
 * spllt_hip_solve_many(_dev) (the rows of C), spllt_hip_solve_batch(_dev) (the vector arguments and the accepted
 * call, as spllt_hip_solve_many_batch(_dev) and spllt_hip_sample_batch(_dev) follow them),
 * spllt_hip_inverse_diag_batch, spllt_hip_solve_sparse_info and spllt_hip_release_batch.
 *
 * THE MATHEMATICS, per member b of the last batch, all in user variable order.  A_b: the matrix of member b.  C: ONE
 * k x n matrix, 1 <= k <= 64 dense rows, shared by all members.
 *   W_b = A_b^-1 C^T (n x k),  S_b = C W_b = G_b G_b^T (k x k),  U_b = W_b G_b^-T (n x k)
 *   correction of x towards C x = e:   r = C x - e,  t = G_b^-1 r,  x* = x - U_b t,  lambda = G_b^-T t = S_b^-1 r
 *   constrained solve:                 correct(A_b^-1 b)
 *   constrained sample of N(mu_b, A_b^-1) | C x = e:   correct(the kind-0 sample of spllt_hip_sample_batch)
 *   constrained marginal variances:    (A_b^-1)_ii - sum_j U_b[i, j]^2
 *
 * LAYOUT.  The batch's: vector q of member b at x[(b*nvec + q)*ldx .. + n), ldx >= n.  C: row i at c[i*ldc .. + n),
 * ldc >= n.  e: null means zeros; lde = 0 means one column of k targets shared by every vector of every member; else
 * the targets of vector q of member b at e[(b*nvec + q)*lde .. + k), lde >= k.  lambda: null, or the multipliers at
 * lambda[(b*nvec + q)*ldl .. + k), ldl >= k.  Nothing outside these ranges is read or written; a NaN in a caller's
 * padding never reaches a product.
 *
 * STORAGE, one all-or-nothing transaction, in doubles, for nbatch members and nc = the number of chunks of n (chunks
 * of max(64, 64 ceil(ceil(n / 256) / 64)) positions, at most 256 of them):
 *     k n  (C)  +  nbatch k n  (U)  +  nbatch (64 * 64 + 4)  (G and the scalars)
 *     +  nbatch nc 64 * 64  (the partial sums)  +  nbatch 3 * 32 * 64  (T, and the staged e and lambda of a pass)
 * Failure: SPLLT_ERROR_ALLOCATION, nothing kept.  Host vectors go through the batch's own staging buffer, which
 * grows as for spllt_hip_solve_many_batch.
 *
 * INDEPENDENT STATE.  These constraints belong to the batch: they neither read nor touch the constraints of
 * spllt_hip_constrain.h on the same handle, as the batch factor and the single factor are independent.
 * spllt_hip_release_batch and spllt_deallocate_fkeep give the storage back too (C is then forgotten).
 *
 * A LATER BATCH IS PICKED UP.  C stays stored; U_b, G_b and the scalars belong to ONE batch (the handle counts its
 * spllt_hip_factor_batch(_dev) calls).  After a new batch the first call that needs them rebuilds them: the blocked
 * batch solve of k columns per member plus three launches; a batch with more members than the storage holds takes
 * the storage again first.  Numbers of an old batch are never returned: until the rebuild,
 * spllt_hip_constraints_batch_info reports NaN for every member.
 *
 * A MEMBER THAT IS NOT POSITIVE DEFINITE.  Nothing of it is read or written by the kernels of this family: its
 * vectors stay bit-identical for spllt_hip_constrain_batch and spllt_hip_solve_constrained_batch; its lambda, its
 * samples and its variance row are NaN; its scalars are NaN.  The call returns SPLLT_ERROR_NOT_POSDEF after serving
 * the others (the convention of spllt_hip_sample_batch and spllt_hip_solve_refined_batch).
 *
 * DEPENDENT CONSTRAINTS.  The pivot test of spllt_hip_constrain.h (pivot_j <= 2^-26 S_jj, or not finite), applied to
 * every factorized member.  If ANY of them fails it, spllt_hip_set_constraints_batch returns SPLLT_ERROR_NOT_POSDEF
 * with a message that names the first such member (0-based, as spllt_hip_batch_status) and the row (1-based):
 * "member 2, row 5 of C".  The batch then holds NO constraints; the batch factor and every other call stay usable.
 *
 * WHICH SOLVE.  W_b is always built with spllt_hip_solve_many_batch_dev; the solve of
 * spllt_hip_solve_constrained_batch is its job 0; the sample is the kind-0 path of spllt_hip_sample_batch(_dev),
 * spllt_hip_set_batch_blocked_solve included.  The kernels of this family use no atomic add: every sum has an order
 * fixed by n, k and the wavefront number, which depends neither on nbatch, nor on nvec, nor on a vector's place in
 * its pass of at most 32, nor on the other members' data, nor on the entry point.
 *
 * ERRORS, in the order of the entry ladder: null handle or pointer, k < 0, k > 64, ldc < n, a negative count,
 * ldx < n, 0 < lde < k, ldl < k with lambda given -> SPLLT_ERROR_PARAMETER; a partitioned handle ->
 * SPLLT_ERROR_UNIMPLEMENTED; no batch yet, no constraints set -> SPLLT_ERROR_PARAMETER; no device memory ->
 * SPLLT_ERROR_ALLOCATION with nothing kept.  The work is ordered on the engine's stream and has finished when a call
 * returns.
 *
 * The header is self-contained; the handle is the fkeep of spllt_iface.h, the error codes are its SPLLT_ERROR_*
 * values (PARAMETER -10, NOT_POSDEF -20, HIP -30, UNIMPLEMENTED -98, ALLOCATION -1).
 */
#ifndef SPLLT_HIP_CONSTRAIN_BATCH_H
#define SPLLT_HIP_CONSTRAIN_BATCH_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* stores C and computes W_b (the blocked batch solve), S_b, G_b, U_b, log det S_b and the smallest relative pivot for
 * every member of the last batch.  1 <= k <= 64; k = 0 clears the constraints (c is then not read and may be null). */
int spllt_hip_set_constraints_batch(void *fkeep, int k, const double *c_host, int64_t ldc);
int spllt_hip_set_constraints_batch_dev(void *fkeep, int k, const double *c_dev, int64_t ldc);

/* the correction, in place, of nvec vectors per member.  nvec = 0 is a no-op. */
int spllt_hip_constrain_batch(void *fkeep, int nvec, double *x_host, int64_t ldx, const double *e_host, int64_t lde,
                              double *lambda_host, int64_t ldl);
int spllt_hip_constrain_batch_dev(void *fkeep, int nvec, double *x_dev, int64_t ldx, const double *e_dev, int64_t lde,
                                  double *lambda_dev, int64_t ldl);

/* spllt_hip_solve_many_batch_dev (job 0) on the right-hand sides in x, then the correction */
int spllt_hip_solve_constrained_batch(void *fkeep, int nrhs, double *x_host, int64_t ldx, const double *e_host,
                                      int64_t lde, double *lambda_host, int64_t ldl);
int spllt_hip_solve_constrained_batch_dev(void *fkeep, int nrhs, double *x_dev, int64_t ldx, const double *e_dev,
                                          int64_t lde, double *lambda_dev, int64_t ldl);

/* the kind-0 path of spllt_hip_sample_batch(_dev) -- same noise, streams and mean handling (mean: null, n doubles for
 * all members with ldmean = 0, or member b's at mean + b*ldmean) --, then the correction.  e: k shared targets or
 * null. */
int spllt_hip_sample_constrained_batch(void *fkeep, int nsamp, double *x_host, int64_t ldx, uint64_t seed,
                                       uint64_t first_sample, uint32_t stream0, int stream_step,
                                       const double *mean_host, int64_t ldmean, const double *e_host);
int spllt_hip_sample_constrained_batch_dev(void *fkeep, int nsamp, double *x_dev, int64_t ldx, uint64_t seed,
                                           uint64_t first_sample, uint32_t stream0, int stream_step,
                                           const double *mean_dev, int64_t ldmean, const double *e_dev);

/* out[b*ldout + i] = (A_b^-1)_ii - sum_j U_b[i, j]^2 (host, user order), ldout >= n.  Needs a valid selected inverse of
 * the batch and fails like spllt_hip_inverse_diag_batch when there is none or it is stale. */
int spllt_hip_inverse_diag_constrained_batch(void *fkeep, double *out, int64_t ldout);

/* out[0]: k (0: none set), out[1]: rebuilds of the U_b so far (the first build included), out[2]: device bytes held,
 * out[3]: kernel launches of this family in the last call.  stat (may be null; ldstat >= 2), for every member of the
 * last batch: stat[b*ldstat + 0] = log det S_b, stat[b*ldstat + 1] = the smallest pivot_j / S_jj of S_b; NaN for a
 * member that is not positive definite.  Zeros on a handle without an engine or without constraints. */
int spllt_hip_constraints_batch_info(void *fkeep, int64_t out[4], double *stat, int64_t ldstat);

/* everything back to the pool, C forgotten.  Return codes as spllt_hip_release_batch. */
int spllt_hip_release_constraints_batch(void *fkeep);

#ifdef __cplusplus
}
#endif
#endif
