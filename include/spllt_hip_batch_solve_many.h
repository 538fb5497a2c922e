/*
 * spllt_hip_batch_solve_many.h -- the blocked many-right-hand-side solve for every member of a batch: the
 * batch twin of spllt_hip_solve_many of spllt_hip.h, and a second way to the numbers of spllt_hip_solve_batch.
 *
 * WHY A HEADER OF ITS OWN.  The recorded table of the entry ladder (tests/capi_ladder.py and the two files
 * under tests/golden/) has one row per entry point of spllt_hip.h that takes a handle, and it is recorded
 * from the library of the commit BEFORE a change of the boundary.  This family was added without
 * regenerating that table, so it is declared here, bound by a table of its own (spllt_amd/_lib.py,
 * _BATCH_SOLVE_MANY) and checked by a ladder of its own (tests/test_solve_many_batch_cpu.py,
 * tests/test_solve_many_batch_gpu.py), whose expected codes are the recorded rows of the siblings
 * spllt_hip_solve_batch / spllt_hip_solve_batch_dev / spllt_hip_release_batch.  When the table is next
 * regenerated these declarations are to be folded into the batch section of spllt_hip.h (together with
 * those of spllt_hip_batch_mult.h), with their rows in tests/capi_ladder.py and their prototypes in
 * _lib._HIP, and this file goes.
 *
 * The header is self-contained; the handle is the fkeep of spllt_iface.h, the error codes are its
 * SPLLT_ERROR_* values (PARAMETER -10, NOT_POSDEF -20, HIP -30, UNIMPLEMENTED -98, ALLOCATION -1).
 */
#ifndef SPLLT_HIP_BATCH_SOLVE_MANY_H
#define SPLLT_HIP_BATCH_SOLVE_MANY_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- blocked solve for the members of a batch (single GPU) ------------------------------
 * What spllt_hip_solve_batch(_dev) computes, for ALL members of the LAST batch (spllt_hip_factor_batch), by the
 * kernels of spllt_hip_solve_many applied to the members' arenas: a member's vectors go in blocks of 32 (a tail
 * of at most 16 is a block of 16), every product runs on the fp64 matrix cores, and a member's factor is read
 * once per BLOCK where spllt_hip_solve_batch reads it once per VECTOR.  Vector q of member b is at
 * x[(b*nrhs + q)*ldx .. + n), ldx >= n, the layout of spllt_hip_solve_batch; nothing else is read or written.
 * job 0: A_b x = b; 1: the forward sweep; 2: the backward sweep.  pivot_order as spllt_hip_solve_batch_dev.
 * Per block the launches are a pack, those of the batch's solve program and an unpack; every launch carries all
 * members, so their number does not depend on nbatch (unless a grid would overflow and the members are split
 * into ranges).  The strips add with fp64 atomics: results repeat to rounding only, as those of
 * spllt_hip_solve_batch do, and agree with them to rounding.
 *
 * WHEN TO USE IT.  With more than a few right-hand sides per member: measured, with 8 or
 * more per member and 4 or more members it is 1.3 to 12 times faster than spllt_hip_solve_batch_dev.  With a
 * single right-hand side per member a block of 16 carries 15 columns of zeros, and for the backward sweep alone
 * (job 2) spllt_hip_solve_batch_dev is then the faster call (this one at 0.73-0.98 of it); so it is for a batch
 * of ONE small matrix with well over 32 right-hand sides of job 2 (0.57 on a 128 x 128 Poisson problem with 128).
 * Nothing is routed here by default.
 *
 * Storage is taken from the handle's device pool on the first call: nbatch * 32 * n doubles; when that does not
 * fit, nbatch * 16 * n doubles and blocks of 16 only.  When that does not fit either the call returns
 * SPLLT_ERROR_ALLOCATION, keeps nothing, and the batch, spllt_hip_solve_batch and the single factorization
 * stay usable.  The storage stays until spllt_hip_release_solve_many_batch, spllt_hip_release_batch or
 * spllt_deallocate_fkeep and is taken again when a later batch brings a larger nbatch.  The host entry point
 * stages its vectors in groups of at most 32 per member.  All work is ordered on spllt_hip_engine_stream and
 * finished when a call returns.
 *
 * A member that is not positive definite: its vectors are left bit-identical, the call returns
 * SPLLT_ERROR_NOT_POSDEF and the other members are served.
 *
 * Errors, the rungs of spllt_hip_solve_batch(_dev) in the same order: null handle or pointer, negative count,
 * ldx < n, bad job, no batch yet -> SPLLT_ERROR_PARAMETER; a handle after spllt_hip_set_partition with
 * nranks > 1 -> SPLLT_ERROR_UNIMPLEMENTED; no device -> SPLLT_ERROR_HIP.  Messages: spllt_hip_last_error.
 * nrhs = 0 is a no-op that returns 0. */
int spllt_hip_solve_many_batch(void *fkeep, int nrhs, double *x_host, int64_t ldx, int job);
int spllt_hip_solve_many_batch_dev(void *fkeep, int nrhs, double *x_dev, int64_t ldx, int job, int pivot_order);
/* on != 0: the backward sweep of the precision kind (kind 0) of spllt_hip_sample_batch(_dev) runs through the
 * blocked path instead of spllt_hip_solve_batch_dev; the noise, the mean, the covariance kind and the NaN samples
 * of a member that is not positive definite are untouched.  Off by default.  Returns the previous setting (0 or
 * 1); SPLLT_ERROR_PARAMETER without an analysis; SPLLT_ERROR_UNIMPLEMENTED when switched on on a partitioned
 * handle. */
int spllt_hip_set_batch_blocked_solve(void *fkeep, int on);
/* out[0]: the block width in use (32; 16 when the storage for 32 did not fit; 0 while none is held), out[1]: blocks
 * per member and out[2]: kernel launches of the last spllt_hip_solve_many_batch(_dev), out[3]: bytes of the
 * workspace.  Zeros on a handle without an engine. */
int spllt_hip_solve_many_batch_info(void *fkeep, int64_t out[4]);
/* give the workspace back; the next call takes it again.  Return codes as spllt_hip_release_batch. */
int spllt_hip_release_solve_many_batch(void *fkeep);

#ifdef __cplusplus
}
#endif
#endif
