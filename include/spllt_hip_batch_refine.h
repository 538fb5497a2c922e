/*
 * spllt_hip_batch_refine.h -- the device product A_b x and the refined solves for every member of a batch: the
 * batch twins of spllt_hip_matvec and spllt_hip_solve_refined of spllt_hip.h.
 *
 * WHY A HEADER OF ITS OWN.  The recorded table of the entry ladder (tests/capi_ladder.py and the two files
 * under tests/golden/) has one row per entry point of spllt_hip.h that takes a handle, and it is recorded
 * from the library of the commit BEFORE a change of the boundary.  This family was added without
 * regenerating that table, so it is declared here, bound by a table of its own (spllt_amd/_lib.py,
 * _BATCH_REFINE) and checked by a ladder of its own (tests/test_refine_batch_cpu.py,
 * tests/test_refine_batch_gpu.py), whose expected codes are the recorded rows of the siblings
 * spllt_hip_solve_batch(_dev), spllt_hip_matvec(_dev), spllt_hip_solve_refined(_dev) and
 * spllt_hip_release_batch.  When the table is next regenerated these declarations are to be folded into the
 * batch section of spllt_hip.h (together with those of the other spllt_hip_batch_*.h), with their rows in
 * tests/capi_ladder.py and their prototypes in _lib._HIP, and this file goes.
 *
 * The header is self-contained; the handle is the fkeep of spllt_iface.h, the error codes are its
 * SPLLT_ERROR_* values (PARAMETER -10, NOT_POSDEF -20, HIP -30, UNIMPLEMENTED -98, ALLOCATION -1).
 */
#ifndef SPLLT_HIP_BATCH_REFINE_H
#define SPLLT_HIP_BATCH_REFINE_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the product A_b x for nbatch value sets on the analysed pattern (single GPU) ---------
 * y_b = A_b x_b with A_b = (the analysed pattern, val[b*ldval .. + nnz)), ldval >= nnz, for b < nbatch, on the
 * device, in one set of launches for all members.  Vector q of member b is at x[(b*nvec + q)*ldx .. + n) and
 * y[(b*nvec + q)*ldy .. + n), ldx, ldy >= n: the layout of spllt_hip_solve_batch.  Nothing else is read or
 * written; x and y must not overlap.  pivot_order as spllt_hip_matvec_dev.  Member b's product is bit-identical
 * to spllt_hip_matvec called with val_b, and repeats bit-identically: every sum has a fixed order.  Needs neither
 * a factor nor a batch.  nbatch = 0 and nvec = 0 are no-ops that return 0.
 * Storage: the operator tables (those of spllt_hip_matvec, one copy for both) and -- unless the vectors are on the
 * device in pivot order -- a workspace of the product's own, nbatch * min(nvec, 32) * n doubles twice (three times for
 * the host entry point, plus nbatch * nnz for its values); when that does not fit the call returns
 * SPLLT_ERROR_ALLOCATION and every other call stays usable.  The solver's work arrays are not touched.  All of it goes
 * back with spllt_hip_release_refine_batch or spllt_hip_release_batch.
 * Errors: null handle or pointer, negative count, nnz not the pattern's, ldval < nnz, ldx / ldy < n ->
 * SPLLT_ERROR_PARAMETER; a partitioned handle -> SPLLT_ERROR_UNIMPLEMENTED; no device -> SPLLT_ERROR_HIP. */
int spllt_hip_matvec_batch(void *fkeep, int nbatch, int nnz, const double *val_host, int64_t ldval, int nvec,
                           const double *x_host, int64_t ldx, double *y_host, int64_t ldy);
int spllt_hip_matvec_batch_dev(void *fkeep, int nbatch, int nnz, const double *val_dev, int64_t ldval, int nvec,
                               const double *x_dev, int64_t ldx, double *y_dev, int64_t ldy, int pivot_order);

/* ---- refined solves for the members of the LAST batch ------------------------------------
 * What spllt_hip_solve_refined does, for all members at once: A_b x = b with A_b = (pattern, val_b), the factor
 * of member b of the last spllt_hip_factor_batch as M^-1, to the backward error tol.  The two uses are those of
 * the single handle: val = the values that were factorized recovers the accuracy the inverse-multiply panels
 * lose; val = values that have moved a little since reuses the factors.  method 0:
 * iterative refinement, 1: conjugate gradients preconditioned by the factor.  x: the right-hand sides on entry,
 * the solutions on exit (user order), vector q of member b at x[(b*nrhs + q)*ldx .. + n).
 * iterations[b*nrhs + q]: applications of the factor after the first; error[b*nrhs + q]: the backward error
 * |b - A x|_2 / (|b|_2 + max|a_ij| |x|_2) of a true residual, max|a_ij| being member b's.  Either may be NULL.  A
 * pair that does not reach tol in max_iter iterations, or meets a NaN, keeps its best confirmed iterate; a NaN in
 * val_b ends member b's vectors only, a NaN in a right-hand side that vector only.
 * The vectors go in passes of at most 32 per member; every launch of a pass carries all members, and the host
 * reads one array (error and state of every pair) per iteration.  M^-1 is spllt_hip_solve_many_batch_dev at every
 * count of vectors: measured, both sweeps of the blocked solve beat spllt_hip_solve_batch_dev from one vector per
 * member on (the threshold BRF_BLOCKED_MIN is 1, the environment variable
 * SPLLT_BRF_BLOCKED_MIN = N sends passes of fewer than N vectors per member through spllt_hip_solve_batch_dev);
 * spllt_hip_set_batch_blocked_solve is not consulted.  The sweeps know no member mask: a member whose vectors
 * have all converged rides along with zero columns until the last pair of the pass is done.
 *
 * Storage is taken from the handle's device pool on the first call, all or nothing: six work arrays of
 * nbatch * 32 * n doubles, the partial sums and the scalars; when that does not fit, passes of 16, then of 8.
 * When that does not fit either the call returns SPLLT_ERROR_ALLOCATION, keeps nothing, and the batch and every
 * other call stay usable.  The storage stays until spllt_hip_release_refine_batch, spllt_hip_release_batch or
 * spllt_deallocate_fkeep and is taken again when a later batch brings more members.  The operator tables are
 * those of spllt_hip_matvec: one copy serves both.
 *
 * A member that is not positive definite: nothing of it is read or written, its vectors stay bit-identical,
 * iterations = 0 and error = NaN for it, and the call returns SPLLT_ERROR_NOT_POSDEF after serving the others.
 * Return value: a negative code; else 0 when every pair reached tol, 1 when at least one did not.
 * Errors, the rungs of spllt_hip_solve_batch(_dev) and of spllt_hip_solve_refined in the same order: null
 * handle or pointer, negative count, nnz not the pattern's, ldval < nnz, ldx < n, bad method, tol <= 0,
 * max_iter < 0, no batch yet -> SPLLT_ERROR_PARAMETER; a partitioned handle -> SPLLT_ERROR_UNIMPLEMENTED; no
 * device -> SPLLT_ERROR_HIP.  nrhs = 0 is a no-op that returns 0. */
int spllt_hip_solve_refined_batch(void *fkeep, int nnz, const double *val_host, int64_t ldval, int nrhs, double *x_host,
                                  int64_t ldx, int method, double tol, int max_iter, int *iterations, double *error);
int spllt_hip_solve_refined_batch_dev(void *fkeep, int nnz, const double *val_dev, int64_t ldval, int nrhs, double *x_dev,
                                      int64_t ldx, int method, double tol, int max_iter, int *iterations, double *error);
/* out[0]: the pass width the storage holds (32, 16 or 8; 0 while none is held), out[1]: passes and out[2]: kernel
 * launches of the last spllt_hip_solve_refined_batch(_dev) -- those of this family and of the sweeps, whichever
 * route M^-1 took --, out[3]: bytes of the storage.  (The iterations of
 * the last call are its iterations[] array.)  Zeros on a handle without an engine. */
int spllt_hip_solve_refined_batch_info(void *fkeep, int64_t out[4]);
/* give the storage back; the next call takes it again.  Return codes as spllt_hip_release_batch. */
int spllt_hip_release_refine_batch(void *fkeep);

#ifdef __cplusplus
}
#endif
#endif
