/*
 * spllt_hip_solve_sparse_batch.h -- sparse right-hand sides, selected outputs and B^T A_b^-1 B for the members of
 * a batch: with L_b the factors of the last spllt_hip_factor_batch (also after spllt_hip_updown_batch), a few entries
 * of A_b^-1 B for a sparse B, and the k x k matrices B^T A_b^-1 B.  The batch twin of
 * spllt_hip_solve_sparse / spllt_hip_gram_sparse (spllt_hip.h).
 *
 * WHY A HEADER OF ITS OWN.  As spllt_hip_updown_batch.h: the recorded table of the entry ladder
 * (tests/capi_ladder.py and the two files under tests/golden/) is not regenerated for this family, so it is
 * declared here, bound by a table of its own (spllt_amd/_lib.py, _SOLVE_SPARSE_BATCH) and checked against the
 * recorded rows of its siblings.  When the table is next regenerated these declarations are to be folded into the
 * batch section of spllt_hip.h, and this file goes.
 *
 * The header is self-contained; the handle is the fkeep of spllt_iface.h, the error codes are its
 * SPLLT_ERROR_* values (PARAMETER -10, NOT_POSDEF -20, HIP -30, UNIMPLEMENTED -98, ALLOCATION -1).
 */
#ifndef SPLLT_HIP_SOLVE_SPARSE_BATCH_H
#define SPLLT_HIP_SOLVE_SPARSE_BATCH_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the right-hand sides ------------------------------------------------------------------------------------
 * B has ONE pattern for all members: k sparse columns, bptr (k + 1) / brow, CSC, 1-based, user variable order, rows
 * strictly increasing within a column -- exactly the arrays of spllt_hip_solve_sparse, with its host checks, all
 * made before anything is enqueued.  bptr / brow / bval / sel are host arrays in every form.  Values: ldb = 0 is one
 * set for every member, bval[e] for CSC position e (0-based, e < bptr[k] - 1); ldb >= bptr[k] - 1 gives member b its
 * own, bval[b * ldb + e].  There is no nbatch argument: the call serves EVERY member of the last batch.
 * sel / nsel / job as in spllt_hip_solve_sparse: the wanted user variables (1-based, any order, duplicates allowed;
 * sel null or nsel < 0: all n entries), job 0 A_b^-1 B, 1 L_b^-1 P B, 2 L_b^-T of P B restricted to the closure of
 * the wanted rows.
 *
 * Output: column q of member b at wanted entry t is x[(b * k + q) * ldx + t], ldx >= nsel (>= n when all entries
 * are wanted); nothing else is written.  The pattern is shared, so one host plan, one filtered substitution program
 * (the batch's own) and one upload per group of 32 columns serve every member, and every kernel launch carries all
 * members: the number of launches does not depend on the number of members.  The sweeps add with fp64 atomics, as
 * the blocked batch solve does: results repeat to rounding.
 *
 * Returns 0; SPLLT_ERROR_PARAMETER (message in spllt_hip_last_error) for a malformed column or sel, a null array, a
 * job other than 0 / 1 / 2, ldb neither 0 nor >= bptr[k] - 1, ldx too small, or a handle without a batch -- every
 * refusal is decided on the host and leaves the outputs untouched; k = 0 and nsel = 0 return 0.  A member that is
 * not positive definite (flagged by the factorization or by a failed downdate) gets NaN in all of its outputs; the
 * call still serves the others and then returns SPLLT_ERROR_NOT_POSDEF.  SPLLT_ERROR_UNIMPLEMENTED on a partitioned
 * handle, and while spllt_hip_set_batch_reproducible is on (the filtered sweeps would break its promise).
 * SPLLT_ERROR_ALLOCATION: nothing of this feature stays allocated, the batch and every other call stay usable. */
int spllt_hip_solve_sparse_batch(void *fkeep, int k, const int *bptr, const int *brow, const double *bval, int64_t ldb,
                                 int nsel, const int *sel, double *x_host, int64_t ldx, int job);
int spllt_hip_solve_sparse_batch_dev(void *fkeep, int k, const int *bptr, const int *brow, const double *bval,
                                     int64_t ldb, int nsel, const int *sel, double *x_dev, int64_t ldx, int job);

/* G_b = B_b^T A_b^-1 B_b for every member, by forward sweeps only: k x k, column-major, both triangles, exactly
 * symmetric, at g + b * k * ldg, ldg >= k.  Arguments, return codes and flagged members as above. */
int spllt_hip_gram_sparse_batch(void *fkeep, int k, const int *bptr, const int *brow, const double *bval, int64_t ldb,
                                double *g_host, int64_t ldg);
int spllt_hip_gram_sparse_batch_dev(void *fkeep, int k, const int *bptr, const int *brow, const double *bval,
                                    int64_t ldb, double *g_dev, int64_t ldg);

/* of the last call: out[0..5] the fields of spllt_hip_solve_sparse_info -- block columns of the forward / backward
 * sweep, entries of L in them (per member), kernel launches, workgroups of the sweeps summed over the members --
 * out[6] members served, out[7] members flagged.  All zero after a call that was refused or had nothing to do. */
int spllt_hip_solve_sparse_batch_info(void *fkeep, int64_t out[8]);

/* give the staged tables, the output buffer and the workspaces of the products back; the next call takes them
 * again.  Return codes as spllt_hip_release_batch (which returns this storage too). */
int spllt_hip_release_solve_sparse_batch(void *fkeep);

#ifdef __cplusplus
}
#endif
#endif
