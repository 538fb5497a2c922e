/*
 * spllt_hip_batch_repro.h -- the bit-reproducible batch: a deterministic form of spllt_hip_factor_batch and of
 * every blocked sweep over the members of a batch.
 *
 * WHY A HEADER OF ITS OWN.  As spllt_hip_batch_solve_many.h: the recorded table of the entry ladder
 * (tests/capi_ladder.py and the two files under tests/golden/) is not regenerated for this family, so it is
 * declared here, bound by a table of its own (spllt_amd/_lib.py, _BATCH_REPRO) and checked against the recorded
 * rows of its siblings.  When the table is next regenerated these declarations are to be folded into the batch
 * section of spllt_hip.h, and this file goes.
 *
 * The header is self-contained; the handle is the fkeep of spllt_iface.h, the error codes are its
 * SPLLT_ERROR_* values (PARAMETER -10, NOT_POSDEF -20, HIP -30, UNIMPLEMENTED -98, ALLOCATION -1).
 */
#ifndef SPLLT_HIP_BATCH_REPRO_H
#define SPLLT_HIP_BATCH_REPRO_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the switch -------------------------------------------------------------------------------------------
 * on != 0: from now on
 *   - spllt_hip_factor_batch(_dev) runs the deterministic batch program ("batch_det_*" of spllt_hip_program_get):
 *     the product of every inter-node update unit is STORED in a per-member scratch and one gather launch per tree
 *     level subtracts the stored blocks from their destination tiles in table order -- no atomic add;
 *   - EVERY sweep over the members of a batch runs the reproducible blocked kernels: a strip stores its products,
 *     the diagonal launch that owns a row subtracts them in the order of the "batch_rsolve_*" tables.  That covers
 *     spllt_hip_solve_batch(_dev) (routed to the blocked path), spllt_hip_solve_many_batch(_dev), W_b and the sweeps
 *     of the constrained batch family, the precision kind of spllt_hip_sample_batch(_dev) and the preconditioner of
 *     spllt_hip_solve_refined_batch.
 * With the switch on the bits of a member's factor, log det and solutions depend on that member's values and
 * right-hand sides alone: not on the run, on nbatch, on the member's place in the batch, on the grid mapping or on
 * the split of the members into ranges; and the bits of a vector's solution do not depend on the block width, on
 * the vector's place in its block or on the other vectors.  They are NOT the bits of the default batch, and not
 * those of the single handle's deterministic factorization (engine flag 4096).
 * Flipping the switch keeps an existing batch (its factors stay what they are until the next
 * spllt_hip_factor_batch).  Off by default; with it off no entry point changes its launches or its results.
 * Returns the previous setting (0 or 1); SPLLT_ERROR_PARAMETER without an analysis; SPLLT_ERROR_UNIMPLEMENTED
 * when switched on on a partitioned handle. */
int spllt_hip_set_batch_reproducible(void *fkeep, int on);

/* ---- the reproducible sweep, whatever the switch says -----------------------------------------------------
 * Arguments, layout, jobs 0 / 1 / 2, return codes and the treatment of a member that is not positive definite as
 * spllt_hip_solve_many_batch(_dev).  Storage besides that call's workspace, taken on the first reproducible sweep:
 * the five tables and nbatch * rb * max(frows, bsize) doubles, rb = 32, or 16 when that does not fit (the blocks
 * are then 16 wide); SPLLT_ERROR_ALLOCATION keeps nothing and leaves the batch and every other solve usable. */
int spllt_hip_solve_repro_batch(void *fkeep, int nrhs, double *x_host, int64_t ldx, int job);
int spllt_hip_solve_repro_batch_dev(void *fkeep, int nrhs, double *x_dev, int64_t ldx, int job, int pivot_order);

/* out[0]: the switch; out[1]: 1 when the LAST batch was factorized by the deterministic program; out[2]: the
 * kernel launches of that factorization (0 otherwise); out[3]: the width of the last block of the last
 * reproducible sweep (0: none yet); out[4]: bytes of the factor scratch; out[5]: bytes of the sweep scratch.
 * out[1 .. 5] are zero on a handle without an engine. */
int spllt_hip_batch_repro_info(void *fkeep, int64_t out[6]);

/* give the sweep's scratch and tables back; the next reproducible sweep takes them again.  The factor scratch goes
 * with the batch (spllt_hip_release_batch).  Return codes as spllt_hip_release_batch. */
int spllt_hip_release_batch_repro(void *fkeep);

#ifdef __cplusplus
}
#endif
#endif
