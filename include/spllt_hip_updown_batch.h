/*
 * spllt_hip_updown_batch.h -- low-rank update / downdate of the factors of a batch: with L_b the factors of the
 * last spllt_hip_factor_batch, the members' arenas afterwards hold the factors of P (A_b + sign W_b W_b^T) P^T
 * (DESIGN.md section 28).  The batch twin of spllt_hip_updown (spllt_hip.h).
 *
 * WHY A HEADER OF ITS OWN.  As spllt_hip_batch_repro.h: the recorded table of the entry ladder
 * (tests/capi_ladder.py and the two files under tests/golden/) is not regenerated for this family, so it is
 * declared here, bound by a table of its own (spllt_amd/_lib.py, _BATCH_UPDOWN) and checked against the recorded
 * rows of its siblings.  When the table is next regenerated these declarations are to be folded into the batch
 * section of spllt_hip.h, and this file goes.
 *
 * The header is self-contained; the handle is the fkeep of spllt_iface.h, the error codes are its
 * SPLLT_ERROR_* values (PARAMETER -10, NOT_POSDEF -20, HIP -30, UNIMPLEMENTED -98, ALLOCATION -1).
 */
#ifndef SPLLT_HIP_UPDOWN_BATCH_H
#define SPLLT_HIP_UPDOWN_BATCH_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the modification ---------------------------------------------------------------------------------------
 * W_b has ONE pattern for all members: k sparse columns, wptr (k + 1) / wrow, CSC, 1-based, user variable order,
 * rows strictly increasing within a column -- exactly the arrays of spllt_hip_updown, with its admissibility rule
 * (the pattern of a column is a clique of the analysed matrix) and its host checks, all made before anything is
 * enqueued.  wptr / wrow are host arrays in both forms.  Each member has its OWN values: member b's value of CSC
 * position e (0-based, e < wptr[k] - 1) at wval[b * ldw + e], ldw >= wptr[k] - 1.  There is no nbatch argument: the
 * call reads the values of EVERY member of the last batch.  sign: +1 update, -1 downdate, for all members.
 *
 * It runs in place and in the layout of the batch: the arenas (spllt_hip_get_factor_batch) hold the new factors, the
 * inverted 64-wide diagonal panels are rebuilt, and every sweep over the batch (solve, blocked solve, products,
 * samplers, refined and constrained solves, log det) then works on the modified factors.  Afterwards the members'
 * selected inverses are stale and their factor adjoints unseeded; the constraints of the batch rebuild on their
 * next call; spllt_hip_factor_serial(fkeep, 1) has advanced.  The single factor and its features are not touched.
 *
 * Per pass of up to 8 columns the call makes one scatter launch, and per block column of the pass's plan
 * (spllt_hip_updown_plan: the pattern is shared, so is the plan) one launch of a workgroup per member plus, where
 * the block column has rows below its square, one launch of (strips x members) workgroups -- whatever nbatch.
 * A member whose values are zero on a block column's own columns skips that block column (it would be an
 * identity) and keeps its entries bit for bit: with a union pattern (leave-one-out: k columns, member b non-zero
 * in its own) every member pays for its own path, and a member whose values are all zero is untouched.
 *
 * Returns 0; SPLLT_ERROR_PARAMETER (message in spllt_hip_last_error) for a malformed or inadmissible column, a
 * sign other than +1 / -1, a null array, ldw too small, a value that is not finite (host form only: the _dev form
 * does not look at the values), or a handle without a batch -- every such refusal leaves all arenas bit for bit
 * alone; k = 0 and empty columns return 0.  A downdate that meets d^2 - w_j^2 <= 0 in member b flags that member
 * (spllt_hip_batch_status reports -20 and the 1-based pivot position) and goes on with r = d; the member is then
 * skipped by every batch call, as a member that failed in spllt_hip_factor_batch is, until the next
 * spllt_hip_factor_batch.  The call still serves the other members and returns SPLLT_ERROR_NOT_POSDEF (also when a
 * member was flagged before the call); a failure of this call is reported on stderr as well.
 * SPLLT_ERROR_ALLOCATION: nothing is kept, the batch and the single factor stay usable.  SPLLT_ERROR_UNIMPLEMENTED
 * on a partitioned handle.  A launch or a wait that fails mid-sweep (SPLLT_ERROR_HIP) leaves the handle without a
 * batch.
 *
 * Storage, taken in one transaction on the first call and kept until spllt_hip_release_batch or
 * spllt_hip_release_updown_batch: nbatch * (8 n + 24 * (widest block column)) doubles and nbatch words. */
int spllt_hip_updown_batch(void *fkeep, int k, const int *wptr, const int *wrow, const double *wval_host,
                           int64_t ldw, int sign);
int spllt_hip_updown_batch_dev(void *fkeep, int k, const int *wptr, const int *wrow, const double *wval_dev,
                               int64_t ldw, int sign);

/* of the last call: out[0] block columns visited, out[1] entries of L in them per member, out[2] kernel launches,
 * out[3] passes, out[4] members served (not flagged when the call began), out[5] members that failed in this call.
 * All zero after a call that was refused, that had nothing to do or that could not take its storage. */
int spllt_hip_updown_batch_info(void *fkeep, int64_t out[6]);

/* device time of the last call, from the first scatter to the last kernel, between HIP events (milliseconds) */
int spllt_hip_updown_batch_time(void *fkeep, double *device_ms);

/* give the work arrays, the coefficient scratch and the words back; the next call takes them again.  Return codes as
 * spllt_hip_release_batch. */
int spllt_hip_release_updown_batch(void *fkeep);

#ifdef __cplusplus
}
#endif
#endif
