/*
 * spllt_hip_batch_adjoint.h -- the reverse-mode derivative of the factors of a batch: the batch twin of
 * spllt_hip_factor_adjoint* of spllt_hip.h.
 *
 * WHY A HEADER OF ITS OWN.  The recorded table of the entry ladder (tests/capi_ladder.py and the two files
 * under tests/golden/) has one row per entry point of spllt_hip.h that takes a handle, and it is recorded
 * from the library of the commit BEFORE a change of the boundary.  This family was added without
 * regenerating that table, so it is declared here, bound by a table of its own (spllt_amd/_lib.py,
 * _BATCH_ADJOINT) and checked by a ladder of its own (tests/batch_adjoint_ladder.py, driven by
 * tests/test_batch_adjoint_cpu.py and tests/test_batch_adjoint_gpu.py), whose expected codes are the recorded
 * rows of the siblings spllt_hip_factor_adjoint*, spllt_hip_selected_inverse_batch,
 * spllt_hip_get_inverse_batch and spllt_hip_release_inverse_batch.  When the table is next regenerated these
 * declarations are to be folded into the batch section of spllt_hip.h (together with those of
 * spllt_hip_batch_mult.h and spllt_hip_batch_solve_many.h), with their rows in tests/capi_ladder.py and their
 * prototypes in _lib._HIP, and this file goes.
 *
 * The header is self-contained; the handle is the fkeep of spllt_iface.h, the error codes are its
 * SPLLT_ERROR_* values (PARAMETER -10, NOT_POSDEF -20, HIP -30, UNIMPLEMENTED -98, ALLOCATION -1).
 */
#ifndef SPLLT_HIP_BATCH_ADJOINT_H
#define SPLLT_HIP_BATCH_ADJOINT_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- factor adjoint of the members of a batch (single GPU) ---------------------------------
 * For every member b of the LAST batch (spllt_hip_factor_batch) there is one more arena G_b with the layout of
 * spllt_hip_get_factor_batch.  It is seeded with d loss / d L_b on the lower positions of the factor; the sweep
 * turns it into d loss / d (P A_b P^T) on every stored lower position (a stored lower entry standing for both
 * a_ij and a_ji) and reads the entries of the analysed pattern out in the order of val.  What the calls compute
 * per member is what spllt_hip_factor_adjoint* compute for one matrix; every launch carries all members, so the
 * number of launches does not depend on nbatch (unless a grid would overflow and the members are split into
 * ranges).  A step of the sweep is three launches; with spllt_hip_debug("batch_fadj_fused=1") a step whose panels
 * all have at most 64 rows below them is ONE launch that gives the same numbers (off by default: DESIGN.md section
 * 23 has the measurement).  No atomics: two sweeps over the same factors and seeds give the same bits, and a
 * member's bits do not depend on the other members.
 *
 * STATES, for the whole batch: unseeded -> seeded -> swept.  A seed with accumulate = 0 or
 * spllt_hip_set_factor_adjoint_batch makes the arenas seeded; accumulate = 1 needs seeded arenas; the sweep needs
 * freshly seeded arenas (a second sweep is refused); spllt_hip_get_factor_adjoint_batch needs seeded or swept
 * arenas; spllt_hip_factor_batch(_dev) makes them unseeded.  Every refusal happens before anything is enqueued.
 * The adjoint arena of the single factor (spllt_hip_factor_adjoint*) and its state are not touched.
 *
 * STORAGE.  nbatch arenas and the step scratch are taken from the handle's device pool on first use, all or
 * nothing: when they do not fit the call returns SPLLT_ERROR_ALLOCATION, keeps nothing, and the batch, its solves
 * and its selected inversion stay usable.  They are taken again for a larger nbatch and stay until
 * spllt_hip_release_factor_adjoint_batch, spllt_hip_release_batch or spllt_deallocate_fkeep.  Program tables and
 * step scratch are shared with spllt_hip_selected_inverse_batch (the last of the two releases returns the
 * scratch); the inverse arenas are separate: an adjoint run between two readers of the inverse changes nothing.
 *
 * A member that is not positive definite is skipped by every launch: nothing of it is read or written, its row of
 * gval is NaN, the sweep returns SPLLT_ERROR_NOT_POSDEF and the other members are served.
 *
 * All work is ordered on spllt_hip_engine_stream and finished when a call returns.
 *
 * Errors, the rungs of spllt_hip_factor_adjoint* plus "no batch yet", in the order of
 * spllt_hip_selected_inverse_batch: null handle or pointer, nvec < 0, ld < n, ldout < nnz, ldarena < arena,
 * count < 0, accumulate not 0 / 1, order_flags not 0 .. 3, no batch yet, a state that does not allow the call
 * -> SPLLT_ERROR_PARAMETER; a handle after spllt_hip_set_partition with nranks > 1 -> SPLLT_ERROR_UNIMPLEMENTED;
 * no device -> SPLLT_ERROR_HIP.  Messages: spllt_hip_last_error. */

/* G_b (+)= alpha * sum_q a_bq b_bq^T on the lower positions of every member b.  Vector q of member b is at
 * a[(b*nvec + q)*ld .. + n), b likewise: the layout of spllt_hip_solve_batch_dev.  order_flags bit 0 / bit 1: a / b
 * is in pivot order (else in the user's variable order).  Per entry ONE fma chain over q ascending, alpha applied
 * once: the _dev call writes, for member b, the bits spllt_hip_factor_adjoint_seed_dev writes for that member's
 * vectors.  The host call stages its vectors in groups of at most 32 per member, each group one such call (the
 * later ones accumulating).  nvec = 0 with accumulate = 0 zeroes the arenas. */
int spllt_hip_factor_adjoint_seed_batch_dev(void *fkeep, int nvec, const double *a_dev, const double *b_dev,
                                            int64_t ld, double alpha, int accumulate, int order_flags);
int spllt_hip_factor_adjoint_seed_batch(void *fkeep, int nvec, const double *a_host, const double *b_host,
                                        int64_t ld, double alpha, int accumulate, int order_flags);
/* an arbitrary seed for ALL members: member b's arena (the layout of spllt_hip_get_factor_batch) at
 * host_arenas + b*ldarena, ldarena >= arena */
int spllt_hip_set_factor_adjoint_batch(void *fkeep, const double *host_arenas, int64_t ldarena);
/* the first min(count, arena) doubles of member's adjoint arena, seeded or swept */
int spllt_hip_get_factor_adjoint_batch(void *fkeep, int member, double *out, int64_t count);
/* the arenas on the device (member b at + b * *member_stride doubles); null and stride 0 while unseeded */
double *spllt_hip_device_factor_adjoint_batch(void *fkeep, int64_t *member_stride);
/* the sweep and the reader: gval[b*ldout + k] = d loss / d val_b[k], ldout >= nnz */
int spllt_hip_factor_adjoint_batch_dev(void *fkeep, double *gval_dev, int64_t ldout);
int spllt_hip_factor_adjoint_batch(void *fkeep, double *gval_host, int64_t ldout);
/* kernel launches of the last sweep, the reader included, the seed not; 0 when there was none */
int spllt_hip_batch_adjoint_launches(void *fkeep);
/* give the arenas back (and the step scratch, unless the batched inversion holds it); return codes as
 * spllt_hip_release_inverse_batch */
int spllt_hip_release_factor_adjoint_batch(void *fkeep);

#ifdef __cplusplus
}
#endif
#endif
