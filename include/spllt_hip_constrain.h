/*
 * spllt_hip_constrain.h -- hard linear constraints C x = e on the field of the current factor: conditioned solves,
 * samples and marginal variances (spllt_amd/csrc/constrain.hip).
 *
 * WHY A HEADER OF ITS OWN.  As spllt_hip_batch_refine.h: the recorded table of the entry ladder (tests/capi_ladder.py
 * and the two files under tests/golden/) has one row per entry point of spllt_hip.h and is recorded from the library
 * of the commit BEFORE a change of the boundary.  This family was added without regenerating that table, so it is
 * declared here, bound by a table of its own (spllt_amd/_lib.py, _CONSTRAIN) and checked by a ladder of its own
 * (tests/constrain_ladder.py), whose expected codes are the recorded rows of the siblings
 * spllt_hip_solve_many(_dev) (the vector arguments), spllt_hip_solve_refined(_dev) (the accepted call: a factorization
 * has to have been enqueued), spllt_hip_inverse_diag, spllt_hip_solve_sparse_info and spllt_hip_release_solve_repro.
 *
 * THE MATHEMATICS, all in user variable order.  A: the matrix of the current factor.  C: k x n, k <= 64 dense rows.
 *   W = A^-1 C^T (n x k),  S = C W (k x k, SPD iff C has full row rank),  S = G G^T,  U = W G^-T (n x k).
 *   correction of x towards C x = e:   r = C x - e,  t = G^-1 r,  x* = x - U t,  lambda = G^-T t = S^-1 r
 *   constrained solve:                 x* = correct(A^-1 b); (x*, lambda) solves A x + C^T lambda = b, C x = e
 *   constrained sample of N(mu, A^-1) | C x = e:   correct(mu + P^T L^-T z)
 *   constrained marginal variances:    Var(x_i | C x = e) = (A^-1)_ii - sum_j U[i, j]^2
 * C and U (k n doubles each), G, the partial sums of the products and two scalars stay on the device.
 *
 * LAYOUT.  Vectors as spllt_hip_solve_many: vector q at x[q*ldx .. q*ldx + n), ldx >= n; C the same: row i at
 * c[i*ldc .. i*ldc + n), ldc >= n.  Nothing outside those ranges is read or written.
 *
 * A LATER FACTOR IS PICKED UP.  C stays stored; U, G and the scalars belong to ONE factor (the serial behind
 * spllt_hip_factor_serial).  After spllt_factor, spllt_hip_factor_dev or a successful spllt_hip_updown the first call
 * that needs them rebuilds them: one blocked solve of k columns plus the small kernels.  Numbers of the old factor
 * are never returned.  A factor that failed (-20, or invalid after a failed downdate) gives what the solves give
 * in that state.
 *
 * DEPENDENT CONSTRAINTS.  The Cholesky factorization of S stops at the first j with pivot_j <= 2^-26 S_jj (the square
 * root of the machine precision: below it the conditioned quantities have lost half their digits) or with a pivot
 * that is not finite.  The call returns SPLLT_ERROR_NOT_POSDEF with a message that names row j (1-based); the handle
 * then holds NO constraints; the factor and every other call stay usable.
 *
 * WHICH SOLVE.  With spllt_hip_set_reproducible_solve on, W and the sample go through spllt_hip_solve_repro_dev,
 * otherwise through spllt_hip_solve_many_dev.  The kernels of this family use no atomic add: every sum has a fixed
 * order that depends neither on nvec, nor on the vector's place in its pass of at most 32, nor on the entry point.
 *
 * ERRORS, in the order of the entry ladder: null handle or pointer, k < 0, k > 64, ldc < n, a negative count,
 * ldx < n, 0 < lde < k, ldl < k with lambda given, nothing factorized, no constraints set -> SPLLT_ERROR_PARAMETER;
 * a partitioned handle -> SPLLT_ERROR_UNIMPLEMENTED; no device memory -> SPLLT_ERROR_ALLOCATION with nothing kept
 * half-allocated.  The work is ordered on the engine's stream and has finished when a call returns.
 *
 * The header is self-contained; the handle is the fkeep of spllt_iface.h, the error codes are its SPLLT_ERROR_*
 * values (PARAMETER -10, NOT_POSDEF -20, HIP -30, UNIMPLEMENTED -98, ALLOCATION -1).
 */
#ifndef SPLLT_HIP_CONSTRAIN_H
#define SPLLT_HIP_CONSTRAIN_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* stores C and computes W (the blocked solve), S, G, U, log det S and the smallest relative pivot for the current
 * factor.  1 <= k <= 64; k = 0 clears the constraints (c is then not read and may be null). */
int spllt_hip_set_constraints(void *fkeep, int k, const double *c_host, int64_t ldc);
int spllt_hip_set_constraints_dev(void *fkeep, int k, const double *c_dev, int64_t ldc);

/* the correction, in place.  e: null (zeros); lde = 0: one column of k targets shared by all vectors; else vector q's
 * targets at e[q*lde .. + k), lde >= k.  lambda: null, or k multipliers per vector at lambda[q*ldl .. + k), ldl >= k.
 * nvec = 0 is a no-op. */
int spllt_hip_constrain(void *fkeep, int nvec, double *x_host, int64_t ldx, const double *e_host, int64_t lde,
                        double *lambda_host, int64_t ldl);
int spllt_hip_constrain_dev(void *fkeep, int nvec, double *x_dev, int64_t ldx, const double *e_dev, int64_t lde,
                            double *lambda_dev, int64_t ldl);

/* spllt_hip_solve_many_dev (job 0) on the right-hand sides in x, then the correction */
int spllt_hip_solve_constrained(void *fkeep, int nrhs, double *x_host, int64_t ldx, const double *e_host, int64_t lde,
                                double *lambda_host, int64_t ldl);
int spllt_hip_solve_constrained_dev(void *fkeep, int nrhs, double *x_dev, int64_t ldx, const double *e_dev, int64_t lde,
                                    double *lambda_dev, int64_t ldl);

/* the kind-0 path of spllt_hip_sample(_dev) -- same noise, same mean handling --, then the correction.  e: k shared
 * targets or null. */
int spllt_hip_sample_constrained(void *fkeep, int nsamp, double *x_host, int64_t ldx, uint64_t seed,
                                 uint64_t first_sample, const double *mean_host, const double *e_host);
int spllt_hip_sample_constrained_dev(void *fkeep, int nsamp, double *x_dev, int64_t ldx, uint64_t seed,
                                     uint64_t first_sample, const double *mean_dev, const double *e_dev);

/* out[i] = (A^-1)_ii - sum_j U[i, j]^2 (host, user order).  Needs a valid selected inverse and fails like
 * spllt_hip_inverse_diag when there is none or it is stale. */
int spllt_hip_inverse_diag_constrained(void *fkeep, double *out, int n);

/* out[0]: k (0: none set), out[1]: rebuilds of U so far (the first build included), out[2]: device bytes held,
 * out[3]: kernel launches of this family in the last call.  stat[0]: log det S, stat[1]: the smallest pivot_j / S_jj.
 * Zeros on a handle without an engine or without constraints. */
int spllt_hip_constraints_info(void *fkeep, int64_t out[4], double stat[2]);

/* everything back to the pool, C forgotten.  Return codes as spllt_hip_release_solve_repro. */
int spllt_hip_release_constraints(void *fkeep);

#ifdef __cplusplus
}
#endif
#endif
