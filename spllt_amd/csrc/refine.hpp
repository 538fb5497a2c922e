// Launchers of refine.hip: the symmetric sparse matrix-vector product on the analysed pattern and the
// fused vector kernels of the refined solves (iterative refinement, factor-preconditioned CG).
//
// Work vectors are vector-major in pivot order, v[q * ld + p]: the layout spllt_hip_solve_dev (ld = n) and
// spllt_hip_solve_many_dev(..., pivot_order = 1) take.  Every scalar of the iteration lives on the device:
//
//   ds (doubles): alpha[G] beta[G] rz[G] bnorm[G] ebest[G] out[2 G] amax     (RF_DS doubles)
//   is (ints):    st[G] decl[G] restart[G] improve[G]                         (RF_IS ints)
//
// st: 0 iterating, 1 converged, 2 failed (a NaN or an infinity); a vector whose st is not 0 is frozen: no
// kernel writes it any more.  decl: declared converged on the recurrence residual, to be confirmed with a
// true one.  out[q] = best confirmed error, out[G + q] = st: the one array the host reads per iteration.
//
// Reductions are two-stage: every workgroup stores its partial sums (part[(slot * 2 + which) * G + q]),
// k_rf_finalize adds them in a fixed order.  No atomics anywhere.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace spx {

constexpr int RF_G = 32;          // vectors of a group (the block of the blocked solve)
constexpr int RF_NV = 8;          // vectors that share one read of a row's col / src / val streams
constexpr int RF_VROWS = 1024;    // rows per workgroup of the vector kernels
constexpr int RF_AMAX_WG = 256;   // workgroups of the max |val| kernel
constexpr int RF_DS = 7 * RF_G + 1, RF_IS = 4 * RF_G;
enum RfDs { RFD_ALPHA = 0, RFD_BETA = RF_G, RFD_RZ = 2 * RF_G, RFD_BNORM = 3 * RF_G, RFD_EBEST = 4 * RF_G,
            RFD_OUT = 5 * RF_G, RFD_AMAX = 7 * RF_G };
enum RfIs { RFI_ST = 0, RFI_DECL = RF_G, RFI_RESTART = 2 * RF_G, RFI_IMPROVE = 3 * RF_G };
enum RfStage { RFS_AMAX = 0, RFS_BNORM, RFS_TRUE, RFS_ALPHA, RFS_REC, RFS_BETA, RFS_FINAL };

// the operator on the device: rows sorted into three classes by their length (4, 16 or 64 lanes per row)
struct RfOperator {
  const int64_t* rowptr;
  const int* col;
  const int* src;
  const int* rows;      // the rows of class 0, then of class 1, then of class 2
  int nrows[3];
};

// workgroups (= partial slots) of one product
int spmv_slots(const RfOperator& op);
// y = A x (b = null) or y = b - A x, nvec vectors; a vector q takes part when sel == null or sel[q] == want.
// part != null: partials x.y (which 0) of the plain product; |y|^2 (which 0) and |x|^2 (which 1) of the residual.
// x and y must not overlap.  b has y's leading dimension: vector q of b starts at b + q * ldy.
void launch_spmv(hipStream_t st, const RfOperator& op, const double* val, const double* x, int64_t ldx,
                 const double* b, double* y, int64_t ldy, int nvec, const int* sel, int want, double* part);

int vec_slots(int n);
// x += alpha p (alpha = null: 1) and, with q != null, r -= alpha q; partials |r|^2, |x|^2 (part may be null)
void launch_rf_axpy(hipStream_t st, int n, int nvec, const double* alpha, double* x, const double* p, double* r,
                    const double* q, const int* sel, int want, double* part);
// p = z + beta p (beta == 0: p = z, whatever p held)
void launch_rf_pupdate(hipStream_t st, int n, int nvec, const double* beta, double* p, const double* z,
                       const int* sel, int want);
// partials a.b (which 0)
void launch_rf_dot(hipStream_t st, int n, int nvec, const double* a, const double* b, const int* sel, int want,
                   double* part);
// dst = src for the selected vectors; zero_others: the other vectors of dst are set to 0 (a work column that the
// substitution sweeps although its vector is frozen then stays 0 instead of growing from sweep to sweep)
void launch_rf_copy(hipStream_t st, int n, int nvec, double* dst, const double* src, const int* sel, int want,
                    bool zero_others = false);
// part[slot] = max |val| of the slot's share, a NaN wins (RF_AMAX_WG slots)
void launch_rf_absmax(hipStream_t st, const double* val, int64_t nnz, double* part);
// second stage of every reduction and the scalar step that follows it (one workgroup)
void launch_rf_finalize(hipStream_t st, int stage, const double* part, int nslots, int nvec, double tol, int pcg,
                        double* ds, int* is);

// ---- the same for the members of a batch (batch_refine.hip) --------------------------------------------
// One pass serves nv <= RF_G vectors of each of nbatch members.  Work vectors are member-major, vector-major in
// pivot order, v[(b * nv + q) * n + p]: the layout spllt_hip_solve_batch_dev(nrhs = nv, ldx = n, pivot_order = 1)
// takes.  The pair (member b, vector q) has the index g = b * nv + q; with np = nbatch * nv pairs in the pass
//
//   ds (doubles): alpha[np] beta[np] rz[np] bnorm[np] ebest[np] out[2 np]      (BRF_DS * np doubles)
//   is (ints):    st[np] decl[np] restart[np] improve[np]                      (RF_IS / RF_G * np ints)
//   amax[b]:      max |a_ij| of member b (an array of its own: it outlives the passes of a call)
//   sigma[b]:     2^-exponent(amax[b]): |b|^2 and |r|^2 are summed over sigma-scaled entries and bnorm is
//                 sigma |b| (rf_body.hpp), so that a member scaled by 2^600 does not overflow its squares
//
// out[g] = best confirmed error, out[np + g] = st: the one array the host reads per iteration.  The partial sums of
// a workgroup go to part[(slot * 2 + which) * np + g]: the layout of the single handle with np in place of RF_G.
// flag (may be null): the flags of the batch; a member whose flag is not INT_MAX is skipped by every kernel --
// nothing of it is read or written; the finalize of RFS_BNORM gives its pairs the state 2.
constexpr int BRF_DS = 7;
// vectors per member in a pass from which on M^-1 is the blocked batch solve.  Measured: both
// sweeps of the blocked solve beat solve_batch at EVERY count, 1 included (0.62-0.87 of its time at one vector), so
// the threshold is 1; solve_batch stays reachable through SPLLT_BRF_BLOCKED_MIN.
constexpr int BRF_BLOCKED_MIN = 1;
struct BrfView {
  const int* flag;
  int nbatch, nv;
  double* amax;
  double* sigma;
  double* ds;
  int* is;
  double* part;
  int np() const { return nbatch * nv; }
  double* alpha() const { return ds; }
  double* beta() const { return ds + np(); }
  double* out() const { return ds + 5 * (int64_t)np(); }
  const int* st() const { return is; }
  const int* decl() const { return is + np(); }
  const int* improve() const { return is + 3 * (int64_t)np(); }
};
// the sum of the launch counts of several launchers; fits turns false once one of them returned -1
struct BrfTally {
  int64_t n = 0;
  bool fits = true;
  void add(int k) { if (k < 0) fits = false; else n += k; }
  int count() const { return fits ? (int)n : -1; }
};
// Every launcher returns the number of launches it made (the members are split into ranges when a grid would pass
// batch_grid_limit() workgroups), or -1, nothing launched, when ONE member's work items overflow a grid.
// y_b = A_b x_b (b = null) or y_b = b_b - A_b x_b with A_b = (pattern, val + b * ldval); vector q of member b at
// x + b * xstride + q * ldx (y and b: ystride, ldy).  sel (may be null) is indexed by the pair; part as launch_spmv.
int launch_bspmv(hipStream_t st, const RfOperator& op, const BrfView& v, const double* val, int64_t ldval,
                 const double* x, int64_t xstride, int64_t ldx, const double* b, double* y, int64_t ystride, int64_t ldy,
                 const int* sel, int want, bool partials);
// the vector kernels on work vectors (the layout above); alpha / beta are indexed by the pair
int launch_brf_axpy(hipStream_t st, const BrfView& v, int n, const double* alpha, double* x, const double* p, double* r,
                    const double* q, const int* sel, int want, bool partials);
int launch_brf_pupdate(hipStream_t st, const BrfView& v, int n, const double* beta, double* p, const double* z,
                       const int* sel, int want);
// (residual_like: both factors are of the size of a right-hand side -- |b|^2 -- and are scaled by sigma)
int launch_brf_dot(hipStream_t st, const BrfView& v, int n, const double* a, const double* b, const int* sel, int want,
                   bool residual_like);
int launch_brf_copy(hipStream_t st, const BrfView& v, int n, double* dst, const double* src, const int* sel, int want,
                    bool zero_others = false);
// caller's vectors x[b * xstride + q * ldx + i] <-> work vectors W[(b * nv + q) * n + order[i]] (order = null: i)
int launch_brf_permute(hipStream_t st, const BrfView& v, bool unpack, double* x, int64_t xstride, int64_t ldx,
                       const int* order, int n, double* W);
// amax[b] = max |val_b| (a NaN wins), through v.part (nbatch * RF_AMAX_WG doubles): two launches per range
int launch_brf_absmax(hipStream_t st, const BrfView& v, const double* val, int64_t ldval, int64_t nnz);
// second stage of every reduction and the scalar step that follows it: one workgroup per member
int launch_brf_finalize(hipStream_t st, const BrfView& v, int stage, int nslots, double tol, int flag);

}  // namespace spx
