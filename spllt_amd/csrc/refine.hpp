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

}  // namespace spx
