// Refined solves on gfx950: the operator A on the analysed pattern and the vector kernels around the
// existing substitution programs (refine.hpp has the layouts).
//
//   k_spmv<LPR, RES>   Y = A X or Y = B - A X on the gather-only CSR of P A P^T (rowptr / col / src): LPR = 4, 16
//                      or 64 lanes share a row (rows of at most 16 / at most 128 / more entries), RF_NV vectors
//                      share one read of the row's col / src / val streams; fixed summation order per row
//   k_rf_axpy          x += alpha p, r -= alpha q, partials of |r|^2 and |x|^2
//   k_rf_pupdate       p = z + beta p
//   k_rf_dot           partials of a.b
//   k_rf_copy (optionally zeroing the vectors it does not copy), k_rf_absmax
//   k_rf_finalize      the second stage of every reduction and the scalar arithmetic behind it
//
// alpha, beta and the per-vector state are read from device memory; a vector that is not selected is
// neither read for its result nor written.  No atomics: every sum has a fixed order.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "refine.hpp"
#include "rf_body.hpp"

namespace spx {

// ---------------------------------------------------------------------------------------------------
// rows[first .. first + nrows) of one length class; workgroup = 4 wavefronts x (64 / LPR) rows, grid.y =
// chunk of RF_NV vectors (the row body: rf_body.hpp).  The kernels of this file pass the literal 1.0 for the
// bodies' scale `sc`: after inlining the products with it fold away (x * 1.0 is x for every x, NaN and signed zero
// included), so the arithmetic is what it was before the bodies were shared; tests/test_refine_gpu.py pins it.
// ---------------------------------------------------------------------------------------------------
template <int LPR, bool RES>
__global__ __launch_bounds__(256) void k_spmv(const int* __restrict__ rows, int nrows, const int64_t* __restrict__ rowptr,
                                              const int* __restrict__ col, const int* __restrict__ src,
                                              const double* __restrict__ val, const double* __restrict__ x, int64_t ldx,
                                              const double* __restrict__ b, double* __restrict__ y, int64_t ldy, int nvec,
                                              const int* __restrict__ sel, int want, double* __restrict__ part,
                                              int slot0) {
  __shared__ double red[4][2 * RF_NV];
  const int q0 = blockIdx.y * RF_NV;
  const int nq = min(RF_NV, nvec - q0);
  unsigned act = 0;
  for (int j = 0; j < nq; ++j)
    if (rf_selected(sel, want, q0 + j)) act |= 1u << j;
  if (!act) return;   // (the same for every thread of the workgroup)
  rf_spmv_body<LPR, RES>((int)blockIdx.x, q0, nq, act, rows, nrows, rowptr, col, src, val, x, ldx, b, y, ldy,
                         part ? part + ((int64_t)(slot0 + blockIdx.x) * 2) * RF_G : nullptr, RF_G, 1.0, red);
}

// ---------------------------------------------------------------------------------------------------
// vector kernels: grid (ceil(n / RF_VROWS), nvec), thread t takes rows i0 + t + 256 k
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_rf_axpy(int n, const double* __restrict__ alpha, double* __restrict__ x,
                                                 const double* __restrict__ p, double* __restrict__ r,
                                                 const double* __restrict__ qv, const int* __restrict__ sel, int want,
                                                 double* __restrict__ part) {
  const int q = blockIdx.y;
  if (!rf_selected(sel, want, q)) return;
  const double a = alpha ? alpha[q] : 1.0;
  const int64_t base = (int64_t)q * n;
  double rr, xx;
  rf_axpy_body(n, (int)blockIdx.x, a, x + base, p + base, r ? r + base : nullptr, qv ? qv + base : nullptr, 1.0, rr, xx);
  if (part) rf_block_sum2(rr, xx, part + ((int64_t)blockIdx.x * 2) * RF_G + q, RF_G);
}

__global__ __launch_bounds__(256) void k_rf_pupdate(int n, const double* __restrict__ beta, double* __restrict__ p,
                                                    const double* __restrict__ z, const int* __restrict__ sel,
                                                    int want) {
  const int q = blockIdx.y;
  if (!rf_selected(sel, want, q)) return;
  const int64_t base = (int64_t)q * n;
  rf_pupdate_body(n, (int)blockIdx.x, beta[q], p + base, z + base);
}

__global__ __launch_bounds__(256) void k_rf_dot(int n, const double* __restrict__ a, const double* __restrict__ b,
                                                const int* __restrict__ sel, int want, double* __restrict__ part) {
  const int q = blockIdx.y;
  if (!rf_selected(sel, want, q)) return;
  const int64_t base = (int64_t)q * n;
  const double s = rf_dot_body(n, (int)blockIdx.x, a + base, b + base, 1.0);
  rf_block_sum2(s, 0.0, part + ((int64_t)blockIdx.x * 2) * RF_G + q, RF_G);
}

__global__ __launch_bounds__(256) void k_rf_copy(int n, double* __restrict__ dst, const double* __restrict__ src,
                                                 const int* __restrict__ sel, int want, int zero_others) {
  const int q = blockIdx.y;
  const bool mine = rf_selected(sel, want, q);
  if (!mine && !zero_others) return;
  const int64_t base = (int64_t)q * n;
  rf_copy_body(n, (int)blockIdx.x, mine, dst + base, src + base);
}

__global__ __launch_bounds__(256) void k_rf_absmax(const double* __restrict__ val, int64_t nnz, double* __restrict__ part) {
  __shared__ double red[4];
  rf_absmax_body(val, nnz, (int)blockIdx.x, (int)gridDim.x, part + blockIdx.x, red);
}

// ---------------------------------------------------------------------------------------------------
// One workgroup of 256: the second stage of a reduction (rf_second_stage), then thread q does the scalar step
// of vector q.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_rf_finalize(int stage, const double* __restrict__ part, int nslots, int nvec,
                                                     double tol, int flag, double* __restrict__ ds, int* __restrict__ is) {
  __shared__ double red[2][8][RF_G];
  __shared__ double mred[256];
  const int t = threadIdx.x;
  if (stage == RFS_AMAX) {
    const double m = rf_absmax_final(part, nslots, mred);
    if (t == 0) ds[RFD_AMAX] = m;
    return;
  }
  double s0, s1;
  rf_second_stage(stage != RFS_FINAL, part, RF_G, nslots, true, red, s0, s1);
  if (t >= RF_G || t >= nvec) return;
  const int q = t;
  const RfScalars v{ds + RFD_ALPHA + q, ds + RFD_BETA + q,  ds + RFD_RZ + q,          ds + RFD_BNORM + q,
                    ds + RFD_EBEST + q, ds + RFD_OUT + q,   ds + RFD_OUT + RF_G + q,  is + RFI_ST + q,
                    is + RFI_DECL + q,  is + RFI_RESTART + q, is + RFI_IMPROVE + q};
  rf_scalar_step(stage, s0, s1, tol, flag, ds[RFD_AMAX], v);
}

// ---------------------------------------------------------------------------------------------------
static inline int rf_rows_per_wg(int c) { return c == 0 ? 64 : (c == 1 ? 16 : 4); }

int spmv_slots(const RfOperator& op) {
  int s = 0;
  for (int c = 0; c < 3; ++c) s += (op.nrows[c] + rf_rows_per_wg(c) - 1) / rf_rows_per_wg(c);
  return s;
}

template <int LPR>
static void launch_spmv_class(hipStream_t st, const RfOperator& op, const int* rows, int nrows, int slot0,
                              const double* val, const double* x, int64_t ldx, const double* b, double* y, int64_t ldy,
                              int nvec, const int* sel, int want, double* part) {
  if (nrows <= 0) return;
  constexpr int RPB = 4 * (64 / LPR);
  dim3 g((unsigned)((nrows + RPB - 1) / RPB), (unsigned)((nvec + RF_NV - 1) / RF_NV));
  if (b)
    hipLaunchKernelGGL((k_spmv<LPR, true>), g, dim3(256), 0, st, rows, nrows, op.rowptr, op.col, op.src, val, x, ldx, b, y,
                       ldy, nvec, sel, want, part, slot0);
  else
    hipLaunchKernelGGL((k_spmv<LPR, false>), g, dim3(256), 0, st, rows, nrows, op.rowptr, op.col, op.src, val, x, ldx, b, y,
                       ldy, nvec, sel, want, part, slot0);
}

void launch_spmv(hipStream_t st, const RfOperator& op, const double* val, const double* x, int64_t ldx,
                 const double* b, double* y, int64_t ldy, int nvec, const int* sel, int want, double* part) {
  if (nvec <= 0) return;
  const int* rows = op.rows;
  int slot0 = 0;
  launch_spmv_class<4>(st, op, rows, op.nrows[0], slot0, val, x, ldx, b, y, ldy, nvec, sel, want, part);
  rows += op.nrows[0];
  slot0 += (op.nrows[0] + 63) / 64;
  launch_spmv_class<16>(st, op, rows, op.nrows[1], slot0, val, x, ldx, b, y, ldy, nvec, sel, want, part);
  rows += op.nrows[1];
  slot0 += (op.nrows[1] + 15) / 16;
  launch_spmv_class<64>(st, op, rows, op.nrows[2], slot0, val, x, ldx, b, y, ldy, nvec, sel, want, part);
}

int vec_slots(int n) { return (n + RF_VROWS - 1) / RF_VROWS; }

static inline dim3 rf_vgrid(int n, int nvec) { return dim3((unsigned)vec_slots(n), (unsigned)nvec); }

void launch_rf_axpy(hipStream_t st, int n, int nvec, const double* alpha, double* x, const double* p, double* r,
                    const double* q, const int* sel, int want, double* part) {
  if (n <= 0 || nvec <= 0) return;
  hipLaunchKernelGGL(k_rf_axpy, rf_vgrid(n, nvec), dim3(256), 0, st, n, alpha, x, p, r, q, sel, want, part);
}

void launch_rf_pupdate(hipStream_t st, int n, int nvec, const double* beta, double* p, const double* z,
                       const int* sel, int want) {
  if (n <= 0 || nvec <= 0) return;
  hipLaunchKernelGGL(k_rf_pupdate, rf_vgrid(n, nvec), dim3(256), 0, st, n, beta, p, z, sel, want);
}

void launch_rf_dot(hipStream_t st, int n, int nvec, const double* a, const double* b, const int* sel, int want,
                   double* part) {
  if (n <= 0 || nvec <= 0) return;
  hipLaunchKernelGGL(k_rf_dot, rf_vgrid(n, nvec), dim3(256), 0, st, n, a, b, sel, want, part);
}

void launch_rf_copy(hipStream_t st, int n, int nvec, double* dst, const double* src, const int* sel, int want,
                    bool zero_others) {
  if (n <= 0 || nvec <= 0) return;
  hipLaunchKernelGGL(k_rf_copy, rf_vgrid(n, nvec), dim3(256), 0, st, n, dst, src, sel, want, zero_others ? 1 : 0);
}

void launch_rf_absmax(hipStream_t st, const double* val, int64_t nnz, double* part) {
  hipLaunchKernelGGL(k_rf_absmax, dim3(RF_AMAX_WG), dim3(256), 0, st, val, nnz, part);
}

void launch_rf_finalize(hipStream_t st, int stage, const double* part, int nslots, int nvec, double tol, int flag,
                        double* ds, int* is) {
  hipLaunchKernelGGL(k_rf_finalize, dim3(1), dim3(256), 0, st, stage, part, nslots, nvec, tol, flag, ds, is);
}

}  // namespace spx
