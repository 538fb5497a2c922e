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

namespace spx {

__device__ __forceinline__ bool rf_selected(const int* sel, int want, int q) { return !sel || sel[q] == want; }

// sum over the wavefront (butterfly: every lane ends with the same bits)
__device__ __forceinline__ double rf_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// the workgroup's sums of a and b to part[(slot * 2 + 0 / 1) * G + q]; every thread of the 256 calls it
__device__ __forceinline__ void rf_block_sum2(double a, double b, double* part, int slot, int q) {
  __shared__ double red[2][4];
  a = rf_wave_sum(a);
  b = rf_wave_sum(b);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { red[0][wave] = a; red[1][wave] = b; }
  __syncthreads();
  if (threadIdx.x < 2) {
    const int w = threadIdx.x;
    part[((int64_t)slot * 2 + w) * RF_G + q] = ((red[w][0] + red[w][1]) + red[w][2]) + red[w][3];
  }
}

// ---------------------------------------------------------------------------------------------------
// rows[first .. first + nrows) of one length class; workgroup = 4 wavefronts x (64 / LPR) rows, grid.y =
// chunk of RF_NV vectors.  Lane `sub` of a row's LPR lanes takes entries sub, sub + LPR, ... in order, the
// LPR sums meet in a butterfly.
// ---------------------------------------------------------------------------------------------------
template <int LPR, bool RES>
__global__ __launch_bounds__(256) void k_spmv(const int* __restrict__ rows, int nrows, const int64_t* __restrict__ rowptr,
                                              const int* __restrict__ col, const int* __restrict__ src,
                                              const double* __restrict__ val, const double* __restrict__ x, int64_t ldx,
                                              const double* __restrict__ b, double* __restrict__ y, int64_t ldy, int nvec,
                                              const int* __restrict__ sel, int want, double* __restrict__ part,
                                              int slot0) {
  constexpr int RPW = 64 / LPR, RPB = 4 * RPW;
  __shared__ double red[4][2 * RF_NV];
  const int q0 = blockIdx.y * RF_NV;
  const int nq = min(RF_NV, nvec - q0);
  unsigned act = 0;
  for (int j = 0; j < nq; ++j)
    if (rf_selected(sel, want, q0 + j)) act |= 1u << j;
  if (!act) return;   // (the same for every thread of the workgroup)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sub = lane % LPR;
  const int ri = blockIdx.x * RPB + wave * RPW + lane / LPR;
  const bool has = ri < nrows;
  const int row = has ? rows[ri] : 0;
  const int64_t k0 = has ? rowptr[row] : 0, k1 = has ? rowptr[row + 1] : 0;
  double acc[RF_NV];
#pragma unroll
  for (int j = 0; j < RF_NV; ++j) acc[j] = 0.0;
  for (int64_t k = k0 + sub; k < k1; k += LPR) {
    const int c = col[k];
    const double a = val[src[k]];
#pragma unroll
    for (int j = 0; j < RF_NV; ++j)
      if (j < nq) acc[j] = fma(a, x[(int64_t)(q0 + j) * ldx + c], acc[j]);
  }
#pragma unroll
  for (int j = 0; j < RF_NV; ++j)
#pragma unroll
    for (int off = LPR / 2; off >= 1; off >>= 1) acc[j] += __shfl_xor(acc[j], off, 64);
  const bool lead = has && sub == 0;
  double p0[RF_NV], p1[RF_NV];
#pragma unroll
  for (int j = 0; j < RF_NV; ++j) {
    p0[j] = 0.0;
    p1[j] = 0.0;
    if (lead && ((act >> j) & 1u)) {
      const double xr = x[(int64_t)(q0 + j) * ldx + row];
      const double out = RES ? b[(int64_t)(q0 + j) * ldy + row] - acc[j] : acc[j];
      y[(int64_t)(q0 + j) * ldy + row] = out;
      p0[j] = RES ? out * out : xr * out;
      p1[j] = RES ? xr * xr : 0.0;
    }
  }
  if (!part) return;
#pragma unroll
  for (int j = 0; j < RF_NV; ++j) {
    p0[j] = rf_wave_sum(p0[j]);
    p1[j] = rf_wave_sum(p1[j]);
    if (lane == 0) { red[wave][2 * j] = p0[j]; red[wave][2 * j + 1] = p1[j]; }
  }
  __syncthreads();
  if (threadIdx.x < 2 * RF_NV) {
    const int j = threadIdx.x >> 1, w = threadIdx.x & 1;
    if (j < nq)
      part[((int64_t)(slot0 + blockIdx.x) * 2 + w) * RF_G + q0 + j] =
          ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
  }
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
  double rr = 0.0, xx = 0.0;
#pragma unroll
  for (int k = 0; k < RF_VROWS / 256; ++k) {
    const int i = blockIdx.x * RF_VROWS + k * 256 + threadIdx.x;
    if (i < n) {
      const double xv = fma(a, p[base + i], x[base + i]);
      x[base + i] = xv;
      xx = fma(xv, xv, xx);
      if (qv) {
        const double rv = fma(-a, qv[base + i], r[base + i]);
        r[base + i] = rv;
        rr = fma(rv, rv, rr);
      }
    }
  }
  if (part) rf_block_sum2(rr, xx, part, blockIdx.x, q);
}

__global__ __launch_bounds__(256) void k_rf_pupdate(int n, const double* __restrict__ beta, double* __restrict__ p,
                                                    const double* __restrict__ z, const int* __restrict__ sel,
                                                    int want) {
  const int q = blockIdx.y;
  if (!rf_selected(sel, want, q)) return;
  const double bt = beta[q];
  const int64_t base = (int64_t)q * n;
#pragma unroll
  for (int k = 0; k < RF_VROWS / 256; ++k) {
    const int i = blockIdx.x * RF_VROWS + k * 256 + threadIdx.x;
    if (i < n) p[base + i] = bt == 0.0 ? z[base + i] : fma(bt, p[base + i], z[base + i]);
  }
}

__global__ __launch_bounds__(256) void k_rf_dot(int n, const double* __restrict__ a, const double* __restrict__ b,
                                                const int* __restrict__ sel, int want, double* __restrict__ part) {
  const int q = blockIdx.y;
  if (!rf_selected(sel, want, q)) return;
  const int64_t base = (int64_t)q * n;
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < RF_VROWS / 256; ++k) {
    const int i = blockIdx.x * RF_VROWS + k * 256 + threadIdx.x;
    if (i < n) s = fma(a[base + i], b[base + i], s);
  }
  rf_block_sum2(s, 0.0, part, blockIdx.x, q);
}

__global__ __launch_bounds__(256) void k_rf_copy(int n, double* __restrict__ dst, const double* __restrict__ src,
                                                 const int* __restrict__ sel, int want, int zero_others) {
  const int q = blockIdx.y;
  const bool mine = rf_selected(sel, want, q);
  if (!mine && !zero_others) return;
  const int64_t base = (int64_t)q * n;
#pragma unroll
  for (int k = 0; k < RF_VROWS / 256; ++k) {
    const int i = blockIdx.x * RF_VROWS + k * 256 + threadIdx.x;
    if (i < n) dst[base + i] = mine ? src[base + i] : 0.0;
  }
}

// max that a NaN wins: once m is a NaN no comparison replaces it
__device__ __forceinline__ double rf_nanmax(double m, double a) { return (a > m || a != a) ? a : m; }

__global__ __launch_bounds__(256) void k_rf_absmax(const double* __restrict__ val, int64_t nnz, double* __restrict__ part) {
  __shared__ double red[4];
  double m = 0.0;
  for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < nnz; k += (int64_t)gridDim.x * 256)
    m = rf_nanmax(m, fabs(val[k]));
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) m = rf_nanmax(m, __shfl_xor(m, off, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = rf_nanmax(rf_nanmax(rf_nanmax(red[0], red[1]), red[2]), red[3]);
}

// ---------------------------------------------------------------------------------------------------
// One workgroup of 256: thread t adds the partials of vector t & 31 in slots (t >> 5), (t >> 5) + 8, ... ;
// the eight slices of a vector are then added in order by thread q, which also does the scalar step.
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool rf_finite(double v) { return v == v && fabs(v) <= 1.79769313486231570e308; }

__global__ __launch_bounds__(256) void k_rf_finalize(int stage, const double* __restrict__ part, int nslots, int nvec,
                                                     double tol, int flag, double* __restrict__ ds, int* __restrict__ is) {
  __shared__ double red[2][8][RF_G];
  __shared__ double mred[256];
  const int t = threadIdx.x;
  if (stage == RFS_AMAX) {
    double m = 0.0;
    for (int s = t; s < nslots; s += 256) m = rf_nanmax(m, part[s]);
    mred[t] = m;
    __syncthreads();
    if (t == 0) {
      for (int s = 1; s < 256; ++s) m = rf_nanmax(m, mred[s]);
      ds[RFD_AMAX] = m;
    }
    return;
  }
  const int q = t & (RF_G - 1), sl = t >> 5;
  double s0 = 0.0, s1 = 0.0;
  if (stage != RFS_FINAL)
    for (int s = sl; s < nslots; s += 8) {
      s0 += part[((int64_t)s * 2) * RF_G + q];
      s1 += part[((int64_t)s * 2 + 1) * RF_G + q];
    }
  red[0][sl][q] = s0;
  red[1][sl][q] = s1;
  __syncthreads();
  if (t >= RF_G || t >= nvec) return;
  s0 = red[0][0][q];
  s1 = red[1][0][q];
  for (int s = 1; s < 8; ++s) { s0 += red[0][s][q]; s1 += red[1][s][q]; }
  int st = is[RFI_ST + q];
  switch (stage) {
    case RFS_BNORM:   // s0 = |b|^2: the start of a group
      ds[RFD_BNORM + q] = sqrt(s0);
      ds[RFD_EBEST + q] = -1.0;
      ds[RFD_RZ + q] = 0.0;
      ds[RFD_ALPHA + q] = 0.0;
      ds[RFD_BETA + q] = 0.0;
      st = 0;
      is[RFI_DECL + q] = 0;
      is[RFI_RESTART + q] = 1;
      is[RFI_IMPROVE + q] = 0;
      break;
    case RFS_TRUE: {  // s0 = |b - A x|^2, s1 = |x|^2 of the vectors with st == 0 (flag = 0) / decl == 1 (flag = 1)
      const bool mine = flag ? is[RFI_DECL + q] == 1 : st == 0;
      int improve = 0;
      if (mine) {
        const double e = s0 == 0.0 ? 0.0 : sqrt(s0) / (ds[RFD_BNORM + q] + ds[RFD_AMAX] * sqrt(s1));
        const double eb = ds[RFD_EBEST + q];
        if (eb < 0.0 || e < eb) { improve = 1; ds[RFD_EBEST + q] = e; }
        if (!rf_finite(e)) st = 2;
        else if (e <= tol) st = 1;
        else is[RFI_RESTART + q] = 1;   // (PCG: go on from the true residual with a fresh direction)
        is[RFI_DECL + q] = 0;
      }
      is[RFI_IMPROVE + q] = improve;
      break;
    }
    case RFS_ALPHA:   // s0 = p.q
      if (st == 0) {
        const double a = ds[RFD_RZ + q] / s0;
        if (!rf_finite(a)) st = 2;
        ds[RFD_ALPHA + q] = rf_finite(a) ? a : 0.0;
      }
      break;
    case RFS_REC:     // s0 = |r|^2 of the recurrence, s1 = |x|^2
      if (st == 0) {
        const double e = s0 == 0.0 ? 0.0 : sqrt(s0) / (ds[RFD_BNORM + q] + ds[RFD_AMAX] * sqrt(s1));
        if (!rf_finite(e)) st = 2;
        else if (e <= tol) is[RFI_DECL + q] = 1;
      }
      break;
    case RFS_BETA:    // s0 = r.z
      if (st == 0) {
        const double bt = is[RFI_RESTART + q] ? 0.0 : s0 / ds[RFD_RZ + q];
        if (!rf_finite(bt) || !rf_finite(s0)) st = 2;
        ds[RFD_BETA + q] = rf_finite(bt) ? bt : 0.0;
        ds[RFD_RZ + q] = s0;
        is[RFI_RESTART + q] = 0;
      }
      break;
    case RFS_FINAL:   // what still iterates gets one true residual before the call returns
      is[RFI_DECL + q] = st == 0 ? 1 : 0;
      break;
    default: break;
  }
  is[RFI_ST + q] = st;
  ds[RFD_OUT + q] = ds[RFD_EBEST + q];
  ds[RFD_OUT + RF_G + q] = (double)st;
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
