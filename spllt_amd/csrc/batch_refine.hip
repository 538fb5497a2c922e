// Refined solves for the members of a batch on gfx950: the operator A_b on the analysed pattern for every
// member and the vector kernels around the batch's substitution programs (refine.hpp has the layouts).  The
// device bodies are those of refine.hip (rf_body.hpp): a member's sums have the order of the single handle.
//
//   k_bspmv<LPR, RES>   Y_b = A_b X_b or Y_b = B_b - A_b X_b: k_spmv for (member, row block, chunk of RF_NV vectors)
//   k_brf_axpy / k_brf_pupdate / k_brf_dot / k_brf_copy     the vector kernels for (member, vector, slot)
//   k_brf_permute       caller's vectors <-> work vectors
//   k_brf_absmax        partial max |val_b|
//   k_brf_finalize      one workgroup per member: second stage of every reduction, the scalar step of its vectors
//
// Grids are linear, the member folded in.  The product puts the members of one (row block, chunk) next to each
// other: they read the same col / src / rowptr entries, so those streams stay in the caches while the members'
// values and vectors stream through; no index is shared through LDS (a workgroup serves one member, as in
// refine.hip, which keeps the lane order of a row).  The vector kernels keep a member's workgroups together.
// A member whose flag is set is skipped by every kernel, before any barrier.  No atomics, no inline assembly.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>

#include "batch_split.hpp"
#include "kernels.hpp"
#include "refine.hpp"
#include "rf_body.hpp"

namespace spx {

__device__ __forceinline__ bool brf_skipped(const int* flag, int b) { return flag && flag[b] != INT_MAX; }

// workgroup -> (member b, row block, chunk): wg = (chunk * nrb + rblock) * nb + (b - b0)
template <int LPR, bool RES>
__global__ __launch_bounds__(256) void k_bspmv(const int* __restrict__ rows, int nrows, const int64_t* __restrict__ rowptr,
                                               const int* __restrict__ col, const int* __restrict__ src,
                                               const double* __restrict__ val, int64_t ldval,
                                               const double* __restrict__ x, int64_t xstride, int64_t ldx,
                                               const double* __restrict__ bv, double* __restrict__ y, int64_t ystride,
                                               int64_t ldy, int nvec, const int* __restrict__ sel, int want,
                                               double* __restrict__ part, int slot0, int64_t np,
                                               const int* __restrict__ flag, const double* __restrict__ sigma, int b0,
                                               int nb, int nrb) {
  __shared__ double red[4][2 * RF_NV];
  const unsigned wg = blockIdx.x;
  const int b = b0 + (int)(wg % (unsigned)nb);
  if (brf_skipped(flag, b)) return;
  const unsigned item = wg / (unsigned)nb;
  const int rblock = (int)(item % (unsigned)nrb), q0 = (int)(item / (unsigned)nrb) * RF_NV;
  const int nq = min(RF_NV, nvec - q0);
  const int64_t g0 = (int64_t)b * nvec;
  unsigned act = 0;
  for (int j = 0; j < nq; ++j)
    if (rf_selected(sel ? sel + g0 : nullptr, want, q0 + j)) act |= 1u << j;
  if (!act) return;   // (the same for every thread of the workgroup)
  rf_spmv_body<LPR, RES>(rblock, q0, nq, act, rows, nrows, rowptr, col, src, val + (int64_t)b * ldval,
                         x + (int64_t)b * xstride, ldx, bv ? bv + (int64_t)b * ystride : nullptr,
                         y + (int64_t)b * ystride, ldy, part ? part + ((int64_t)(slot0 + rblock) * 2) * np + g0 : nullptr,
                         np, sigma ? sigma[b] : 1.0, red);
}

// workgroup -> (member, vector, slot) of the vector kernels: wg = ((b - b0) * nv + q) * vslots + slot
struct BrfItem { int b, q, slot; int64_t g; };
__device__ __forceinline__ BrfItem brf_item(int b0, int nv, int vslots) {
  const unsigned wg = blockIdx.x;
  BrfItem it;
  it.slot = (int)(wg % (unsigned)vslots);
  const unsigned pr = wg / (unsigned)vslots;
  it.q = (int)(pr % (unsigned)nv);
  it.b = b0 + (int)(pr / (unsigned)nv);
  it.g = (int64_t)it.b * nv + it.q;
  return it;
}

__global__ __launch_bounds__(256) void k_brf_axpy(int n, int nv, int vslots, int b0, const int* __restrict__ flag,
                                                  const double* __restrict__ alpha, double* __restrict__ x,
                                                  const double* __restrict__ p, double* __restrict__ r,
                                                  const double* __restrict__ qv, const int* __restrict__ sel, int want,
                                                  double* __restrict__ part, int64_t np,
                                                  const double* __restrict__ sigma) {
  const BrfItem it = brf_item(b0, nv, vslots);
  if (brf_skipped(flag, it.b) || (sel && sel[it.g] != want)) return;
  const double a = alpha ? alpha[it.g] : 1.0;
  const int64_t base = it.g * n;
  double rr, xx;
  rf_axpy_body(n, it.slot, a, x + base, p + base, r ? r + base : nullptr, qv ? qv + base : nullptr, sigma[it.b], rr, xx);
  if (part) rf_block_sum2(rr, xx, part + ((int64_t)it.slot * 2) * np + it.g, np);
}

__global__ __launch_bounds__(256) void k_brf_pupdate(int n, int nv, int vslots, int b0, const int* __restrict__ flag,
                                                     const double* __restrict__ beta, double* __restrict__ p,
                                                     const double* __restrict__ z, const int* __restrict__ sel, int want) {
  const BrfItem it = brf_item(b0, nv, vslots);
  if (brf_skipped(flag, it.b) || (sel && sel[it.g] != want)) return;
  const int64_t base = it.g * n;
  rf_pupdate_body(n, it.slot, beta[it.g], p + base, z + base);
}

__global__ __launch_bounds__(256) void k_brf_dot(int n, int nv, int vslots, int b0, const int* __restrict__ flag,
                                                 const double* __restrict__ a, const double* __restrict__ b,
                                                 const int* __restrict__ sel, int want, double* __restrict__ part,
                                                 int64_t np, const double* __restrict__ sigma) {
  const BrfItem it = brf_item(b0, nv, vslots);
  if (brf_skipped(flag, it.b) || (sel && sel[it.g] != want)) return;
  const int64_t base = it.g * n;
  const double s = rf_dot_body(n, it.slot, a + base, b + base, sigma ? sigma[it.b] : 1.0);
  rf_block_sum2(s, 0.0, part + ((int64_t)it.slot * 2) * np + it.g, np);
}

__global__ __launch_bounds__(256) void k_brf_copy(int n, int nv, int vslots, int b0, const int* __restrict__ flag,
                                                  double* __restrict__ dst, const double* __restrict__ src,
                                                  const int* __restrict__ sel, int want, int zero_others) {
  const BrfItem it = brf_item(b0, nv, vslots);
  if (brf_skipped(flag, it.b)) return;
  const bool mine = !sel || sel[it.g] == want;
  if (!mine && !zero_others) return;
  const int64_t base = it.g * n;
  rf_copy_body(n, it.slot, mine, dst + base, src + base);
}

__global__ __launch_bounds__(256) void k_brf_permute(int unpack, int n, int nv, int vslots, int b0,
                                                     const int* __restrict__ flag, unsigned long long* __restrict__ x,
                                                     int64_t xstride, int64_t ldx, const int* __restrict__ order,
                                                     unsigned long long* __restrict__ W) {
  const BrfItem it = brf_item(b0, nv, vslots);
  if (brf_skipped(flag, it.b)) return;
  unsigned long long* xv = x + (int64_t)it.b * xstride + (int64_t)it.q * ldx;
  unsigned long long* wv = W + it.g * n;
#pragma unroll
  for (int k = 0; k < RF_VROWS / 256; ++k) {
    const int i = it.slot * RF_VROWS + k * 256 + (int)threadIdx.x;
    if (i < n) {
      const int p = order ? order[i] : i;
      if (unpack) xv[i] = wv[p];
      else wv[p] = xv[i];
    }
  }
}

// workgroup -> (member, share): wg = (b - b0) * RF_AMAX_WG + share
__global__ __launch_bounds__(256) void k_brf_absmax(const double* __restrict__ val, int64_t ldval, int64_t nnz, int b0,
                                                    const int* __restrict__ flag, double* __restrict__ part) {
  __shared__ double red[4];
  const int b = b0 + (int)(blockIdx.x / RF_AMAX_WG), share = (int)(blockIdx.x % RF_AMAX_WG);
  if (brf_skipped(flag, b)) return;
  rf_absmax_body(val + (int64_t)b * ldval, nnz, share, RF_AMAX_WG, part + (int64_t)b * RF_AMAX_WG + share, red);
}

// one workgroup of 256 per member
__global__ __launch_bounds__(256) void k_brf_finalize(int stage, const BrfView v, int b0, int nslots, double tol,
                                                      int flagarg) {
  __shared__ double red[2][8][RF_G];
  __shared__ double mred[256];
  const int t = threadIdx.x, b = b0 + (int)blockIdx.x, nv = v.nv;
  const int64_t np = (int64_t)v.nbatch * nv, g = (int64_t)b * nv + (t & (RF_G - 1));
  const bool live = (t & (RF_G - 1)) < nv;
  if (brf_skipped(v.flag, b)) {
    // a member without a factor: its pairs never iterate, nothing else of it is touched
    if (stage == RFS_BNORM && t < nv) {
      v.is[g] = 2;
      v.is[np + g] = 0;
      v.is[2 * np + g] = 0;
      v.is[3 * np + g] = 0;
      v.ds[5 * np + g] = -1.0;
      v.ds[6 * np + g] = 2.0;
    }
    return;
  }
  if (stage == RFS_AMAX) {
    const double m = rf_absmax_final(v.part + (int64_t)b * RF_AMAX_WG, RF_AMAX_WG, mred);
    if (t == 0) {
      // sigma_b = 2^-exponent(max |a_ij|): what scales a residual of member b to the size of its solution
      v.amax[b] = m;
      // (the exponent clamped to the normal range: a subnormal max |a_ij| must not make sigma infinite)
      v.sigma[b] = (rf_finite(m) && m > 0.0) ? scalbn(1.0, -min(max(ilogb(m), -1022), 1022)) : 1.0;
    }
    return;
  }
  double s0, s1;
  rf_second_stage(stage != RFS_FINAL, v.part + (int64_t)b * nv, np, nslots, live, red, s0, s1);
  if (t >= RF_G || t >= nv) return;
  const RfScalars sc{v.ds + g,          v.ds + np + g,     v.ds + 2 * np + g, v.ds + 3 * np + g,
                     v.ds + 4 * np + g, v.ds + 5 * np + g, v.ds + 6 * np + g, v.is + g,
                     v.is + np + g,     v.is + 2 * np + g, v.is + 3 * np + g};
  rf_scalar_step(stage, s0, s1, tol, flagarg, v.amax[b] * v.sigma[b], sc);
}

// ---------------------------------------------------------------------------------------------------
namespace {
template <int LPR>
int launch_bspmv_class(hipStream_t st, const RfOperator& op, const int* rows, int nrows, int slot0, const BrfView& v,
                       const double* val, int64_t ldval, const double* x, int64_t xstride, int64_t ldx, const double* b,
                       double* y, int64_t ystride, int64_t ldy, const int* sel, int want, double* part) {
  if (nrows <= 0) return 0;
  constexpr int RPB = 4 * (64 / LPR);
  const int nrb = (nrows + RPB - 1) / RPB, nchunk = (v.nv + RF_NV - 1) / RF_NV;
  const int64_t np = v.np();
  return batch_member_ranges(v.nbatch, (int64_t)nrb * nchunk, [&](int b0, int nb) {
    const dim3 g((unsigned)((int64_t)nrb * nchunk * nb));
    if (b)
      hipLaunchKernelGGL((k_bspmv<LPR, true>), g, dim3(256), 0, st, rows, nrows, op.rowptr, op.col, op.src, val, ldval, x,
                         xstride, ldx, b, y, ystride, ldy, v.nv, sel, want, part, slot0, np, v.flag, v.sigma, b0, nb, nrb);
    else
      hipLaunchKernelGGL((k_bspmv<LPR, false>), g, dim3(256), 0, st, rows, nrows, op.rowptr, op.col, op.src, val, ldval, x,
                         xstride, ldx, b, y, ystride, ldy, v.nv, sel, want, part, slot0, np, v.flag, v.sigma, b0, nb, nrb);
  });
}

}  // namespace

int launch_bspmv(hipStream_t st, const RfOperator& op, const BrfView& v, const double* val, int64_t ldval,
                 const double* x, int64_t xstride, int64_t ldx, const double* b, double* y, int64_t ystride, int64_t ldy,
                 const int* sel, int want, bool partials) {
  if (v.nv <= 0 || v.nbatch <= 0) return 0;
  // (nothing is launched unless every class fits: the widest grid is that of the first populated class or another)
  for (int c = 0; c < 3; ++c) {
    const int rpb = c == 0 ? 64 : (c == 1 ? 16 : 4);
    if ((int64_t)((op.nrows[c] + rpb - 1) / rpb) * ((v.nv + RF_NV - 1) / RF_NV) > batch_grid_limit_max()) return -1;
  }
  double* part = partials ? v.part : nullptr;
  const int* rows = op.rows;
  int slot0 = 0;
  BrfTally c;
  c.add(launch_bspmv_class<4>(st, op, rows, op.nrows[0], slot0, v, val, ldval, x, xstride, ldx, b, y, ystride, ldy, sel, want, part));
  rows += op.nrows[0];
  slot0 += (op.nrows[0] + 63) / 64;
  c.add(launch_bspmv_class<16>(st, op, rows, op.nrows[1], slot0, v, val, ldval, x, xstride, ldx, b, y, ystride, ldy, sel, want, part));
  rows += op.nrows[1];
  slot0 += (op.nrows[1] + 15) / 16;
  c.add(launch_bspmv_class<64>(st, op, rows, op.nrows[2], slot0, v, val, ldval, x, xstride, ldx, b, y, ystride, ldy, sel, want, part));
  return c.count();
}

namespace {
// the grid of a vector kernel: (members of the range) x nv x vslots workgroups
template <class Fn>
int brf_vector_launch(const BrfView& v, int n, Fn&& fn) {
  if (n <= 0 || v.nv <= 0) return 0;
  const int vslots = vec_slots(n);
  return batch_member_ranges(v.nbatch, (int64_t)vslots * v.nv,
                    [&](int b0, int nb) { fn(dim3((unsigned)((int64_t)vslots * v.nv * nb)), vslots, b0); });
}
}  // namespace

int launch_brf_axpy(hipStream_t st, const BrfView& v, int n, const double* alpha, double* x, const double* p, double* r,
                    const double* q, const int* sel, int want, bool partials) {
  return brf_vector_launch(v, n, [&](dim3 g, int vslots, int b0) {
    hipLaunchKernelGGL(k_brf_axpy, g, dim3(256), 0, st, n, v.nv, vslots, b0, v.flag, alpha, x, p, r, q, sel, want,
                       partials ? v.part : nullptr, (int64_t)v.np(), v.sigma);
  });
}

int launch_brf_pupdate(hipStream_t st, const BrfView& v, int n, const double* beta, double* p, const double* z,
                       const int* sel, int want) {
  return brf_vector_launch(v, n, [&](dim3 g, int vslots, int b0) {
    hipLaunchKernelGGL(k_brf_pupdate, g, dim3(256), 0, st, n, v.nv, vslots, b0, v.flag, beta, p, z, sel, want);
  });
}

int launch_brf_dot(hipStream_t st, const BrfView& v, int n, const double* a, const double* b, const int* sel, int want,
                   bool residual_like) {
  return brf_vector_launch(v, n, [&](dim3 g, int vslots, int b0) {
    hipLaunchKernelGGL(k_brf_dot, g, dim3(256), 0, st, n, v.nv, vslots, b0, v.flag, a, b, sel, want, v.part, (int64_t)v.np(),
                       residual_like ? v.sigma : nullptr);
  });
}

int launch_brf_copy(hipStream_t st, const BrfView& v, int n, double* dst, const double* src, const int* sel, int want,
                    bool zero_others) {
  return brf_vector_launch(v, n, [&](dim3 g, int vslots, int b0) {
    hipLaunchKernelGGL(k_brf_copy, g, dim3(256), 0, st, n, v.nv, vslots, b0, v.flag, dst, src, sel, want, zero_others ? 1 : 0);
  });
}

int launch_brf_permute(hipStream_t st, const BrfView& v, bool unpack, double* x, int64_t xstride, int64_t ldx,
                       const int* order, int n, double* W) {
  return brf_vector_launch(v, n, [&](dim3 g, int vslots, int b0) {
    hipLaunchKernelGGL(k_brf_permute, g, dim3(256), 0, st, unpack ? 1 : 0, n, v.nv, vslots, b0, v.flag,
                       reinterpret_cast<unsigned long long*>(x), xstride, ldx, order, reinterpret_cast<unsigned long long*>(W));
  });
}

int launch_brf_absmax(hipStream_t st, const BrfView& v, const double* val, int64_t ldval, int64_t nnz) {
  BrfTally c;
  c.add(batch_member_ranges(v.nbatch, RF_AMAX_WG, [&](int b0, int nb) {
    hipLaunchKernelGGL(k_brf_absmax, dim3((unsigned)(RF_AMAX_WG * nb)), dim3(256), 0, st, val, ldval, nnz, b0, v.flag, v.part);
  }));
  c.add(launch_brf_finalize(st, v, RFS_AMAX, RF_AMAX_WG, 0.0, 0));
  return c.count();
}

int launch_brf_finalize(hipStream_t st, const BrfView& v, int stage, int nslots, double tol, int flag) {
  return batch_member_ranges(v.nbatch, 1, [&](int b0, int nb) {
    hipLaunchKernelGGL(k_brf_finalize, dim3((unsigned)nb), dim3(256), 0, st, stage, v, b0, nslots, tol, flag);
  });
}

}  // namespace spx
