// The device bodies of the blocked substitution (solve_many.hip: one arena; batch_solve_many.hip: one arena per
// member of a batch).  A body is a function of (unit or tile, L, dinv, W, rlist, the LDS array) alone: the
// kernels around it only say which arena, which dinv scratch and which workspace.  Every sum runs in the order
// it has always had in k_sm_*: fixed by the tables and by K, never by the wrapper.  (The pack / unpack body, which
// the products use too, is in sm_mm.hpp.)
//
// Workspace layout: W[p * RB + q], pivot position p, right-hand side q < RB.  Lane l of a wavefront supplies
// A[l&15][l>>4] and B[l>>4][l&15] and receives C[(l>>4) + 4 r][l&15] in register r.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.hpp"
#include "sm_mm.hpp"

namespace spx {

// ---------------------------------------------------------------------------
// Diagonal tile of one block column per workgroup (4 wavefronts, wavefront v owns rows 16 v .. 16 v + 15
// of the current panel):
//   forward   x_p = inv(L_pp)   (y_p - L_p,<p x_<p)
//   backward  x_p = inv(L_pp)^T (y_p - L_>p,p^T x_>p)
// x lives in W (the block column's w x RB rows, L2-resident); only t = y_p - ... of the current panel
// goes through LDS (T).  The dinv layout (SolveUnit::pw / cb) as in k_solve_diag.
// ---------------------------------------------------------------------------
template <bool BWD, int RB>
__device__ __forceinline__ void sm_diag_body(const SolveUnit u, const double* __restrict__ L,
                                             const double* __restrict__ dinv, double* W, double (*T)[RB + SM_PAD]) {
  constexpr int NC = RB / 16;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int g = lane >> 4, col = lane & 15;
  const int w = u.w, pw = u.pw;
  const double* A = L + u.off;
  double* Wb = W + (int64_t)u.gcol0 * RB;   // (the block column's own columns are consecutive pivot positions)
  const int np = (w + pw - 1) / pw;
  for (int pp = 0; pp < np; ++pp) {
    const int p = BWD ? np - 1 - pp : pp;
    const int c0 = p * pw, pn = min(pw, w - c0);
    // inv(L_pp) inside the inverse of its chain block (schedule.hpp winv_offset / winv_ld)
    const int g0 = (c0 / u.cb) * u.cb, ldw = min(u.cb, w - g0);
    int64_t slot = u.dinv_off;
    for (int t = 0; t < g0; t += u.cb) {
      const int64_t cwt = min(u.cb, w - t);
      slot += cwt * cwt;
    }
    const double* D = dinv + slot + (int64_t)(c0 - g0) * ldw + (c0 - g0);
    const bool active = 16 * wv < pn;
    const int m = min(16 * wv + col, pn - 1);   // the lane's row of the panel as an A operand
    // what the step reads besides L_p,<p / L_>p,p and x: the panel's own rows of y and the lane's share of
    // inv(L_pp) (forward: row m, k <= m; backward: column m, k >= m; the other triangle of the slot is not
    // relied upon) -- requested before the product, so that they arrive during it
    double yv[4][NC], dv[16];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = min(16 * wv + g + 4 * r, pn - 1);
#pragma unroll
      for (int c = 0; c < NC; ++c) yv[r][c] = Wb[(int64_t)(c0 + row) * RB + 16 * c + col];
    }
    const int kbeg = BWD ? 16 * wv : 0, kend = BWD ? pn : min(pn, 16 * wv + 16);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int k = kbeg + 4 * e + g;
      const bool ok = BWD ? (k >= m && k < pn) : k <= m;
      const int kc = BWD ? min(max(k, m), pn - 1) : min(k, m);
      const double d = BWD ? D[(int64_t)kc * ldw + m] : D[(int64_t)m * ldw + kc];
      dv[e] = ok ? d : 0.0;
    }
    d4 acc[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = d4{0.0, 0.0, 0.0, 0.0};
    if (active) {
      if (!BWD) {
        if (c0 > 0) sm_mm<RB>(A + (int64_t)(c0 + m) * w, 1, c0, Wb, RB, lane, acc);
      } else {
        const int kb = c0 + pn;
        if (kb < w) sm_mm<RB>(A + (int64_t)kb * w + c0 + m, w, w - kb, Wb + (int64_t)kb * RB, RB, lane, acc);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * wv + g + 4 * r;
#pragma unroll
      for (int c = 0; c < NC; ++c)
        T[row][16 * c + col] = row < pn ? yv[r][c] - acc[c][r] : 0.0;
    }
    __syncthreads();
    if (active) {
      d4 x[NC];
#pragma unroll
      for (int c = 0; c < NC; ++c) x[c] = d4{0.0, 0.0, 0.0, 0.0};
      // forward: x_j = sum_{k <= j} Dinv[j][k] t_k;  backward: x_j = sum_{k >= j} Dinv[k][j] t_k
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int k0 = kbeg + 4 * e;
        if (k0 < kend) {
#pragma unroll
          for (int c = 0; c < NC; ++c)
            x[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(dv[e], T[k0 + g][16 * c + col], x[c], 0, 0, 0);
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * wv + g + 4 * r;
        if (row < pn) {
#pragma unroll
          for (int c = 0; c < NC; ++c) Wb[(int64_t)(c0 + row) * RB + 16 * c + col] = x[c][r];
        }
      }
    }
    __syncthreads();   // the panel's x is in W for every wavefront of the workgroup; T may change
  }
}

// ---------------------------------------------------------------------------
// Rows below the diagonal tile, strip ti of kSolveStripRows (64) rows of block column u per workgroup.
//   forward : W[idx[r]] -= L[r, :] x_J : wavefront v owns rows 16 v .. 16 v + 15, K = w  (no barrier)
// ---------------------------------------------------------------------------
template <int RB>
__device__ __forceinline__ void sm_strip_fwd_body(int ti, const SolveUnit u, const double* __restrict__ L,
                                                  const int* __restrict__ rlist, double* W) {
  constexpr int NC = RB / 16;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int g = lane >> 4, col = lane & 15;
  const int w = u.w;
  const int r0 = w + ti * kSolveStripRows;
  const int nr = min(kSolveStripRows, u.nrow - r0);
  if (16 * wv >= nr) return;
  const double* arow = L + u.off + (int64_t)(r0 + min(16 * wv + col, nr - 1)) * w;
  d4 acc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[c] = d4{0.0, 0.0, 0.0, 0.0};
  sm_mm<RB>(arow, 1, w, W + (int64_t)u.gcol0 * RB, RB, lane, acc);
  const int* idx = rlist + u.idx_off + r0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = 16 * wv + g + 4 * r;
    if (row < nr) {
      double* dst = W + (int64_t)idx[row] * RB + col;
#pragma unroll
      for (int c = 0; c < NC; ++c) unsafeAtomicAdd(dst + 16 * c, -acc[c][r]);
    }
  }
}

//   backward: W[gcol0 + k] -= sum_r L[r][k] x[idx[r]] : the strip's 64 rows of x gathered into LDS (X),
//   wavefront v owns the 16-column tiles v, v + 4, ... of the block column, K = the strip's rows
template <int RB>
__device__ __forceinline__ void sm_strip_bwd_body(int ti, const SolveUnit u, const double* __restrict__ L,
                                                  const int* __restrict__ rlist, double* W,
                                                  double (*X)[RB + SM_PAD]) {
  constexpr int NC = RB / 16;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int g = lane >> 4, col = lane & 15;
  const int w = u.w;
  const int r0 = w + ti * kSolveStripRows;
  const int nr = min(kSolveStripRows, u.nrow - r0);
  const double* A = L + u.off + (int64_t)r0 * w;
  const int* idx = rlist + u.idx_off + r0;
  for (int e = tid; e < kSolveStripRows * RB; e += 256) {
    const int r = e / RB, q = e % RB;
    X[r][q] = r < nr ? W[(int64_t)idx[r] * RB + q] : 0.0;
  }
  __syncthreads();
  double* Wb = W + (int64_t)u.gcol0 * RB;
  for (int kt = wv; 16 * kt < w; kt += 4) {
    d4 acc[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = d4{0.0, 0.0, 0.0, 0.0};
    sm_mm<RB>(A + min(16 * kt + col, w - 1), w, nr, &X[0][0], RB + SM_PAD, lane, acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int k = 16 * kt + g + 4 * r;
      if (k < w) {
        double* dst = Wb + (int64_t)k * RB + col;
#pragma unroll
        for (int c = 0; c < NC; ++c) unsafeAtomicAdd(dst + 16 * c, -acc[c][r]);
      }
    }
  }
}

}  // namespace spx
