// The bodies of the factor-adjoint kernels (factor_adjoint.hip: one arena; batch_adjoint.hip: the arena of
// member b of a batch), as functions of (tile or unit, L, dinv, G, scratch, the LDS arrays).  One set of
// bodies: the batch kernels compute, per member, exactly what the single-handle kernels compute, every sum
// in the same order.  The LDS strides and their bank argument: the header of factor_adjoint.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.hpp"
#include "si_body.hpp"   // d4; the SYMM step of the adjoint is si_symm_body<true>

namespace spx {

constexpr int FA_T = kSelinvTile;   // 64
constexpr int FA_LDA = 66;
constexpr int FA_LDB = 80;
constexpr int FA_NV = 32;           // vectors per pass of the seed

// ---------------------------------------------------------------------------
// One workgroup per (block column, 64-row strip).  Thread t: column (t & 63) of the current 64-column
// chunk, rows (t >> 6) + 4 k.  Per entry ONE chain acc = fma(a_q[r], b_q[c], acc) over q ascending, whatever
// nvec is (the passes of FA_NV vectors keep their accumulators), alpha applied once at the end: a vector's
// contribution does not depend on nvec or on its place among the others.  a_q[r] comes from LDS as a
// same-address read of the wavefront, b_q[c] sits in registers, the stores run along the arena's rows.
// The strict upper triangle of a diagonal tile is not written.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void fa_seed_body(const UpdTile tl, const FadjCol u, const int* __restrict__ rlist,
                                             const int* __restrict__ porder, double* __restrict__ G, int nvec,
                                             const double* __restrict__ a, const double* __restrict__ b, int64_t ld,
                                             double alpha, int accumulate, int a_pivot, int b_pivot,
                                             double (*As)[FA_T], int* Ra) {
  const int tid = threadIdx.x, cl = tid & 63, rg = tid >> 6;
  const int r0 = tl.ti * FA_T;
  const int nr = min(FA_T, u.nrow - r0);
  if (tid < FA_T) {
    const int p = rlist[u.idx_off + r0 + min(tid, nr - 1)];
    Ra[tid] = a_pivot ? p : porder[p];
  }
  for (int c0 = 0; c0 < u.w; c0 += FA_T) {
    const int col = c0 + cl;
    const bool cin = col < u.w;
    const int pc = u.gcol0 + min(col, u.w - 1);
    const int jb = b_pivot ? pc : porder[pc];
    double acc[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) acc[k] = 0.0;
    for (int q0 = 0; q0 < nvec; q0 += FA_NV) {
      const int nq = min(FA_NV, nvec - q0);
      __syncthreads();   // (Ra written; the last pass read)
      for (int e = tid; e < FA_NV * FA_T; e += 256) {
        const int q = e >> 6, r = e & 63;
        As[q][r] = (q < nq && r < nr) ? a[(int64_t)(q0 + q) * ld + Ra[r]] : 0.0;
      }
      double bq[FA_NV];
#pragma unroll
      for (int q = 0; q < FA_NV; ++q) bq[q] = q < nq ? b[(int64_t)(q0 + q) * ld + jb] : 0.0;
      __syncthreads();
#pragma unroll
      for (int q = 0; q < FA_NV; ++q) {
        if (q < nq) {
#pragma unroll
          for (int k = 0; k < 16; ++k) acc[k] = fma(As[q][rg + 4 * k], bq[q], acc[k]);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int r = r0 + rg + 4 * k;   // row of the block column: r < w is pivot gcol0 + r
      if (rg + 4 * k < nr && cin && (r >= u.w || r >= col)) {
        double* g = G + u.off + (int64_t)r * u.w + col;
        const double v = alpha * acc[k];
        *g = accumulate ? *g + v : v;
      }
    }
  }
}

// acc[c] += A B for the wavefront's 16 rows arow .. arow + 15 and the column blocks c < ncb; K = 4 ks
__device__ __forceinline__ void fadj_mm4(const double (*At)[FA_LDA], int arow, const double (*Bt)[FA_LDB], int ks,
                                         int ncb, int lane, d4 (&acc)[4]) {
  const int g = lane >> 4, col = lane & 15;
  for (int s = 0; s < ks; ++s) {
    const double av = At[arow + col][4 * s + g];
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < ncb) acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, Bt[4 * s + g][16 * c + col], acc[c], 0, 0, 0);
  }
}

// the wavefront's 16 x 16 block (bi, bj) of At Bt, K = 4 ks
__device__ __forceinline__ d4 fadj_mm1(const double (*At)[FA_LDA], const double (*Bt)[FA_LDB], int bi, int bj, int ks,
                                       int lane) {
  const int g = lane >> 4, col = lane & 15;
  d4 acc = d4{0.0, 0.0, 0.0, 0.0};
  for (int s = 0; s < ks; ++s)
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(At[16 * bi + col][4 * s + g], Bt[4 * s + g][16 * bj + col], acc, 0, 0, 0);
  return acc;
}

// ---------------------------------------------------------------------------
// SCALE: one 64-row tile of R, 4 wavefronts; wavefront w owns rows 16 w .. 16 w + 15 of each product.
// At: T, then W^T.  Bt: inv(L_JJ), then the tile's rows of L_RJ.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void fa_scale_body(const UpdTile t, const SelinvUnit u, const double* __restrict__ L,
                                              const double* __restrict__ dinv, double* __restrict__ G,
                                              double* __restrict__ scratch, double (*At)[FA_LDA], double (*Bt)[FA_LDB]) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int j = lane, g = lane >> 4, col = lane & 15;
  const int nR = u.nR, pn = u.pn;
  const int i0 = t.ti * FA_T;
  const int nr = min(FA_T, nR - i0);
  double* Grj = G + u.off + (int64_t)(u.c0 + pn + i0) * u.ld + u.c0;
  const double* Lrj = L + u.off + (int64_t)(u.c0 + pn + i0) * u.ld + u.c0;
  for (int q = 0; q < 16; ++q) {
    const int i = wv + 4 * q;
    double tv = 0.0, dv = 0.0;
    if (j < pn) {
      if (i < nr) {
        double y = 0.0;
        for (int s = 0; s < u.nsplit; ++s) y += scratch[u.y_off + ((int64_t)s * nR + i0 + i) * pn + j];
        tv = Grj[(int64_t)i * u.ld + j] - y;
      }
      if (i < pn && j <= i) dv = dinv[u.dinv_off + (int64_t)i * u.dinv_ld + j];
    }
    At[i][j] = tv;
    Bt[i][j] = dv;
  }
  __syncthreads();
  const int ncb = (pn + 15) >> 4;
  d4 acc[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) acc[c] = d4{0.0, 0.0, 0.0, 0.0};
  fadj_mm4(At, 16 * wv, Bt, (pn + 3) >> 2, ncb, lane, acc);   // W = T inv(L_JJ)
  __syncthreads();
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = 16 * wv + g + 4 * r, jj = 16 * c + col;
      const double w = acc[c][r];   // (0 outside nr x pn: T and inv(L_JJ) are zero there)
      if (i < nr && jj < pn) Grj[(int64_t)i * u.ld + jj] = w;
      At[jj][i] = w;
    }
  for (int q = 0; q < 16; ++q) {
    const int i = wv + 4 * q;
    Bt[i][j] = (i < nr && j < pn) ? Lrj[(int64_t)i * u.ld + j] : 0.0;
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < 4; ++c) acc[c] = d4{0.0, 0.0, 0.0, 0.0};
  fadj_mm4(At, 16 * wv, Bt, (nr + 3) >> 2, ncb, lane, acc);    // Q = W^T L_RJ over the tile's rows
  double* Q = scratch + u.p_off + (int64_t)t.ti * pn * pn;
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int a = 16 * wv + g + 4 * r, bb = 16 * c + col;
      if (a < pn && bb < pn) Q[a * pn + bb] = acc[c][r];
    }
}

// ---------------------------------------------------------------------------
// DIAG: one panel, 16 wavefronts: wavefront w owns the 16 x 16 block (w >> 2, w & 3) of each of the three
// products.  L_JJ and G_JJ are masked to their lower triangles (the upper halves of the arenas are
// unspecified), the dinv slot as well; rows and columns past pn are zero in every operand.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void fa_diag_body(const SelinvUnit u, const double* __restrict__ L,
                                             const double* __restrict__ dinv, double* __restrict__ G,
                                             const double* __restrict__ scratch, double (*At)[FA_LDA],
                                             double (*Bt)[FA_LDB]) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int b = lane, g = lane >> 4, col = lane & 15;
  const int bi = wv >> 2, bj = wv & 3;
  const int pn = u.pn, ks = (pn + 3) >> 2;
  const double* Ljj = L + u.off + (int64_t)u.c0 * u.ld + u.c0;
  double* Gjj = G + u.off + (int64_t)u.c0 * u.ld + u.c0;
  double d[4];
  for (int q = 0; q < 4; ++q) {
    const int a = wv + 16 * q;
    double lv = 0.0, mv = 0.0;
    d[q] = 0.0;
    if (a < pn && b <= a) {
      lv = Ljj[(int64_t)a * u.ld + b];
      d[q] = dinv[u.dinv_off + (int64_t)a * u.dinv_ld + b];
      const double* p = scratch + u.p_off + (int64_t)a * pn + b;
      double s = 0.0;
#pragma unroll 8
      for (int ti = 0; ti < u.ntile; ++ti) s += p[(int64_t)ti * pn * pn];
      mv = Gjj[(int64_t)a * u.ld + b] - s;
    }
    At[b][a] = lv;   // L_JJ^T
    Bt[a][b] = mv;   // M
  }
  __syncthreads();
  d4 x = fadj_mm1(At, Bt, bi, bj, ks, lane);   // L_JJ^T M
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = 16 * bi + g + 4 * r, cc = 16 * bj + col;
    if (row >= cc) {   // sym(tril(.)): Phi + Phi^T
      At[row][cc] = x[r];
      At[cc][row] = x[r];
    }
  }
  for (int q = 0; q < 4; ++q) Bt[wv + 16 * q][b] = d[q];
  __syncthreads();
  x = fadj_mm1(At, Bt, bi, bj, ks, lane);      // (P + P^T) inv(L_JJ)
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) Bt[16 * bi + g + 4 * r][16 * bj + col] = x[r];
  for (int q = 0; q < 4; ++q) At[b][wv + 16 * q] = d[q];   // inv(L_JJ)^T
  __syncthreads();
  x = fadj_mm1(At, Bt, bi, bj, ks, lane);      // N
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = 16 * bi + g + 4 * r, cc = 16 * bj + col;
    if (row < pn && cc <= row) Gjj[(int64_t)row * u.ld + cc] = row == cc ? 0.5 * x[r] : x[r];
  }
}

}  // namespace spx
