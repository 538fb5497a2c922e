// The bodies of the step kernels of the selected inversion (selinv.hip: one arena; batch_selinv.hip: the arena
// of member b of a batch), as functions of (tile or unit, the tables, L, dinv, Z, scratch, the LDS arrays).  One
// set of bodies: the batch kernels compute, per member, exactly what the single-handle kernels compute, every
// sum in the same order.  A step of the SelinvProgram (schedule.hpp) is [SYMM] [SCALE] DIAG:
//
//   si_symm_body   Y = Z_RR L_RJ for one 64-row tile of R and one K slice, fp64 MFMA
//                  (v_mfma_f64_16x16x4_f64): Z_RR gathered through the row descriptors (its lower
//                  half directly, its upper half transposed from the same storage), L_RJ dense,
//                  both staged through LDS; the partial goes to the scratch (no atomics)
//   si_scale_body  the K slices summed in order, Z_RJ = -Y inv(L_JJ) stored into the Z arena,
//                  and the tile's  L_RJ^T Z_RJ  into the scratch
//   si_diag_body   Z_JJ = inv(L_JJ)^T (inv(L_JJ) - sum over the tiles, in order)
//   si_small_gather_body   product 1 of the fused whole-step kernels (a unit with nR <= 64 and one K slice):
//                  all of Z_RR and L_RJ into LDS at once
// Every sum runs in a fixed order: two runs on the same L give a bit-identical Z.
//
// MFMA lane map: lane l supplies A[l&15][l>>4] and B[l>>4][l&15] and receives C[(l>>4) + 4 r][l&15] in
// register r.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.hpp"

namespace spx {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int SI_KC = 32;           // K rows per LDS stage of si_symm_body
constexpr int SI_T = kSelinvTile;   // 64

// ---------------------------------------------------------------------------
// Y(i, j) = sum_k Z(r_i, r_k) L(r_k, j) over the unit's K slice; 4 wavefronts, wavefront w owns
// rows 16 w .. 16 w + 15 of the tile and all (<= 64) columns.
// ---------------------------------------------------------------------------
// kDoubleDiag: the gathered block is S = tril(G_RR) + tril(G_RR)^T of the factor adjoint (factor_adjoint.hip,
// batch_adjoint.hip: Z is then the adjoint arena), whose diagonal counts twice; a diagonal entry occurs in the
// generic branch only (r_i == r_k), the two dense-path branches hold chunks strictly above or below the tile.
// Selected inversion instantiates false.
template <bool kDoubleDiag>
__device__ __forceinline__ void si_symm_body(const UpdTile t, const SelinvUnit u, const SelinvRow* __restrict__ rows,
                                             const int* __restrict__ relpos, const double* __restrict__ L,
                                             const double* __restrict__ Z, double* __restrict__ scratch,
                                             double (*As)[SI_KC + 1], double (*Bs)[SI_T + 1], SelinvRow* Ri) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int nR = u.nR, pn = u.pn;
  const int i0 = t.ti * SI_T;
  const int k0 = t.tj * u.kslice;
  const int k1 = min(nR, k0 + u.kslice);
  const SelinvRow* nrows = rows + u.row_off;
  if (tid < SI_T && i0 + tid < nR) Ri[tid] = nrows[u.rbase + i0 + tid];
  __syncthreads();
  // A elements of this thread: (i = ai0 + 8 q, k = ak); B elements: (k = bk0 + 4 q, j = bj)
  const int ak = tid % SI_KC, ai0 = tid / SI_KC;
  const int bj = tid & 63, bk0 = tid >> 6;
  const double* Lrj = L + u.off + (int64_t)(u.c0 + pn) * u.ld + u.c0;
  double ra[8], rb[8];
  // a chunk wholly in the upper half of Z_RR (every tile row above every K row) is read transposed
  // through the tile rows' descriptors with the tile row fastest across the threads (coalesced);
  // otherwise the K row is fastest (coalesced for the lower half).
  // Dense path: where the rows that hold the entries -- the K rows for a lower chunk, the tile rows
  // for an upper one -- are the node's own columns inside ONE block column, Z_RR is a dense block of
  // that block column: one descriptor for the whole chunk, no per-element table loads or selects.
  auto upper = [&](int kb) { return i0 + SI_T <= kb; };
  auto lower = [&](int kb) { return kb + SI_KC <= i0; };
  auto own_block = [&](int first, int last) {   // R-local rows [first, last]
    const int a = u.rbase + first, b = u.rbase + last;
    return b < u.ncol && a / u.nb == b / u.nb;
  };
  const bool tile_dense = own_block(i0, min(nR, i0 + SI_T) - 1);
  const SelinvRow dI0 = Ri[0];
  auto load = [&](int kb) {
    const int klast = min(k1, kb + SI_KC) - 1;
    if (upper(kb) && tile_dense) {
      const int il = tid & 63;
      const bool iin = i0 + il < nR;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int kk = kb + (tid >> 6) + 4 * q;
        ra[q] = (iin && kk < k1) ? Z[dI0.cbase + il + (int64_t)(u.rbase + kk) * dI0.ld] : 0.0;
      }
    } else if (lower(kb) && own_block(kb, klast)) {
      const SelinvRow dK0 = nrows[u.rbase + kb];
      const bool kin = kb + ak < k1;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int ii = i0 + ai0 + 8 * q;
        ra[q] = (kin && ii < nR) ? Z[dK0.cbase + ak + (int64_t)(u.rbase + ii) * dK0.ld] : 0.0;
      }
    } else if (upper(kb)) {
      const int il = tid & 63, ii = i0 + il;
      const bool iin = ii < nR;
      const SelinvRow d = iin ? Ri[il] : SelinvRow{0, 0, -1};
      const int ri = u.rbase + ii;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int kk = kb + (tid >> 6) + 4 * q;
        double v = 0.0;
        if (iin && kk < k1) {
          const int rk = u.rbase + kk;
          const int64_t qpos = d.map < 0 ? (int64_t)rk : (int64_t)relpos[(int64_t)d.map + rk - ri];
          v = Z[d.cbase + qpos * d.ld];
        }
        ra[q] = v;
      }
    } else {
      const int kk = kb + ak;
      const bool kin = kk < k1;
      const int rk = u.rbase + kk;
      SelinvRow dk{0, 0, -1};
      if (kin) dk = nrows[rk];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int ii = i0 + ai0 + 8 * q;
        double v = 0.0;
        if (kin && ii < nR) {
          const int ri = u.rbase + ii;
          // lower half (r_i >= r_k) through row k's descriptor, upper half transposed through row i's
          const SelinvRow d = ri >= rk ? dk : Ri[ai0 + 8 * q];
          const int a = ri >= rk ? ri : rk, b = ri >= rk ? rk : ri;
          const int64_t qpos = d.map < 0 ? (int64_t)a : (int64_t)relpos[(int64_t)d.map + a - b];
          v = Z[d.cbase + qpos * d.ld];
          if (kDoubleDiag && ri == rk) v += v;
        }
        ra[q] = v;
      }
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int kr = kb + bk0 + 4 * q;
      rb[q] = (kr < k1 && bj < pn) ? Lrj[(int64_t)kr * u.ld + bj] : 0.0;
    }
  };
  d4 acc[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) acc[c] = d4{0.0, 0.0, 0.0, 0.0};
  const int ncb = (pn + 15) >> 4;
  load(k0);
  for (int kb = k0; kb < k1; kb += SI_KC) {
    __syncthreads();
    if (upper(kb)) {
#pragma unroll
      for (int q = 0; q < 8; ++q) As[tid & 63][(tid >> 6) + 4 * q] = ra[q];
    } else {
#pragma unroll
      for (int q = 0; q < 8; ++q) As[ai0 + 8 * q][ak] = ra[q];
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) Bs[bk0 + 4 * q][bj] = rb[q];
    __syncthreads();
    if (kb + SI_KC < k1) load(kb + SI_KC);   // in flight during the products
#pragma unroll
    for (int s = 0; s < SI_KC / 4; ++s) {
      const double a = As[16 * wv + (lane & 15)][4 * s + (lane >> 4)];
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (c < ncb) acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Bs[4 * s + (lane >> 4)][16 * c + (lane & 15)], acc[c], 0, 0, 0);
    }
  }
  double* Y = scratch + u.y_off + (int64_t)t.tj * nR * pn;
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = i0 + 16 * wv + (lane >> 4) + 4 * r, col = 16 * c + (lane & 15);
      if (row < nR && col < pn) Y[(int64_t)row * pn + col] = acc[c][r];
    }
}

// ---------------------------------------------------------------------------
// one 64-row tile of R: Y = sum of the K slices (in order), Z_RJ = -Y inv(L_JJ) into the Z arena,
// P = L_RJ^T Z_RJ over the tile's rows into the scratch (p_off + ti pn pn).
// Ms: inv(L_JJ), then the tile's rows of L_RJ
// ---------------------------------------------------------------------------
__device__ __forceinline__ void si_scale_body(const UpdTile t, const SelinvUnit u, const double* __restrict__ L,
                                              const double* __restrict__ dinv, double* __restrict__ Z,
                                              double* __restrict__ scratch, double (*Ys)[SI_T + 1],
                                              double (*Ms)[SI_T + 1]) {
  const int tid = threadIdx.x, j = tid & 63, i0w = tid >> 6;
  const int nR = u.nR, pn = u.pn;
  const int i0 = t.ti * SI_T;
  const int nr = min(SI_T, nR - i0);
  for (int q = 0; q < 16; ++q) {
    const int i = i0w + 4 * q;
    double y = 0.0, d = 0.0;
    if (j < pn) {
      if (i < nr)
        for (int s = 0; s < u.nsplit; ++s) y += scratch[u.y_off + ((int64_t)s * nR + i0 + i) * pn + j];
      if (i < pn && j <= i) d = dinv[u.dinv_off + (int64_t)i * u.dinv_ld + j];
    }
    Ys[i][j] = y;
    Ms[i][j] = d;
  }
  __syncthreads();
  double z[16];
  for (int q = 0; q < 16; ++q) {
    const int i = i0w + 4 * q;
    double s = 0.0;
    for (int c = j; c < pn; ++c) s += Ys[i][c] * Ms[c][j];
    z[q] = -s;
  }
  __syncthreads();
  double* Zrj = Z + u.off + (int64_t)(u.c0 + pn + i0) * u.ld + u.c0;
  const double* Lrj = L + u.off + (int64_t)(u.c0 + pn + i0) * u.ld + u.c0;
  for (int q = 0; q < 16; ++q) {
    const int i = i0w + 4 * q;
    const bool in = i < nr && j < pn;
    if (in) Zrj[(int64_t)i * u.ld + j] = z[q];
    Ys[i][j] = in ? z[q] : 0.0;
    Ms[i][j] = in ? Lrj[(int64_t)i * u.ld + j] : 0.0;
  }
  __syncthreads();
  double* P = scratch + u.p_off + (int64_t)t.ti * pn * pn;
  for (int q = 0; q < 16; ++q) {
    const int a = i0w + 4 * q;
    if (a >= pn || j >= pn) continue;
    double s = 0.0;
    for (int i = 0; i < nr; ++i) s += Ms[i][a] * Ys[i][j];
    P[a * pn + j] = s;
  }
}

// ---------------------------------------------------------------------------
// one panel: T = inv(L_JJ) - sum_t P_t (tiles in order), Z_JJ = inv(L_JJ)^T T, lower triangle stored
// ---------------------------------------------------------------------------
__device__ __forceinline__ void si_diag_body(const SelinvUnit u, const double* __restrict__ dinv, double* __restrict__ Z,
                                             const double* __restrict__ scratch, double (*Ds)[SI_T + 1],
                                             double (*Ts)[SI_T + 1]) {
  const int tid = threadIdx.x, b = tid & 63, a0 = tid >> 6;   // (1024 threads: 16 row groups)
  const int pn = u.pn;
  for (int q = 0; q < 4; ++q) {
    const int a = a0 + 16 * q;
    double d = 0.0, tt = 0.0;
    if (a < pn && b < pn) {
      if (b <= a) d = dinv[u.dinv_off + (int64_t)a * u.dinv_ld + b];
      tt = d;
      const double* p = scratch + u.p_off + (int64_t)a * pn + b;
#pragma unroll 8
      for (int ti = 0; ti < u.ntile; ++ti) tt -= p[(int64_t)ti * pn * pn];
    }
    Ds[a][b] = d;
    Ts[a][b] = tt;
  }
  __syncthreads();
  double* Zjj = Z + u.off + (int64_t)u.c0 * u.ld + u.c0;
  for (int q = 0; q < 4; ++q) {
    const int a = a0 + 16 * q;
    if (a >= pn || b > a) continue;
    double s = 0.0;
    for (int c = a; c < pn; ++c) s += Ds[c][a] * Ts[c][b];
    Zjj[(int64_t)a * u.ld + b] = s;
  }
}

// ---------------------------------------------------------------------------
// Product 1 of a fused whole-step kernel (nR <= 64, one K slice; 256 threads, thread t holds element
// ((t >> 6) + 4 q, t & 63) of a tile): Ri filled with the unit's row descriptors; the lower half of Z_RR read
// through the descriptor of the column's row (the K row fastest across the threads: coalesced) and mirrored into
// the upper half of A, the diagonal doubled under kDoubleDiag; L_RJ into lreg and into B.  A and B are written in
// full (zero outside the unit's rows and columns).  The caller puts a barrier in front of the product.
// ---------------------------------------------------------------------------
template <bool kDoubleDiag, int kLdA, int kLdB>
__device__ __forceinline__ void si_small_gather_body(const SelinvUnit u, const SelinvRow* __restrict__ rows,
                                                     const int* __restrict__ relpos, const double* __restrict__ L,
                                                     const double* __restrict__ Z, double (*A)[kLdA], double (*B)[kLdB],
                                                     SelinvRow* Ri, double (&lreg)[16]) {
  const int tid = threadIdx.x, tj = tid & 63, ti0 = tid >> 6;
  const int nR = u.nR, pn = u.pn;
  const SelinvRow* nrows = rows + u.row_off + u.rbase;
  if (tid < nR) Ri[tid] = nrows[tid];
  __syncthreads();
  const double* Lrj = L + u.off + (int64_t)(u.c0 + pn) * u.ld + u.c0;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int i = ti0 + 4 * q, k = tj;
    double v = 0.0;
    if (i < nR && k <= i) {
      const SelinvRow d = Ri[k];
      const int64_t qpos = d.map < 0 ? (int64_t)(u.rbase + i) : (int64_t)relpos[(int64_t)d.map + i - k];
      v = Z[d.cbase + qpos * d.ld];
      if (kDoubleDiag && k == i) v += v;
    }
    if (k <= i || i >= nR || k >= nR) A[i][k] = v;
    if (k < i && i < nR) A[k][i] = v;
    lreg[q] = (i < nR && tj < pn) ? Lrj[(int64_t)i * u.ld + tj] : 0.0;
    B[i][tj] = lreg[q];
  }
}

}  // namespace spx
