// The device bodies of the factor products (factor_mult.hip: one arena; batch_mult.hip: one arena per member of
// a batch).  A body is a function of (tile or chunk, L, X, Y, tables, scratch) alone: the kernels around it
// only say which arena, which workspaces and which scratch.  Every sum runs in an order fixed by the tables
// and by K, never by RB, by the vector's place in the block or by the member: the same arena bits and
// vector bits give the same result bits through either wrapper.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.hpp"
#include "sm_mm.hpp"

namespace spx {

// ---------------------------------------------------------------------------
// strips.  L X: wavefront v owns rows 16 v .. 16 v + 15 of the strip, K = w (k_sm_strip_fwd with a store).
// L^T X: the strip's rows of X gathered into LDS, wavefront v owns the 16-column tiles v, v + 4, ... of the
// block column, K = the strip's rows (k_sm_strip_bwd with a store).
// Xs: LDS, kSolveStripRows rows (T) or unused (!T).  tile: the index of tl in the tile list.
// ---------------------------------------------------------------------------
template <bool T, int RB>
__device__ __forceinline__ void fm_strip_body(const UpdTile tl, int64_t tile, const SolveUnit u,
                                              const double* __restrict__ L, const int* __restrict__ rlist,
                                              const double* __restrict__ X, const FmultView& fv,
                                              double (*Xs)[RB + SM_PAD]) {
  constexpr int NC = RB / 16;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int g = lane >> 4, col = lane & 15;
  const int w = u.w;
  const int r0 = w + tl.ti * kSolveStripRows;
  const int nr = min(kSolveStripRows, u.nrow - r0);
  const double* A = L + u.off + (int64_t)r0 * w;
  if (!T) {
    if (16 * wv >= nr) return;   // (no barrier in this instance)
    d4 acc[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = d4{0.0, 0.0, 0.0, 0.0};
    sm_mm<RB>(A + (int64_t)min(16 * wv + col, nr - 1) * w, 1, w, X + (int64_t)u.gcol0 * RB, RB, lane, acc);
    double* out = fv.scratch + (fv.fslot[tl.unit] + (r0 - w)) * RB;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * wv + g + 4 * r;
      if (row < nr) {
#pragma unroll
        for (int c = 0; c < NC; ++c) out[(int64_t)row * RB + 16 * c + col] = acc[c][r];
      }
    }
  } else {
    const int* idx = rlist + u.idx_off + r0;
    for (int e = tid; e < kSolveStripRows * RB; e += 256) {
      const int r = e / RB, q = e % RB;
      Xs[r][q] = r < nr ? X[(int64_t)idx[r] * RB + q] : 0.0;
    }
    __syncthreads();
    double* out = fv.scratch + fv.bslot[tile] * RB;
    for (int kt = wv; 16 * kt < w; kt += 4) {
      d4 acc[NC];
#pragma unroll
      for (int c = 0; c < NC; ++c) acc[c] = d4{0.0, 0.0, 0.0, 0.0};
      sm_mm<RB>(A + min(16 * kt + col, w - 1), w, nr, &Xs[0][0], RB + SM_PAD, lane, acc);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int k = 16 * kt + g + 4 * r;
        if (k < w) {
#pragma unroll
          for (int c = 0; c < NC; ++c) out[(int64_t)k * RB + 16 * c + col] = acc[c][r];
        }
      }
    }
  }
}

// the 16 x 16 block of the diagonal tile at (c0, c0), lower triangle only, times rows c0 .. c0 + 15 of X.
// !T: the lane's row m of L, k runs over its columns (k <= m);  T: the lane's column m, k over its rows (k >= m).
// mv: m is a row / column of the tile (< w).  What is masked is neither multiplied nor relied upon.
template <bool T, int RB>
__device__ __forceinline__ void fm_diag_block(const double* __restrict__ A, int w, int c0, int m, bool mv,
                                              const double* __restrict__ Xb, int g, int col, d4 (&acc)[RB / 16]) {
  constexpr int NC = RB / 16;
  double a[4], b[4][NC];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int k = c0 + 4 * e + g;
    const bool ok = mv && k < w && (T ? k >= m : k <= m);
    const int kc = min(k, w - 1);
    const double av = T ? A[(int64_t)kc * w + m] : A[(int64_t)m * w + kc];
    a[e] = ok ? av : 0.0;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const double bv = Xb[(int64_t)kc * RB + 16 * c + col];
      b[e][c] = k < w ? bv : 0.0;
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[e], b[e][c], acc[c], 0, 0, 0);
}

// ---------------------------------------------------------------------------
// One workgroup per (block column, chunk of 64 of its pivot positions); wavefront v owns positions 16 v ..
// 16 v + 15 of the chunk.
//   L X   : y_j = sum_{k <= j} L_jk x_k  (columns before the 16-block through sm_mm, then the masked block),
//           then y[p] += scratch[gsrc[k]] for k = gptr[p] .. gptr[p+1] - 1 in that order
//   L^T X : y_j = sum_{k >= j} L_kj x_k  (the masked block, then the rows behind it through sm_mm),
//           then y_j += the column sums of strip 0, 1, ... in that order
// Ts: LDS, 64 rows (!T) or unused (T).
// ---------------------------------------------------------------------------
template <bool T, int RB>
__device__ __forceinline__ void fm_diag_body(const UpdTile ch, const SolveUnit u, const double* __restrict__ L,
                                             const double* __restrict__ X, double* __restrict__ Y,
                                             const FmultView& fv, double (*Ts)[RB + SM_PAD]) {
  constexpr int NC = RB / 16;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int g = lane >> 4, col = lane & 15;
  const int w = u.w;
  const int j0 = ch.ti * 64;           // first position of the chunk inside the block column
  const int c0 = j0 + 16 * wv;         // ... and of the wavefront's 16
  const double* A = L + u.off;
  const double* Xb = X + (int64_t)u.gcol0 * RB;
  const bool active = c0 < w;
  const bool mv = c0 + col < w;
  const int m = min(c0 + col, w - 1);
  d4 acc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[c] = d4{0.0, 0.0, 0.0, 0.0};
  if (!T) {
    if (active) {
      if (c0 > 0) sm_mm<RB>(A + (int64_t)m * w, 1, c0, Xb, RB, lane, acc);
      fm_diag_block<false, RB>(A, w, c0, m, mv, Xb, g, col, acc);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < NC; ++c) Ts[16 * wv + g + 4 * r][16 * c + col] = acc[c][r];
    __syncthreads();
    // RB lanes per position: a row of the scratch is one contiguous read
    for (int e = tid; e < 64 * RB; e += 256) {
      const int row = e / RB, q = e % RB;
      if (j0 + row >= w) break;
      const int p = u.gcol0 + j0 + row;
      double v = Ts[row][q];
      const int64_t k1 = fv.gptr[p + 1];
      for (int64_t k = fv.gptr[p]; k < k1; k += 4) {
        double s[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) s[i] = fv.scratch[fv.gsrc[k + i < k1 ? k + i : k1 - 1] * RB + q];
#pragma unroll
        for (int i = 0; i < 4; ++i) v += k + i < k1 ? s[i] : 0.0;
      }
      Y[(int64_t)p * RB + q] = v;
    }
  } else {
    if (!active) return;   // (no barrier in this instance)
    fm_diag_block<true, RB>(A, w, c0, m, mv, Xb, g, col, acc);
    const int kb = c0 + 16;
    if (kb < w) sm_mm<RB>(A + (int64_t)kb * w + m, w, w - kb, Xb + (int64_t)kb * RB, RB, lane, acc);
    const int ns = (u.nrow - w + kSolveStripRows - 1) / kSolveStripRows;
    const int64_t bfirst = fv.bfirst[ch.unit];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int k = c0 + g + 4 * r;
      if (k < w) {
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          double v = acc[c][r];
          const double* part = fv.scratch + (bfirst + k) * RB + 16 * c + col;
          for (int t = 0; t < ns; ++t) v += part[(int64_t)t * w * RB];
          Y[(int64_t)(u.gcol0 + k) * RB + 16 * c + col] = v;
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// noise: Philox4x32-10, counter (pivot position, stream, sample lo, sample hi), key (seed lo, seed hi);
// Box-Muller on the two 53-bit uniforms of that one block, one value per block.  Stream 0 is the noise of the
// single-handle samplers; member b of a batch draws from stream stream0 + b * stream_step.
// ---------------------------------------------------------------------------
__device__ __forceinline__ double fm_normal(uint32_t p, uint32_t stream, uint64_t sample, uint64_t seed) {
  uint32_t c0 = p, c1 = stream, c2 = (uint32_t)sample, c3 = (uint32_t)(sample >> 32);
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0;
    c1 = l1;
    c2 = h0 ^ c3 ^ k1;
    c3 = l0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  // u1 in (0, 1] from words 0 (low) and 1 (high), u2 in [0, 1) from words 2 and 3: 53 bits each
  const uint64_t a = (((uint64_t)c1 << 32) | c0) >> 11, b = (((uint64_t)c3 << 32) | c2) >> 11;
  const double u1 = (double)(a + 1) * 0x1p-53, u2 = (double)b * 0x1p-53;
  return sqrt(-2.0 * log(u1)) * cos(6.283185307179586476925 * u2);
}

}  // namespace spx
