// The device bodies of the REPRODUCIBLE blocked substitution (batch_repro.hip: one arena per member of a batch):
// the launches of a SolveProgram on a block of RB = 16 or 32 right-hand sides, every product on
// v_mfma_f64_16x16x4_f64 through sm_mm (sm_mm.hpp), with no atomic add.  A strip STORES its products into a
// scratch; the diagonal launch that owns a row subtracts the stored products in the order of the RsolveTables
// (schedule.hpp) before it runs the unchanged arithmetic of sm_diag_body (sm_body.hpp).  A body is a function of
// (unit or tile, L, dinv, W, scratch, tables) alone.
//
// Workspace W[p * RB + q] as in sm_body.hpp; scratch[s * RB + q]: slot s of the tables, right-hand side q.
// Column q of an MFMA result depends on column q of B alone and its sum runs over k in an order that depends on K
// only; the gathers are one thread per (row, q) walking its list in table order.  So the bits of a vector depend
// neither on RB, nor on its place in the block, nor on the other vectors.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.hpp"
#include "sm_mm.hpp"

namespace spx {

// forward strip ti of block column u (id bcol): scratch[(fslot[bcol] + r - w) * RB + q] = L[r, :] x_J, rows
// r = w + 64 ti ..; wavefront v owns rows 16 v .. 16 v + 15, K = w  (no barrier)
template <int RB>
__device__ __forceinline__ void rsm_strip_fwd_body(int ti, const SolveUnit u, int64_t fslot, const double* __restrict__ L,
                                                   const double* W, double* __restrict__ scratch) {
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
  double* out = scratch + (fslot + (r0 - w)) * RB;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = 16 * wv + g + 4 * r;
    if (row < nr) {
#pragma unroll
      for (int c = 0; c < NC; ++c) out[(int64_t)row * RB + 16 * c + col] = acc[c][r];
    }
  }
}

// backward strip ti of block column u, tile `bslot` of the program: scratch[(bslot + k) * RB + q] =
// sum_r L[r][k] x[idx[r]] over the strip's rows; X: the strip's rows of x gathered into LDS
template <int RB>
__device__ __forceinline__ void rsm_strip_bwd_body(int ti, const SolveUnit u, int64_t bslot, const double* __restrict__ L,
                                                   const int* __restrict__ rlist, const double* W,
                                                   double* __restrict__ scratch, double (*X)[RB + SM_PAD]) {
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
  double* out = scratch + bslot * RB;
  for (int kt = wv; 16 * kt < w; kt += 4) {
    d4 acc[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = d4{0.0, 0.0, 0.0, 0.0};
    sm_mm<RB>(A + min(16 * kt + col, w - 1), w, nr, &X[0][0], RB + SM_PAD, lane, acc);
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

// what a diagonal launch does before the arithmetic of sm_diag_body: the rows of block column u (id bcol) of W
// minus the stored products, one after the other in table order -- one thread per (row, q).  Ends with a barrier.
//   forward : row p = gcol0 + j minus scratch[gsrc[k]], k = gptr[p] .. gptr[p + 1])
//   backward: row j minus the partials of the strips t = 0, 1, .. at scratch[bfirst[bcol] + t w + j]
template <bool BWD, int RB>
__device__ __forceinline__ void rsm_gather_body(const SolveUnit u, int bcol, const RsmTables& tb, double* W,
                                                const double* __restrict__ scratch) {
  const int w = u.w;
  double* Wb = W + (int64_t)u.gcol0 * RB;
  if (!BWD) {
    for (int e = threadIdx.x; e < w * RB; e += 256) {
      const int j = e / RB, q = e % RB;
      const int64_t k0 = tb.gptr[u.gcol0 + j], k1 = tb.gptr[u.gcol0 + j + 1];
      if (k0 == k1) continue;
      double v = Wb[e];
      // (eight slots requested at a time, subtracted one after the other: the order is the table's)
      int64_t k = k0;
      for (; k + 8 <= k1; k += 8) {
        double a[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) a[i] = scratch[tb.gsrc[k + i] * RB + q];
#pragma unroll
        for (int i = 0; i < 8; ++i) v -= a[i];
      }
      for (; k < k1; ++k) v -= scratch[tb.gsrc[k] * RB + q];
      Wb[e] = v;
    }
  } else {
    const int64_t first = tb.bfirst[bcol];
    const int ns = first < 0 ? 0 : (u.nrow - w + kSolveStripRows - 1) / kSolveStripRows;
    if (ns > 0) {
      for (int e = threadIdx.x; e < w * RB; e += 256) {
        double v = Wb[e];
        const double* part = scratch + first * RB + e;   // (slot first + t w + j, vector q: + (j RB + q) = e)
        const int64_t step = (int64_t)w * RB;
        int t = 0;
        for (; t + 8 <= ns; t += 8) {   // (eight partials requested at a time, subtracted in ascending strip index)
          double a[8];
#pragma unroll
          for (int i = 0; i < 8; ++i) a[i] = part[(t + i) * step];
#pragma unroll
          for (int i = 0; i < 8; ++i) v -= a[i];
        }
        for (; t < ns; ++t) v -= part[t * step];
        Wb[e] = v;
      }
    }
  }
  __syncthreads();
}

}  // namespace spx
