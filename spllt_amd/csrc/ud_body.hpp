// The device bodies of the low-rank update / downdate, shared by updown.hip (one factor) and batch_updown.hip
// (the members of a batch): both translation units run the same arithmetic in the same order.
//
//   ud_rotate_chunk    a tile of rows through LDS, a row per thread, rotated by a chunk of columns
//   ud_walk_triangle   the column walk of one panel's triangle in LDS: the coefficients, the rotated triangle
//   ud_panel_inverse   inv of the new triangle, four lanes per column
//   ud_strip_loop      the rows of the diagonal square below a panel, in strips of kUpdownRows
//   ud_gen_block       a whole diagonal square (one workgroup): the four above per panel
//   ud_apply_block     one strip of kUpdownRows rows below the square (one workgroup)
//
// Per column j and vector q (in this order, q fastest):
//   d = L_jj, r = sqrt(d d + sign w_j w_j), c = r / d, t = w_j / d, L_jj = r
//   rows i > j:  L_ij = (L_ij + sign t w_i) / c,  w_i = c w_i - t L_ij
// w_j = 0 gives c = 1, t = 0: the identity, bit for bit.  No atomics; a row belongs to one thread.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.hpp"

namespace spx {

constexpr int kUdKK = kUpdownVec;
constexpr int kUdTileLd = kUpdownChunk + 1;        // doubles: lanes of a half wavefront on distinct banks
constexpr int kUdTriLd = kPanelMax + 1;
constexpr int kUdCoef = 3;                         // c, t, 1 / c
// LDS of a generate workgroup (doubles): the panel's triangle, later the row tile; the inverse; the panel's coefficients
constexpr int kUdGenBufA =
    kUpdownRows * kUdTileLd > kPanelMax * kUdTriLd ? kUpdownRows * kUdTileLd : kPanelMax * kUdTriLd;
constexpr int kUdGenBufX = kPanelMax * kUdTriLd;
constexpr int kUdGenCoef = kPanelMax * kUdKK * kUdCoef;
constexpr size_t kUdGenLds = sizeof(double) * (size_t)(kUdGenBufA + kUdGenBufX + kUdGenCoef);
// LDS of an apply workgroup (doubles): the row tile, the chunk's coefficients
constexpr int kUdApplyTile = kUpdownRows * kUdTileLd;
constexpr int kUdApplyCoef = kUpdownChunk * kUdKK * kUdCoef;

// Rows [row0, row0 + nr) of the block column A (row width ld), columns [c0, c0 + cn), nr <= kUpdownRows, cn <=
// kUpdownChunk: into the LDS tile with coalesced loads (16 bytes per lane where the rows are 16-byte aligned),
// thread i rotates row i with the chunk's coefficients coef[(j * KK + q) * 3 ..] (LDS) and its wi[], and back.
// Every thread of the workgroup calls it; it ends with a barrier (tile and coef may be rewritten after it).
template <int NV>
__device__ __forceinline__ void ud_rotate_chunk(double* __restrict__ A, int ld, int row0, int nr, int c0, int cn,
                                                const double* coef, double (&wi)[NV], double* tile, double sgn) {
  constexpr int KK = kUdKK, kTileLd = kUdTileLd, kCoef = kUdCoef;
  const int tid = threadIdx.x;
  double* base = A + (int64_t)row0 * ld + c0;
  const bool vec = ((ld | cn) & 1) == 0 && (reinterpret_cast<uintptr_t>(base) & 15) == 0;
  if (vec) {
    const int h = cn >> 1;
    for (int e = tid; e < nr * h; e += kUpdownRows) {
      const int r = e / h, c = (e - r * h) * 2;
      const double2 v = *reinterpret_cast<const double2*>(base + (int64_t)r * ld + c);
      tile[r * kTileLd + c] = v.x;
      tile[r * kTileLd + c + 1] = v.y;
    }
  } else {
    for (int e = tid; e < nr * cn; e += kUpdownRows) {
      const int r = e / cn, c = e - r * cn;
      tile[r * kTileLd + c] = base[(int64_t)r * ld + c];
    }
  }
  __syncthreads();
  if (tid < nr) {
    double* t = tile + tid * kTileLd;
    for (int j = 0; j < cn; ++j) {
      double l = t[j];
      const double* cf = coef + j * KK * kCoef;
#pragma unroll
      for (int q = 0; q < NV; ++q) {
        const double c = cf[q * kCoef], tt = cf[q * kCoef + 1], ic = cf[q * kCoef + 2];
        l = (l + sgn * tt * wi[q]) * ic;
        wi[q] = c * wi[q] - tt * l;
      }
      t[j] = l;
    }
  }
  __syncthreads();
  if (vec) {
    const int h = cn >> 1;
    for (int e = tid; e < nr * h; e += kUpdownRows) {
      const int r = e / h, c = (e - r * h) * 2;
      double2 v;
      v.x = tile[r * kTileLd + c];
      v.y = tile[r * kTileLd + c + 1];
      *reinterpret_cast<double2*>(base + (int64_t)r * ld + c) = v;
    }
  } else {
    for (int e = tid; e < nr * cn; e += kUpdownRows) {
      const int r = e / cn, c = e - r * cn;
      base[(int64_t)r * ld + c] = tile[r * kTileLd + c];
    }
  }
  __syncthreads();
}

// The column walk of one panel's triangle T (LDS, pn x pn, row stride kUdTriLd) by the threads of its rows: thread
// j makes the coefficients of column j for all vectors -- they depend on L_jj and on its own w_j only -- the
// threads below apply them.  wi[]: thread tid's entries of the work array (tid < pn).  p0: the pivot position of
// the panel's column 0.  A downdate that meets d d - w_j w_j <= 0 records the pivot position + 1 in *flag (the
// smallest one: the workgroups of a sweep that share a flag word run one after the other) and goes on with r = d.
// Ends without a barrier behind the last column.
template <int NV>
__device__ __forceinline__ void ud_walk_triangle(double* T, double* coef, int pn, int p0, double (&wi)[NV],
                                                 int* __restrict__ flag, double sgn) {
  constexpr int KK = kUdKK, kTriLd = kUdTriLd, kCoef = kUdCoef;
  const int tid = threadIdx.x;
  for (int j = 0; j < pn; ++j) {
    if (tid == j) {
      double d = T[j * kTriLd + j];
      bool bad = false;
#pragma unroll
      for (int q = 0; q < NV; ++q) {
        const double wj = wi[q];
        double r2 = d * d + sgn * wj * wj;
        if (!(r2 > 0.0)) {
          bad = true;
          r2 = d * d;
        }
        const double r = sqrt(r2);
        coef[(j * KK + q) * kCoef] = r / d;
        coef[(j * KK + q) * kCoef + 1] = wj / d;
        coef[(j * KK + q) * kCoef + 2] = d / r;
        d = r;
      }
      T[j * kTriLd + j] = d;
      if (bad) {
        const int p1 = p0 + j + 1;
        if (p1 < *flag) *flag = p1;
      }
    }
    __syncthreads();
    if (tid > j && tid < pn) {
      double l = T[tid * kTriLd + j];
      const double* cf = coef + j * KK * kCoef;
#pragma unroll
      for (int q = 0; q < NV; ++q) {
        const double c = cf[q * kCoef], tt = cf[q * kCoef + 1], ic = cf[q * kCoef + 2];
        l = (l + sgn * tt * wi[q]) * ic;
        wi[q] = c * wi[q] - tt * l;
      }
      T[tid * kTriLd + j] = l;
    }
  }
}

// X = inv(T): X_cc = 1 / T_cc, X_ic = -(sum_{c <= k < i} T_ik X_kc) / T_ii.  Four neighbouring lanes share
// a column (a wavefront takes 16 columns): lane part p sums k = c + p, c + p + 4, ..., the four partial
// sums meet in a butterfly (every lane ends with the same bits), part 0 stores.  A column lives in one
// wavefront, whose LDS operations execute in order: no barrier inside.
__device__ __forceinline__ void ud_panel_inverse(const double* T, double* X, int pn) {
  constexpr int kTriLd = kUdTriLd;
  const int tid = threadIdx.x;
  const int c = tid >> 2, part = tid & 3;
  const int cc = min(c, pn - 1);           // (lanes past the panel compute a copy of its last column, store nothing)
  if (part == 0 && c < pn) X[c * kTriLd + c] = 1.0 / T[c * kTriLd + c];
  for (int i = 1; i < pn; ++i) {
    double sacc = 0.0;
    if (i > cc)
      for (int k = cc + part; k < i; k += 4) sacc += T[i * kTriLd + k] * X[k * kTriLd + cc];
    sacc += __shfl_xor(sacc, 1, 64);
    sacc += __shfl_xor(sacc, 2, 64);
    if (part == 0 && c < pn && i > c) X[i * kTriLd + c] = -sacc / T[i * kTriLd + i];
  }
}

// The rows [r0, w) of the diagonal square A (w x w) below a panel of pn columns at c0, in strips of kUpdownRows:
// a row per thread with its entries of Wd (pivot position gcol0 + row) in registers across the panel's columns.
template <int NV>
__device__ __forceinline__ void ud_strip_loop(double* __restrict__ A, int w, int c0, int pn, int gcol0,
                                              double* __restrict__ Wd, const double* coef, double* tile, double sgn) {
  constexpr int KK = kUdKK, kCoef = kUdCoef;
  const int tid = threadIdx.x;
  for (int r0 = c0 + pn; r0 < w; r0 += kUpdownRows) {
    const int nr = min(kUpdownRows, w - r0);
    const int64_t vp = (int64_t)(gcol0 + r0 + tid) * KK;
    double vi[NV];
    if (tid < nr) {
#pragma unroll
      for (int q = 0; q < NV; ++q) vi[q] = Wd[vp + q];
    }
    for (int cc = 0; cc < pn; cc += kUpdownChunk)
      ud_rotate_chunk(A, w, r0, nr, c0 + cc, min(kUpdownChunk, pn - cc), coef + cc * KK * kCoef, vi, tile, sgn);
    if (tid < nr) {
#pragma unroll
      for (int q = 0; q < NV; ++q) Wd[vp + q] = vi[q];
    }
  }
}

// The diagonal square of one block column, one workgroup of 256 threads.  Panels of u.pw columns (the panels of
// the dinv slots); per panel: the triangle in LDS, walked column by column; the inverse of the new triangle into
// its slot (pn x pn row-major, lower triangle: schedule.hpp winv_offset / winv_ld with cb = pw); zeros into Wd at
// the panel's own columns (their entries are consumed); then the rows of the square below the panel.
// L, dinv, Wd, coefg, flag: of ONE factor (a member's, in the batch).  lds: kUdGenLds bytes.
template <int NV>
__device__ __forceinline__ void ud_gen_block(const SolveUnit& u, double* __restrict__ L, double* __restrict__ dinv,
                                             double* __restrict__ Wd, double* __restrict__ coefg,
                                             int* __restrict__ flag, double sgn, double* lds) {
  constexpr int KK = kUdKK, kTriLd = kUdTriLd, kCoef = kUdCoef;
  double* T = lds;
  double* X = lds + kUdGenBufA;
  double* coef = X + kUdGenBufX;
  const int tid = threadIdx.x;
  const int w = u.w, pw = u.pw;
  double* A = L + u.off;
  int64_t slot = u.dinv_off;
  for (int c0 = 0; c0 < w; c0 += pw) {
    const int pn = min(pw, w - c0);
    for (int e = tid; e < pn * pn; e += 256) {
      const int i = e / pn, j = e - i * pn;
      T[i * kTriLd + j] = A[(int64_t)(c0 + i) * w + c0 + j];
    }
    // (the block column's own columns are consecutive pivot positions)
    const int64_t wp = (int64_t)(u.gcol0 + c0 + tid) * KK;
    double wi[NV];
    if (tid < pn) {
#pragma unroll
      for (int q = 0; q < NV; ++q) wi[q] = Wd[wp + q];
    }
    __syncthreads();
    ud_walk_triangle<NV>(T, coef, pn, u.gcol0 + c0, wi, flag, sgn);
    __syncthreads();
    for (int e = tid; e < pn * pn; e += 256) {
      const int i = e / pn, j = e - i * pn;
      if (j <= i) A[(int64_t)(c0 + i) * w + c0 + j] = T[i * kTriLd + j];
    }
    for (int e = tid; e < pn * KK * kCoef; e += 256) coefg[(int64_t)c0 * KK * kCoef + e] = coef[e];
    if (tid < pn) {
#pragma unroll
      for (int q = 0; q < NV; ++q) Wd[wp + q] = 0.0;
    }
    ud_panel_inverse(T, X, pn);
    __syncthreads();
    for (int e = tid; e < pn * pn; e += 256) {
      const int i = e / pn, j = e - i * pn;
      if (j <= i) dinv[slot + (int64_t)i * pn + j] = X[i * kTriLd + j];
    }
    slot += (int64_t)pn * pn;
    ud_strip_loop<NV>(A, w, c0, pn, u.gcol0, Wd, coef, T, sgn);
    __syncthreads();
  }
}

// The rows below the diagonal square of one block column: strip g takes rows [w + 256 g, w + 256 (g + 1)).
// tile: kUdApplyTile doubles of LDS (16-byte aligned), coef: kUdApplyCoef doubles of LDS.
template <int NV>
__device__ __forceinline__ void ud_apply_block(const SolveUnit& u, double* __restrict__ L,
                                               const int* __restrict__ rlist, double* __restrict__ Wd,
                                               const double* __restrict__ coefg, double sgn, int g, double* tile,
                                               double* coef) {
  constexpr int KK = kUdKK, kCoef = kUdCoef;
  const int tid = threadIdx.x;
  const int w = u.w;
  const int row0 = w + g * kUpdownRows;
  const int nr = min(kUpdownRows, u.nrow - row0);
  double* A = L + u.off;
  int64_t wp = 0;
  double wi[NV];
  if (tid < nr) {
    wp = (int64_t)rlist[u.idx_off + row0 + tid] * KK;
#pragma unroll
    for (int q = 0; q < NV; ++q) wi[q] = Wd[wp + q];
  }
  for (int c0 = 0; c0 < w; c0 += kUpdownChunk) {
    const int cn = min(kUpdownChunk, w - c0);
    for (int e = tid; e < cn * KK * kCoef; e += 256) coef[e] = coefg[(int64_t)c0 * KK * kCoef + e];
    ud_rotate_chunk(A, w, row0, nr, c0, cn, coef, wi, tile, sgn);
  }
  if (tid < nr) {
#pragma unroll
    for (int q = 0; q < NV; ++q) Wd[wp + q] = wi[q];
  }
}

}  // namespace spx
