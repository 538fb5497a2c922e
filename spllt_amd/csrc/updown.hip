// Sparse low-rank update / downdate of the factor on gfx950: L L^T + sign W W^T, in place, on the block
// columns of the elimination-tree paths of W's columns (schedule.hpp build_updown_plan).
//
//   k_updown_scatter   the entries of up to kUpdownVec columns of W into the work array Wd[p * kUpdownVec + q]
//                      (pivot position p, vector q), which is zero between calls
//   k_updown_gen       one workgroup per visited block column walks its diagonal square panel by panel: the
//                      rotation coefficients (c, t, 1 / c) of every column and vector, the rotated square,
//                      inv(L_pp) of every panel into its dinv slot, zeros into Wd at the block column's own
//                      columns (their entries are consumed)
//                      (built for 1, 2, 4 and 8 vectors per pass, like the apply kernel: a single vector does
//                      not pay for seven identity rotations)
//   k_updown_apply     the rows below the square, 256 rows per workgroup, a row per thread with its kUpdownVec
//                      entries of Wd in registers across all the columns; L staged through LDS in chunks of
//                      kUpdownChunk columns, one read and one write of the strip
//
// Per column j and vector q (in this order, q fastest):
//   d = L_jj, r = sqrt(d d + sign w_j w_j), c = r / d, t = w_j / d, L_jj = r
//   rows i > j:  L_ij = (L_ij + sign t w_i) / c,  w_i = c w_i - t L_ij
// w_j = 0 gives c = 1, t = 0: the identity, bit for bit.  No atomics; a row belongs to one thread.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>

#include "kernels.hpp"

namespace spx {

namespace {

constexpr int KK = kUpdownVec;
constexpr int kTileLd = kUpdownChunk + 1;        // doubles: lanes of a half wavefront on distinct banks
constexpr int kTriLd = kPanelMax + 1;
constexpr int kCoef = 3;                         // c, t, 1 / c
// LDS of k_updown_gen (doubles): the panel's triangle, later the row tile; the inverse; the panel's coefficients
constexpr int kGenBufA = kUpdownRows * kTileLd > kPanelMax * kTriLd ? kUpdownRows * kTileLd : kPanelMax * kTriLd;
constexpr int kGenBufX = kPanelMax * kTriLd;
constexpr int kGenCoef = kPanelMax * KK * kCoef;
constexpr size_t kGenLds = sizeof(double) * (size_t)(kGenBufA + kGenBufX + kGenCoef);

__global__ __launch_bounds__(256) void k_updown_scatter(const int64_t* __restrict__ pos, const double* __restrict__ val,
                                                        int64_t count, double* __restrict__ Wd, int* __restrict__ flag,
                                                        int reset_flag) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < count) Wd[pos[i]] = val[i];
  if (reset_flag && i == 0) *flag = INT_MAX;
}

// Rows [row0, row0 + nr) of the block column A (row width ld), columns [c0, c0 + cn), nr <= kUpdownRows, cn <=
// kUpdownChunk: into the LDS tile with coalesced loads (16 bytes per lane where the rows are 16-byte aligned),
// thread i rotates row i with the chunk's coefficients coef[(j * KK + q) * 3 ..] (LDS) and its wi[], and back.
// Every thread of the workgroup calls it; it ends with a barrier (tile and coef may be rewritten after it).
template <int NV>
__device__ __forceinline__ void ud_rotate_chunk(double* __restrict__ A, int ld, int row0, int nr, int c0, int cn,
                                                const double* coef, double (&wi)[NV], double* tile, double sgn) {
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

// The diagonal square of one block column, one workgroup.  Panels of u.pw columns (the panels of the dinv
// slots); per panel: the triangle in LDS, walked column by column by the threads of its rows (thread j makes
// the coefficients of column j for all vectors -- they depend on L_jj and on its own w_j only -- the threads
// below apply them); the inverse of the new triangle, four lanes per column; then the rows of the square below
// the panel in strips of 256.  A downdate that meets d d - w_j w_j <= 0 records the pivot position + 1 in
// *flag (the smallest one: the workgroups of a sweep run one after the other) and goes on with r = d.
template <int NV>
__global__ __launch_bounds__(256) void k_updown_gen(const SolveUnit u, double* __restrict__ L, double* __restrict__ dinv,
                                                    double* __restrict__ Wd, double* __restrict__ coefg,
                                                    int* __restrict__ flag, double sgn) {
  extern __shared__ __attribute__((aligned(16))) double ud_lds[];
  double* T = ud_lds;
  double* X = ud_lds + kGenBufA;
  double* coef = X + kGenBufX;
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
          const int p1 = u.gcol0 + c0 + j + 1;
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
    {
      // X = inv(T): X_cc = 1 / T_cc, X_ic = -(sum_{c <= k < i} T_ik X_kc) / T_ii.  Four neighbouring lanes share
      // a column (a wavefront takes 16 columns): lane part p sums k = c + p, c + p + 4, ..., the four partial
      // sums meet in a butterfly (every lane ends with the same bits), part 0 stores.  A column lives in one
      // wavefront, whose LDS operations execute in order: no barrier inside.
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
    __syncthreads();
    // the slot of panel p: pn x pn row-major, lower triangle (schedule.hpp winv_offset / winv_ld with cb = pw)
    for (int e = tid; e < pn * pn; e += 256) {
      const int i = e / pn, j = e - i * pn;
      if (j <= i) dinv[slot + (int64_t)i * pn + j] = X[i * kTriLd + j];
    }
    slot += (int64_t)pn * pn;
    for (int r0 = c0 + pn; r0 < w; r0 += kUpdownRows) {
      const int nr = min(kUpdownRows, w - r0);
      const int64_t vp = (int64_t)(u.gcol0 + r0 + tid) * KK;
      double vi[NV];
      if (tid < nr) {
#pragma unroll
        for (int q = 0; q < NV; ++q) vi[q] = Wd[vp + q];
      }
      for (int cc = 0; cc < pn; cc += kUpdownChunk)
        ud_rotate_chunk(A, w, r0, nr, c0 + cc, min(kUpdownChunk, pn - cc), coef + cc * KK * kCoef, vi, T, sgn);
      if (tid < nr) {
#pragma unroll
        for (int q = 0; q < NV; ++q) Wd[vp + q] = vi[q];
      }
    }
    __syncthreads();
  }
}

// The rows below the diagonal square of one block column: workgroup g takes rows [w + 256 g, w + 256 (g + 1)).
template <int NV>
__global__ __launch_bounds__(256) void k_updown_apply(const SolveUnit u, double* __restrict__ L,
                                                      const int* __restrict__ rlist, double* __restrict__ Wd,
                                                      const double* __restrict__ coefg, double sgn) {
  __shared__ __attribute__((aligned(16))) double tile[kUpdownRows * kTileLd];
  __shared__ double coef[kUpdownChunk * KK * kCoef];
  const int tid = threadIdx.x;
  const int w = u.w;
  const int row0 = w + (int)blockIdx.x * kUpdownRows;
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

}  // namespace

void launch_updown_scatter(hipStream_t st, const int64_t* pos, const double* val, int64_t count, double* Wd, int* flag,
                           bool reset_flag) {
  const unsigned grid = (unsigned)std::max<int64_t>(1, (count + 255) / 256);
  hipLaunchKernelGGL(k_updown_scatter, dim3(grid), dim3(256), 0, st, pos, val, count, Wd, flag, reset_flag ? 1 : 0);
}

namespace {
template <int NV>
void gen_nv(hipStream_t st, const SolveUnit& u, double* L, double* dinv, double* Wd, double* coef, int* flag, int sign) {
  thread_local int attr_dev = -1;      // (more than 64 KiB of dynamic LDS: allowed per device)
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (dev != attr_dev) {
    (void)hipFuncSetAttribute((const void*)k_updown_gen<NV>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kGenLds);
    attr_dev = dev;
  }
  hipLaunchKernelGGL(k_updown_gen<NV>, dim3(1), dim3(256), kGenLds, st, u, L, dinv, Wd, coef, flag, (double)sign);
}
}  // namespace

// nv: the vectors of the pass; the kernels are built for 1, 2, 4 and 8 (the next of these: the vectors beyond
// nv are zero in Wd, and a zero vector is the identity)
void launch_updown_gen(hipStream_t st, const SolveUnit& u, double* L, double* dinv, double* Wd, double* coef, int* flag,
                       int sign, int nv) {
  if (nv <= 1) gen_nv<1>(st, u, L, dinv, Wd, coef, flag, sign);
  else if (nv == 2) gen_nv<2>(st, u, L, dinv, Wd, coef, flag, sign);
  else if (nv <= 4) gen_nv<4>(st, u, L, dinv, Wd, coef, flag, sign);
  else gen_nv<8>(st, u, L, dinv, Wd, coef, flag, sign);
}

void launch_updown_apply(hipStream_t st, const SolveUnit& u, double* L, const int* rlist, double* Wd, const double* coef,
                         int sign, int nv) {
  const int below = u.nrow - u.w;
  if (below <= 0) return;
  const dim3 grid((unsigned)((below + kUpdownRows - 1) / kUpdownRows));
  const double sgn = (double)sign;
  if (nv <= 1) hipLaunchKernelGGL(k_updown_apply<1>, grid, dim3(256), 0, st, u, L, rlist, Wd, coef, sgn);
  else if (nv == 2) hipLaunchKernelGGL(k_updown_apply<2>, grid, dim3(256), 0, st, u, L, rlist, Wd, coef, sgn);
  else if (nv <= 4) hipLaunchKernelGGL(k_updown_apply<4>, grid, dim3(256), 0, st, u, L, rlist, Wd, coef, sgn);
  else hipLaunchKernelGGL(k_updown_apply<8>, grid, dim3(256), 0, st, u, L, rlist, Wd, coef, sgn);
}

}  // namespace spx
