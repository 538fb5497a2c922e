// The bodies of the kernels of the hard linear constraints C x = e (constrain.hip: the single handle;
// constrain_batch.hip: member b of a batch), as functions of (work item, the arrays of ONE matrix, the LDS arrays).
// One set of bodies: the batch kernels compute, per member, exactly what the single-handle kernels compute, every
// sum in the same order.  The products with the k <= 64 dense rows of C run on v_mfma_f64_16x16x4_f64 (sm_mm.hpp),
// the k x k work in one workgroup.
//
//   cn_dot_body    R = C X^T restricted to a chunk of positions: one workgroup per (chunk of n, 16 rows of C, 16
//                  vectors of X).  K runs along n, the contiguous direction of BOTH operands, so both tiles go through
//                  LDS (the 16 x 32 image of C as it lies, that of X transposed), masked to zero behind n, k and nv: a
//                  NaN in the padding of a caller's array never reaches a product.  The four wavefronts take every
//                  fourth step of 32 positions; their 16 x 16 sums are added in wavefront order and STORED per chunk.
//                  With X := W the same body gives the lower tiles of S.
//   cn_chol_body   (set time) sums the partials of S in chunk order, lower triangle only (S is symmetric by
//                  construction: the upper one is never formed), and factorizes S = G G^T in LDS, right-looking, with
//                  the pivot test of the header and log det S.
//   cn_scale_body  U = W G^-T in place: one thread per position, its k values in an LDS column, G read uniformly.
//   cn_small_body  one workgroup, G in LDS: r = sum of the partials in chunk order - e, t = G^-1 r, lambda = G^-T t.
//   cn_apply_body  X -= U t: one workgroup per 64 positions, one wavefront per 16 of them; A = U (a lane's row is a
//                  position, K = k runs over the columns of U), B = t from LDS; the result goes through LDS so that
//                  X is read and written once, in rows of 64 consecutive doubles.
//   cn_var_body    out_i = zdiag_i - sum_j U[j][i]^2, j ascending.
//
// No atomic add.  Column q of an MFMA result depends on column q of B alone, and every other sum runs in an order
// fixed by n (the chunks), k and the wavefront number: never by nv, by q's place in its pass or by the entry point.
//
// LDS: the rows of As / Bs / Rs / Os are padded by one double (an odd stride in 8-byte words: the 16 lanes that
// walk a column fall into distinct banks), the rows of Ts by SM_PAD as every B image of sm_mm.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.hpp"
#include "sm_mm.hpp"

namespace spx {

constexpr int CN_STEP = 32;   // positions per wavefront and step of cn_dot_body

// cx: the chunk; i0 / q0: the first row of C / vector of X of the 16 x 16 tile
__device__ __forceinline__ void cn_dot_body(int cx, int i0, int q0, const double* __restrict__ C, int64_t ldc, int k,
                                            const double* __restrict__ X, int64_t ldx, int nv, int n, int chunk,
                                            double* __restrict__ part, int ldp, double (*As)[16][CN_STEP + 1],
                                            double (*Bs)[CN_STEP][16 + 1], double (*Rs)[16][16 + 1]) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int p_begin = cx * chunk;
  const int p_end = min(n, p_begin + chunk);
  d4 acc[1];
  acc[0] = d4{0.0, 0.0, 0.0, 0.0};
  const int pp = lane & 31;
  for (int base = p_begin; base < p_end; base += 4 * CN_STEP) {   // (the same trip count for the four wavefronts)
    const int p = base + w * CN_STEP + pp;
    const bool okp = p < p_end;
    for (int r = lane >> 5; r < 16; r += 2) {
      As[w][r][pp] = (okp && i0 + r < k) ? C[(int64_t)(i0 + r) * ldc + p] : 0.0;
      Bs[w][pp][r] = (okp && q0 + r < nv) ? X[(int64_t)(q0 + r) * ldx + p] : 0.0;
    }
    __syncthreads();
    sm_mm<16>(&As[w][lane & 15][0], 1, CN_STEP, &Bs[w][0][0], 16 + 1, lane, acc);
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) Rs[w][(lane >> 4) + 4 * r][lane & 15] = acc[0][r];
  __syncthreads();
  const int i = threadIdx.x >> 4, q = threadIdx.x & 15;
  const double s = ((Rs[0][i][q] + Rs[1][i][q]) + Rs[2][i][q]) + Rs[3][i][q];
  part[((int64_t)cx * kCnMaxRows + i0 + i) * ldp + q0 + q] = s;
}

// stat[0]: log det S, stat[1]: the smallest pivot_j / S_jj, stat[2]: 0, or the 1-based row whose pivot failed the test
__device__ __forceinline__ void cn_chol_body(const double* __restrict__ part, int nchunks, int k, double* __restrict__ G,
                                             double* __restrict__ stat, double (*Ss)[kCnMaxRows + 1], double* d0,
                                             int* bad, double* acc) {
  const int tid = threadIdx.x;
  for (int idx = tid; idx < kCnMaxRows * kCnMaxRows; idx += 256) {
    const int i = idx >> 6, j = idx & 63;
    double s = 0.0;
    if (i < k && j <= i)
      for (int c = 0; c < nchunks; ++c) s += part[((int64_t)c * kCnMaxRows + i) * kCnMaxRows + j];
    Ss[i][j] = s;
  }
  if (tid == 0) { *bad = 0; acc[0] = 0.0; acc[1] = 1.0; }
  __syncthreads();
  if (tid < kCnMaxRows) d0[tid] = Ss[tid][tid];
  __syncthreads();
  for (int j = 0; j < k; ++j) {
    if (tid == 0) {
      const double piv = Ss[j][j];
      // (a NaN fails every comparison: !(piv > ...) catches it, and an all-zero row: 0 > 0 is false)
      if (!(piv > 0x1p-26 * d0[j]) || !isfinite(piv)) {
        *bad = j + 1;
      } else {
        const double d = sqrt(piv);
        Ss[j][j] = d;
        acc[0] += 2.0 * log(d);
        acc[1] = fmin(acc[1], piv / d0[j]);
      }
    }
    __syncthreads();
    if (*bad) break;   // (uniform: read from LDS behind the barrier)
    const double d = Ss[j][j];
    if (tid > j && tid < k) Ss[tid][j] /= d;
    __syncthreads();
    const int m = k - j - 1;   // trailing rows and columns j + 1 .. k - 1, lower part
    for (int idx = tid; idx < m * m; idx += 256) {
      const int i = j + 1 + idx / m, c = j + 1 + idx % m;
      if (c <= i) Ss[i][c] -= Ss[i][j] * Ss[c][j];
    }
    __syncthreads();
  }
  for (int idx = tid; idx < kCnMaxRows * kCnMaxRows; idx += 256) {
    const int i = idx >> 6, j = idx & 63;
    G[idx] = (i < k && j <= i) ? Ss[i][j] : 0.0;
  }
  if (tid == 0) {
    stat[0] = acc[0];
    stat[1] = acc[1];
    stat[2] = (double)*bad;
  }
}

// 64 threads, the positions p0 .. p0 + 63 (no barrier: a thread works on its own column of us)
__device__ __forceinline__ void cn_scale_body(int p0, double* __restrict__ U, int64_t ldu, int n, int k,
                                              const double* __restrict__ G, double (*us)[64]) {
  const int t = threadIdx.x;
  const int p = p0 + t;
  if (p >= n) return;
  for (int i = 0; i < k; ++i) {
    double s = U[(int64_t)i * ldu + p];
    for (int j = 0; j < i; ++j) s -= us[j][t] * G[i * kCnMaxRows + j];
    s /= G[i * kCnMaxRows + i];
    us[i][t] = s;
    U[(int64_t)i * ldu + p] = s;
  }
}

__device__ __forceinline__ void cn_small_body(const double* __restrict__ part, int nchunks, int k, int nv,
                                              const double* __restrict__ G, const double* __restrict__ e, int64_t lde,
                                              double* __restrict__ T, double* __restrict__ lambda, int64_t ldl,
                                              double (*Gs)[kCnMaxRows + 1], double (*Rv)[kCnPass + 1]) {
  const int tid = threadIdx.x;
  for (int idx = tid; idx < kCnMaxRows * kCnMaxRows; idx += 256) Gs[idx >> 6][idx & 63] = G[idx];
  for (int idx = tid; idx < kCnMaxRows * kCnPass; idx += 256) {
    const int i = idx >> 5, q = idx & 31;
    double s = 0.0;
    if (i < k && q < nv) {
      for (int c = 0; c < nchunks; ++c) s += part[((int64_t)c * kCnMaxRows + i) * kCnPass + q];
      if (e) s -= e[(int64_t)q * lde + i];
    }
    Rv[i][q] = s;
  }
  __syncthreads();
  // t = G^-1 r: column j of G leaves the rows below it, j ascending
  for (int j = 0; j < k; ++j) {
    if (tid < kCnPass) Rv[j][tid] /= Gs[j][j];
    __syncthreads();
    const int m = k - j - 1;
    for (int idx = tid; idx < m * kCnPass; idx += 256) {
      const int i = j + 1 + (idx >> 5), q = idx & 31;
      Rv[i][q] -= Gs[i][j] * Rv[j][q];
    }
    __syncthreads();
  }
  for (int idx = tid; idx < kCnMaxRows * kCnPass; idx += 256) {
    const int j = idx & 63, q = idx >> 6;
    T[idx] = Rv[j][q];   // T[q * kCnMaxRows + j]
  }
  if (!lambda) return;   // (uniform)
  __syncthreads();
  // lambda = G^-T t: row j of G leaves the entries above it, j descending
  for (int j = k - 1; j >= 0; --j) {
    if (tid < kCnPass) Rv[j][tid] /= Gs[j][j];
    __syncthreads();
    for (int idx = tid; idx < j * kCnPass; idx += 256) {
      const int i = idx >> 5, q = idx & 31;
      Rv[i][q] -= Gs[j][i] * Rv[j][q];
    }
    __syncthreads();
  }
  for (int idx = tid; idx < k * kCnPass; idx += 256) {
    const int j = idx % k, q = idx / k;
    if (q < nv) lambda[(int64_t)q * ldl + j] = Rv[j][q];
  }
}

// the positions p0 .. p0 + 63
template <int RB>
__device__ __forceinline__ void cn_apply_body(int p0, double* __restrict__ X, int64_t ldx, int nv, int n,
                                              const double* __restrict__ U, int64_t ldu, int k,
                                              const double* __restrict__ T, double (*Ts)[RB + SM_PAD],
                                              double (*Os)[64 + 1]) {
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  for (int idx = tid; idx < kCnMaxRows * RB; idx += 256) {
    const int j = idx & 63, q = idx >> 6;
    Ts[j][q] = T[q * kCnMaxRows + j];
  }
  __syncthreads();
  const int pc = min(p0 + w * 16 + (lane & 15), n - 1);   // (a row behind n repeats the last one and is dropped below)
  d4 acc[RB / 16];
#pragma unroll
  for (int c = 0; c < RB / 16; ++c) acc[c] = d4{0.0, 0.0, 0.0, 0.0};
  sm_mm<RB>(U + pc, ldu, k, &Ts[0][0], RB + SM_PAD, lane, acc);
#pragma unroll
  for (int c = 0; c < RB / 16; ++c)
#pragma unroll
    for (int r = 0; r < 4; ++r) Os[16 * c + (lane & 15)][w * 16 + (lane >> 4) + 4 * r] = acc[c][r];
  __syncthreads();
  for (int idx = tid; idx < RB * 64; idx += 256) {
    const int q = idx >> 6, p = p0 + (idx & 63);
    if (q < nv && p < n) X[(int64_t)q * ldx + p] -= Os[q][idx & 63];
  }
}

__device__ __forceinline__ void cn_var_body(int i, const double* __restrict__ zdiag, const double* __restrict__ U,
                                            int64_t ldu, int n, int k, double* __restrict__ out) {
  if (i >= n) return;
  double s = 0.0;
  for (int j = 0; j < k; ++j) {
    const double u = U[(int64_t)j * ldu + i];
    s += u * u;
  }
  out[i] = zdiag[i] - s;
}

}  // namespace spx
