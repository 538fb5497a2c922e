// Hard linear constraints C x = e on gfx950 (include/spllt_hip_constrain.h): the products
// with the k <= 64 dense rows of C on v_mfma_f64_16x16x4_f64 (sm_mm.hpp), the k x k work in one workgroup.
//
//   k_cn_dot     R = C X^T restricted to a chunk of positions: one workgroup per (chunk of n, 16 rows of C, 16
//                vectors of X).  K runs along n, the contiguous direction of BOTH operands, so both tiles go through
//                LDS (the 16 x 32 image of C as it lies, that of X transposed), masked to zero behind n, k and nv: a
//                NaN in the padding of a caller's array never reaches a product.  The four wavefronts take every
//                fourth step of 32 positions; their 16 x 16 sums are added in wavefront order and STORED per chunk.
//                With X := W the same kernel gives the lower tiles of S.
//   k_cn_chol    (set time) sums the partials of S in chunk order, lower triangle only (S is symmetric by
//                construction: the upper one is never formed), and factorizes S = G G^T in LDS, right-looking, with
//                the pivot test of the header and log det S.
//   k_cn_scale   U = W G^-T in place: one thread per position, its k values in an LDS column, G read uniformly.
//   k_cn_small   one workgroup, G in LDS: r = sum of the partials in chunk order - e, t = G^-1 r, lambda = G^-T t.
//   k_cn_apply   X -= U t: one workgroup per 64 positions, one wavefront per 16 of them; A = U (a lane's row is a
//                position, K = k runs over the columns of U), B = t from LDS; the result goes through LDS so that
//                X is read and written once, in rows of 64 consecutive doubles.
//   k_cn_var     out_i = zdiag_i - sum_j U[j][i]^2, j ascending.
//
// No atomic add.  Column q of an MFMA result depends on column q of B alone, and every other sum runs in an order
// fixed by n (the chunks), k and the wavefront number: never by nv, by q's place in its pass or by the entry point.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.hpp"
#include "sm_mm.hpp"

namespace spx {

constexpr int CN_STEP = 32;   // positions per wavefront and step of k_cn_dot

// positions per chunk: a multiple of 64, at most 256 chunks (one workgroup of k_cn_small sums them)
int cn_chunk(int n) {
  const int per = (n + 255) / 256;
  const int c = (per + 63) / 64 * 64;
  return c < 64 ? 64 : c;
}

__global__ __launch_bounds__(256) void k_cn_dot(const double* __restrict__ C, int64_t ldc, int k,
                                                const double* __restrict__ X, int64_t ldx, int nv, int n, int chunk,
                                                double* __restrict__ part, int ldp, int lower) {
  __shared__ double As[4][16][CN_STEP + 1];
  __shared__ double Bs[4][CN_STEP][16 + 1];
  __shared__ double Rs[4][16][16 + 1];
  if (lower && blockIdx.z > blockIdx.y) return;   // (uniform: the whole workgroup)
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int i0 = blockIdx.y * 16, q0 = blockIdx.z * 16;
  const int p_begin = blockIdx.x * chunk;
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
  part[((int64_t)blockIdx.x * kCnMaxRows + i0 + i) * ldp + q0 + q] = s;
}

__global__ __launch_bounds__(256) void k_cn_chol(const double* __restrict__ part, int nchunks, int k,
                                                 double* __restrict__ G, double* __restrict__ stat) {
  __shared__ double Ss[kCnMaxRows][kCnMaxRows + 1];
  __shared__ double d0[kCnMaxRows];
  __shared__ int bad;
  __shared__ double acc[2];
  const int tid = threadIdx.x;
  for (int idx = tid; idx < kCnMaxRows * kCnMaxRows; idx += 256) {
    const int i = idx >> 6, j = idx & 63;
    double s = 0.0;
    if (i < k && j <= i)
      for (int c = 0; c < nchunks; ++c) s += part[((int64_t)c * kCnMaxRows + i) * kCnMaxRows + j];
    Ss[i][j] = s;
  }
  if (tid == 0) { bad = 0; acc[0] = 0.0; acc[1] = 1.0; }
  __syncthreads();
  if (tid < kCnMaxRows) d0[tid] = Ss[tid][tid];
  __syncthreads();
  for (int j = 0; j < k; ++j) {
    if (tid == 0) {
      const double piv = Ss[j][j];
      // (a NaN fails every comparison: !(piv > ...) catches it, and an all-zero row: 0 > 0 is false)
      if (!(piv > 0x1p-26 * d0[j]) || !isfinite(piv)) {
        bad = j + 1;
      } else {
        const double d = sqrt(piv);
        Ss[j][j] = d;
        acc[0] += 2.0 * log(d);
        acc[1] = fmin(acc[1], piv / d0[j]);
      }
    }
    __syncthreads();
    if (bad) break;   // (uniform: read from LDS behind the barrier)
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
    stat[2] = (double)bad;
  }
}

__global__ __launch_bounds__(64) void k_cn_scale(double* __restrict__ U, int64_t ldu, int n, int k,
                                                 const double* __restrict__ G) {
  __shared__ double us[kCnMaxRows][64];
  const int t = threadIdx.x;
  const int p = blockIdx.x * 64 + t;
  if (p >= n) return;   // (no barrier below: a thread works on its own column of us)
  for (int i = 0; i < k; ++i) {
    double s = U[(int64_t)i * ldu + p];
    for (int j = 0; j < i; ++j) s -= us[j][t] * G[i * kCnMaxRows + j];
    s /= G[i * kCnMaxRows + i];
    us[i][t] = s;
    U[(int64_t)i * ldu + p] = s;
  }
}

__global__ __launch_bounds__(256) void k_cn_small(const double* __restrict__ part, int nchunks, int k, int nv,
                                                  const double* __restrict__ G, const double* __restrict__ e, int64_t lde,
                                                  double* __restrict__ T, double* __restrict__ lambda, int64_t ldl) {
  __shared__ double Gs[kCnMaxRows][kCnMaxRows + 1];
  __shared__ double Rv[kCnMaxRows][kCnPass + 1];
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

template <int RB>
__global__ __launch_bounds__(256) void k_cn_apply(double* __restrict__ X, int64_t ldx, int nv, int n,
                                                  const double* __restrict__ U, int64_t ldu, int k,
                                                  const double* __restrict__ T) {
  __shared__ double Ts[kCnMaxRows][RB + SM_PAD];
  __shared__ double Os[RB][64 + 1];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  for (int idx = tid; idx < kCnMaxRows * RB; idx += 256) {
    const int j = idx & 63, q = idx >> 6;
    Ts[j][q] = T[q * kCnMaxRows + j];
  }
  __syncthreads();
  const int p0 = blockIdx.x * 64;
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

__global__ __launch_bounds__(256) void k_cn_var(const double* __restrict__ zdiag, const double* __restrict__ U, int64_t ldu,
                                                int n, int k, double* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
  for (int j = 0; j < k; ++j) {
    const double u = U[(int64_t)j * ldu + i];
    s += u * u;
  }
  out[i] = zdiag[i] - s;
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
void launch_cn_dot(hipStream_t st, const double* C, int64_t ldc, int k, const double* X, int64_t ldx, int nv, int n,
                   double* part, int ldp, bool lower) {
  if (n <= 0 || k <= 0 || nv <= 0) return;
  const dim3 grid((unsigned)cn_nchunks(n), (unsigned)((k + 15) / 16), (unsigned)((nv + 15) / 16));
  hipLaunchKernelGGL(k_cn_dot, grid, dim3(256), 0, st, C, ldc, k, X, ldx, nv, n, cn_chunk(n), part, ldp, lower ? 1 : 0);
}

void launch_cn_chol(hipStream_t st, const double* part, int nchunks, int k, double* G, double* stat) {
  hipLaunchKernelGGL(k_cn_chol, dim3(1), dim3(256), 0, st, part, nchunks, k, G, stat);
}

void launch_cn_scale(hipStream_t st, double* U, int64_t ldu, int n, int k, const double* G) {
  if (n <= 0 || k <= 0) return;
  hipLaunchKernelGGL(k_cn_scale, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, U, ldu, n, k, G);
}

void launch_cn_small(hipStream_t st, const double* part, int nchunks, int k, int nv, const double* G, const double* e,
                     int64_t lde, double* T, double* lambda, int64_t ldl) {
  hipLaunchKernelGGL(k_cn_small, dim3(1), dim3(256), 0, st, part, nchunks, k, nv, G, e, lde, T, lambda, ldl);
}

void launch_cn_apply(hipStream_t st, double* X, int64_t ldx, int nv, int n, const double* U, int64_t ldu, int k,
                     const double* T) {
  if (n <= 0 || k <= 0 || nv <= 0) return;
  const dim3 grid((unsigned)((n + 63) / 64));
  if (nv <= 16) hipLaunchKernelGGL(k_cn_apply<16>, grid, dim3(256), 0, st, X, ldx, nv, n, U, ldu, k, T);
  else hipLaunchKernelGGL(k_cn_apply<32>, grid, dim3(256), 0, st, X, ldx, nv, n, U, ldu, k, T);
}

void launch_cn_var(hipStream_t st, const double* zdiag, const double* U, int64_t ldu, int n, int k, double* out) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_cn_var, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, zdiag, U, ldu, n, k, out);
}

}  // namespace spx
