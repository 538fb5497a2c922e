// Hard linear constraints C x = e on gfx950 (include/spllt_hip_constrain.h): the products
// with the k <= 64 dense rows of C on v_mfma_f64_16x16x4_f64 (sm_mm.hpp), the k x k work in one workgroup.  The
// kernels are the bodies of cn_body.hpp (which describes them) on the arrays of the single handle; the members of a
// batch run the same bodies in constrain_batch.hip.
//
//   k_cn_dot     R = C X^T, one workgroup per (chunk of n, 16 rows of C, 16 vectors of X), partials STORED per chunk
//   k_cn_chol    (set time) S from its partials in chunk order, S = G G^T with the pivot test, log det S
//   k_cn_scale   U = W G^-T in place
//   k_cn_small   one workgroup: r = sum of the partials in chunk order - e, t = G^-1 r, lambda = G^-T t
//   k_cn_apply   X -= U t, one workgroup per 64 positions
//   k_cn_var     out_i = zdiag_i - sum_j U[j][i]^2, j ascending
//
// No atomic add.  Column q of an MFMA result depends on column q of B alone, and every other sum runs in an order
// fixed by n (the chunks), k and the wavefront number: never by nv, by q's place in its pass or by the entry point.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "cn_body.hpp"
#include "kernels.hpp"

namespace spx {

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
  cn_dot_body((int)blockIdx.x, (int)blockIdx.y * 16, (int)blockIdx.z * 16, C, ldc, k, X, ldx, nv, n, chunk, part, ldp,
              As, Bs, Rs);
}

__global__ __launch_bounds__(256) void k_cn_chol(const double* __restrict__ part, int nchunks, int k,
                                                 double* __restrict__ G, double* __restrict__ stat) {
  __shared__ double Ss[kCnMaxRows][kCnMaxRows + 1];
  __shared__ double d0[kCnMaxRows];
  __shared__ int bad;
  __shared__ double acc[2];
  cn_chol_body(part, nchunks, k, G, stat, Ss, d0, &bad, acc);
}

__global__ __launch_bounds__(64) void k_cn_scale(double* __restrict__ U, int64_t ldu, int n, int k,
                                                 const double* __restrict__ G) {
  __shared__ double us[kCnMaxRows][64];
  cn_scale_body((int)blockIdx.x * 64, U, ldu, n, k, G, us);
}

__global__ __launch_bounds__(256) void k_cn_small(const double* __restrict__ part, int nchunks, int k, int nv,
                                                  const double* __restrict__ G, const double* __restrict__ e, int64_t lde,
                                                  double* __restrict__ T, double* __restrict__ lambda, int64_t ldl) {
  __shared__ double Gs[kCnMaxRows][kCnMaxRows + 1];
  __shared__ double Rv[kCnMaxRows][kCnPass + 1];
  cn_small_body(part, nchunks, k, nv, G, e, lde, T, lambda, ldl, Gs, Rv);
}

template <int RB>
__global__ __launch_bounds__(256) void k_cn_apply(double* __restrict__ X, int64_t ldx, int nv, int n,
                                                  const double* __restrict__ U, int64_t ldu, int k,
                                                  const double* __restrict__ T) {
  __shared__ double Ts[kCnMaxRows][RB + SM_PAD];
  __shared__ double Os[RB][64 + 1];
  cn_apply_body<RB>((int)blockIdx.x * 64, X, ldx, nv, n, U, ldu, k, T, Ts, Os);
}

__global__ __launch_bounds__(256) void k_cn_var(const double* __restrict__ zdiag, const double* __restrict__ U, int64_t ldu,
                                                int n, int k, double* __restrict__ out) {
  cn_var_body((int)(blockIdx.x * 256 + threadIdx.x), zdiag, U, ldu, n, k, out);
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
