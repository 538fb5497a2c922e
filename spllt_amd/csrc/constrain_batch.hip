// Hard linear constraints C x = e for the members of a batch on gfx950 (include/spllt_hip_constrain_batch.h,
// DESIGN.md section 26): the bodies of cn_body.hpp on the arrays of member b, the member taken from the last grid
// dimension.  Every launch carries all members; a workgroup of a member whose flag says "not factorized" leaves at
// once (uniformly: the flag is one word per member), so nothing of that member is read or written.
//
//   k_bcn_bcast  W_b = C^T for every member (the rows of C into the member's slot of U), before the blocked solve
//   k_bcn_dot    R_b = C X_b^T: grid (chunk of n, (16 rows of C) x (16 vectors), member); partials STORED per
//                (member, chunk), chunking = cn_chunk(n)
//   k_bcn_chol   one workgroup per member: S_b from its partials in chunk order, S_b = G_b G_b^T, the pivot test
//   k_bcn_scale  U_b = W_b G_b^-T in place
//   k_bcn_small  one workgroup per member: r = C x - e, t = G_b^-1 r, lambda = G_b^-T t
//   k_bcn_apply  X_b -= U_b t, 16- and 32-wide
//   k_bcn_var    out_b,i = zdiag_b,i - sum_j U_b[j][i]^2, j ascending
//
// No atomic add, and this file is built without -munsafe-fp-atomics.  A member's sums run in the order of the
// single-handle kernels: fixed by n, k and the wavefront number, never by nbatch, nvec, a vector's place in its
// pass, the other members' data or the entry point.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "cn_body.hpp"
#include "kernels.hpp"

namespace spx {

namespace {

__device__ __forceinline__ bool bcn_skipped(const BcnView& v, int b) { return v.flag[b] != INT_MAX; }
__device__ __forceinline__ double* bcn_U(const BcnView& v, int b) { return v.U + (int64_t)b * v.k * v.n; }
__device__ __forceinline__ double* bcn_G(const BcnView& v, int b) { return v.G + (int64_t)b * kCnMaxRows * kCnMaxRows; }
__device__ __forceinline__ double* bcn_T(const BcnView& v, int b) { return v.T + (int64_t)b * kCnPass * kCnMaxRows; }

}  // namespace

__global__ __launch_bounds__(256) void k_bcn_bcast(const BcnView v) {
  const int b = blockIdx.y;
  if (bcn_skipped(v, b)) return;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < (int64_t)v.k * v.n) bcn_U(v, b)[i] = v.C[i];
}

// X: member b's vectors at X + b * xstride.  lower: the tiles of S_b on and below the diagonal (X = U).
__global__ __launch_bounds__(256) void k_bcn_dot(const BcnView v, const double* __restrict__ X, int64_t xstride, int64_t ldx,
                                                 int nv, int chunk, int ldp, int lower) {
  __shared__ double As[4][16][CN_STEP + 1];
  __shared__ double Bs[4][CN_STEP][16 + 1];
  __shared__ double Rs[4][16][16 + 1];
  const int b = blockIdx.z;
  if (bcn_skipped(v, b)) return;
  const int kt = (v.k + 15) / 16;
  const int it = (int)blockIdx.y % kt, qt = (int)blockIdx.y / kt;
  if (lower && qt > it) return;   // (uniform: the whole workgroup)
  cn_dot_body((int)blockIdx.x, it * 16, qt * 16, v.C, (int64_t)v.n, v.k, X + (int64_t)b * xstride, ldx, nv, v.n, chunk,
              v.part + (int64_t)b * v.pstride, ldp, As, Bs, Rs);
}

__global__ __launch_bounds__(256) void k_bcn_chol(const BcnView v, int nchunks) {
  __shared__ double Ss[kCnMaxRows][kCnMaxRows + 1];
  __shared__ double d0[kCnMaxRows];
  __shared__ int bad;
  __shared__ double acc[2];
  const int b = blockIdx.x;
  if (bcn_skipped(v, b)) return;
  cn_chol_body(v.part + (int64_t)b * v.pstride, nchunks, v.k, bcn_G(v, b), v.stat + (int64_t)b * kBcnStat, Ss, d0, &bad,
               acc);
}

__global__ __launch_bounds__(64) void k_bcn_scale(const BcnView v) {
  __shared__ double us[kCnMaxRows][64];
  const int b = blockIdx.y;
  if (bcn_skipped(v, b)) return;
  cn_scale_body((int)blockIdx.x * 64, bcn_U(v, b), (int64_t)v.n, v.n, v.k, bcn_G(v, b), us);
}

// e: null, or member b's targets at e + b * estride (vector q's at + q * lde; lde = 0: one column for all);
// lambda: null, or member b's multipliers at lambda + b * lstride
__global__ __launch_bounds__(256) void k_bcn_small(const BcnView v, int nchunks, int nv, const double* __restrict__ e,
                                                   int64_t estride, int64_t lde, double* __restrict__ lambda,
                                                   int64_t lstride, int64_t ldl) {
  __shared__ double Gs[kCnMaxRows][kCnMaxRows + 1];
  __shared__ double Rv[kCnMaxRows][kCnPass + 1];
  const int b = blockIdx.x;
  if (bcn_skipped(v, b)) return;
  cn_small_body(v.part + (int64_t)b * v.pstride, nchunks, v.k, nv, bcn_G(v, b), e ? e + (int64_t)b * estride : nullptr, lde,
                bcn_T(v, b), lambda ? lambda + (int64_t)b * lstride : nullptr, ldl, Gs, Rv);
}

template <int RB>
__global__ __launch_bounds__(256) void k_bcn_apply(const BcnView v, double* __restrict__ X, int64_t xstride, int64_t ldx,
                                                   int nv) {
  __shared__ double Ts[kCnMaxRows][RB + SM_PAD];
  __shared__ double Os[RB][64 + 1];
  const int b = blockIdx.y;
  if (bcn_skipped(v, b)) return;
  cn_apply_body<RB>((int)blockIdx.x * 64, X + (int64_t)b * xstride, ldx, nv, v.n, bcn_U(v, b), (int64_t)v.n, v.k,
                    bcn_T(v, b), Ts, Os);
}

// member b's row at zdiag + b * ld, in place or into out + b * ld
__global__ __launch_bounds__(256) void k_bcn_var(const BcnView v, const double* __restrict__ zdiag, int64_t ld,
                                                 double* __restrict__ out) {
  const int b = blockIdx.y;
  if (bcn_skipped(v, b)) return;
  cn_var_body((int)(blockIdx.x * 256 + threadIdx.x), zdiag + (int64_t)b * ld, bcn_U(v, b), (int64_t)v.n, v.n, v.k,
              out + (int64_t)b * ld);
}

// ---------------------------------------------------------------------------
// launchers: launches made (0: nothing to do), or -1 when the members do not fit a grid dimension
// ---------------------------------------------------------------------------
namespace {
constexpr int kMaxGridYZ = 65535;
bool bcn_fits(const BcnView& v) { return v.nbatch <= kMaxGridYZ; }
bool bcn_empty(const BcnView& v) { return v.nbatch <= 0 || v.n <= 0 || v.k <= 0; }
}  // namespace

int launch_bcn_bcast(hipStream_t st, const BcnView& v) {
  if (bcn_empty(v)) return 0;
  const int64_t blocks = ((int64_t)v.k * v.n + 255) / 256;
  if (!bcn_fits(v) || blocks > INT_MAX) return -1;
  hipLaunchKernelGGL(k_bcn_bcast, dim3((unsigned)blocks, (unsigned)v.nbatch), dim3(256), 0, st, v);
  return 1;
}

int launch_bcn_dot(hipStream_t st, const BcnView& v, const double* X, int64_t xstride, int64_t ldx, int nv, int ldp,
                   bool lower) {
  if (bcn_empty(v) || nv <= 0) return 0;
  if (!bcn_fits(v)) return -1;
  const dim3 grid((unsigned)cn_nchunks(v.n), (unsigned)(((v.k + 15) / 16) * ((nv + 15) / 16)), (unsigned)v.nbatch);
  hipLaunchKernelGGL(k_bcn_dot, grid, dim3(256), 0, st, v, X, xstride, ldx, nv, cn_chunk(v.n), ldp, lower ? 1 : 0);
  return 1;
}

int launch_bcn_chol(hipStream_t st, const BcnView& v) {
  if (bcn_empty(v)) return 0;
  hipLaunchKernelGGL(k_bcn_chol, dim3((unsigned)v.nbatch), dim3(256), 0, st, v, cn_nchunks(v.n));
  return 1;
}

int launch_bcn_scale(hipStream_t st, const BcnView& v) {
  if (bcn_empty(v)) return 0;
  if (!bcn_fits(v)) return -1;
  hipLaunchKernelGGL(k_bcn_scale, dim3((unsigned)((v.n + 63) / 64), (unsigned)v.nbatch), dim3(64), 0, st, v);
  return 1;
}

int launch_bcn_small(hipStream_t st, const BcnView& v, int nv, const double* e, int64_t estride, int64_t lde,
                     double* lambda, int64_t lstride, int64_t ldl) {
  if (bcn_empty(v) || nv <= 0) return 0;
  hipLaunchKernelGGL(k_bcn_small, dim3((unsigned)v.nbatch), dim3(256), 0, st, v, cn_nchunks(v.n), nv, e, estride, lde,
                     lambda, lstride, ldl);
  return 1;
}

int launch_bcn_apply(hipStream_t st, const BcnView& v, double* X, int64_t xstride, int64_t ldx, int nv) {
  if (bcn_empty(v) || nv <= 0) return 0;
  if (!bcn_fits(v)) return -1;
  const dim3 grid((unsigned)((v.n + 63) / 64), (unsigned)v.nbatch);
  if (nv <= 16) hipLaunchKernelGGL(k_bcn_apply<16>, grid, dim3(256), 0, st, v, X, xstride, ldx, nv);
  else hipLaunchKernelGGL(k_bcn_apply<32>, grid, dim3(256), 0, st, v, X, xstride, ldx, nv);
  return 1;
}

int launch_bcn_var(hipStream_t st, const BcnView& v, const double* zdiag, int64_t ld, double* out) {
  if (bcn_empty(v)) return 0;
  if (!bcn_fits(v)) return -1;
  hipLaunchKernelGGL(k_bcn_var, dim3((unsigned)((v.n + 255) / 256), (unsigned)v.nbatch), dim3(256), 0, st, v, zdiag, ld,
                     out);
  return 1;
}

}  // namespace spx
