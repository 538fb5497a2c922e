// Selected inversion on gfx950: Z = (P A P^T)^-1 on the pattern of L (schedule.hpp,
// SelinvProgram), plus diag(A^-1) and log det A.
//
//   k_selinv_symm / _scale / _diag   the three step kernels on the handle's one arena; their bodies live in
//                   si_body.hpp (its header describes the steps and the MFMA lane map), shared with the batch.
//                   k_selinv_scale keeps its own copy of si_scale_body's text: see the comment in front of it
//   k_selinv_diag_gather   (A^-1)_ii in the user's variable order
//   k_log_det       2 sum log L_jj, a fixed-order reduction in one workgroup
// Every sum runs in a fixed order: two runs on the same L give a bit-identical Z.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.hpp"
#include "si_body.hpp"

namespace spx {

// kDoubleDiag = true is the SYMM step of the factor adjoint (factor_adjoint.hip): Z is then the adjoint arena
template <bool kDoubleDiag>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_selinv_symm(const UpdTile* __restrict__ tiles, const SelinvUnit* __restrict__ units,
                                                     const SelinvRow* __restrict__ rows, const int* __restrict__ relpos,
                                                     const double* __restrict__ L, const double* __restrict__ Z,
                                                     double* __restrict__ scratch) {
  __shared__ double As[SI_T][SI_KC + 1];
  __shared__ double Bs[SI_KC][SI_T + 1];
  __shared__ SelinvRow Ri[SI_T];
  const UpdTile t = tiles[blockIdx.x];
  si_symm_body<kDoubleDiag>(t, units[t.unit], rows, relpos, L, Z, scratch, As, Bs, Ri);
}

// si_scale_body of si_body.hpp, statement for statement, NOT called: inlined from the header the compiler
// allocates 54 registers per lane where this text gets 68, which crosses the 64-register occupancy step
// (profiles/selinv_body/README.md).  A change to one of the two texts goes into the other.
__global__ __launch_bounds__(256) void k_selinv_scale(const UpdTile* __restrict__ tiles, const SelinvUnit* __restrict__ units,
                                                      const double* __restrict__ L, const double* __restrict__ dinv,
                                                      double* __restrict__ Z, double* __restrict__ scratch) {
  __shared__ double Ys[SI_T][SI_T + 1];
  __shared__ double Ms[SI_T][SI_T + 1];   // inv(L_JJ), then the tile's rows of L_RJ
  const UpdTile t = tiles[blockIdx.x];
  const SelinvUnit u = units[t.unit];
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

__global__ __launch_bounds__(1024) void k_selinv_diag(const SelinvUnit* __restrict__ units, const double* __restrict__ dinv,
                                                     double* __restrict__ Z, const double* __restrict__ scratch) {
  __shared__ double Ds[SI_T][SI_T + 1];
  __shared__ double Ts[SI_T][SI_T + 1];
  si_diag_body(units[blockIdx.x], dinv, Z, scratch, Ds, Ts);
}

__global__ __launch_bounds__(256) void k_selinv_diag_gather(const double* __restrict__ Z, const int64_t* __restrict__ diag_pos,
                                                            const int* __restrict__ order, int n, double* __restrict__ out) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v < n) out[v] = Z[diag_pos[order[v]]];
}

// 2 sum_j log L_jj: thread t sums j = t, t + 1024, ... in order, then a fixed tree in LDS
__global__ __launch_bounds__(1024) void k_log_det(const double* __restrict__ L, const int64_t* __restrict__ diag_pos, int n,
                                                  double* __restrict__ out) {
  __shared__ double part[1024];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int j = tid; j < n; j += 1024) s += log(L[diag_pos[j]]);
  part[tid] = s;
  __syncthreads();
  for (int w = 512; w > 0; w >>= 1) {
    if (tid < w) part[tid] += part[tid + w];
    __syncthreads();
  }
  if (tid == 0) out[0] = 2.0 * part[0];
}

void launch_selinv(hipStream_t st, const SelinvLaunch& l, const SelinvUnit* units, const UpdTile* tiles,
                   const SelinvRow* rows, const int* relpos, const double* L, const double* dinv, double* Z,
                   double* scratch) {
  if (l.count <= 0) return;
  const dim3 grid((unsigned)l.count), block(256);
  if (l.kind == SI_SYMM)
    hipLaunchKernelGGL(k_selinv_symm<false>, grid, block, 0, st, tiles + l.first, units, rows, relpos, L, (const double*)Z, scratch);
  else if (l.kind == SI_SCALE)
    hipLaunchKernelGGL(k_selinv_scale, grid, block, 0, st, tiles + l.first, units, L, dinv, Z, scratch);
  else
    hipLaunchKernelGGL(k_selinv_diag, grid, dim3(1024), 0, st, units + l.first, dinv, Z, (const double*)scratch);
}

void launch_selinv_symm_doubled(hipStream_t st, const SelinvLaunch& l, const SelinvUnit* units, const UpdTile* tiles,
                                const SelinvRow* rows, const int* relpos, const double* L, const double* G,
                                double* scratch) {
  if (l.count <= 0 || l.kind != SI_SYMM) return;
  hipLaunchKernelGGL(k_selinv_symm<true>, dim3((unsigned)l.count), dim3(256), 0, st, tiles + l.first, units, rows, relpos,
                     L, G, scratch);
}

void launch_selinv_diag_gather(hipStream_t st, const double* Z, const int64_t* diag_pos, const int* order, int n,
                               double* out) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_selinv_diag_gather, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, Z, diag_pos, order, n, out);
}

void launch_log_det(hipStream_t st, const double* L, const int64_t* diag_pos, int n, double* out) {
  hipLaunchKernelGGL(k_log_det, dim3(1), dim3(1024), 0, st, L, diag_pos, n, out);
}

}  // namespace spx
