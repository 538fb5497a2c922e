// Sparse right-hand sides and selected outputs for every member of a batch on gfx950: what
// a restricted solve needs around the unchanged sweep kernels of batch_solve_many.hip, on the workspaces W_b =
// W + b * wstride (W_b[p * RB + q], pivot position p, right-hand side q < RB = 16 or 32).  The bodies are the SAME
// device functions as solve_sparse.hip's (ss_body.hpp).  No atomics in this translation unit.
//
//   k_bss_zero          the touched rows (the shared chunk list) of every member's workspace set to zero
//   k_bss_scatter       W_b[pos[i]] = val[b * ldv + i] (ldv = 0: one set of values for all members)
//   k_bss_gather        x[b * xstride + q * ldx + t] = W_b[pos[t] * RB + q]
//   k_bss_gram          per (chunk, member): the 32 x 32 product Y_{b,I}^T Y_{b,J} on v_mfma_f64_16x16x4_f64
//   k_bss_gram_reduce   per member: the blocks of one pair of groups added in ascending chunk order, with the mirror
//
// One launch carries all members on a linear grid: workgroup -> (member = wg / items, item = wg % items), the
// workgroups of one member consecutive.  A workgroup whose member is flagged (not positive definite) tests the
// flag before any barrier: gather and reduce write NaN to that member's outputs, the others return.  The members
// of a launch are split into ranges when (items x members) passes batch_grid_limit().
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <limits>

#include "batch_split.hpp"
#include "kernels.hpp"
#include "ss_body.hpp"

namespace spx {

template <int RB>
__global__ __launch_bounds__(256) void k_bss_zero(const int* __restrict__ flag, const int* __restrict__ chunks,
                                                  unsigned nchunk, double* __restrict__ W, int64_t wstride) {
  const unsigned b = blockIdx.x / nchunk, c = blockIdx.x % nchunk;
  if (flag[b] != INT_MAX) return;
  ss_zero_body<RB>(chunks[2 * c], chunks[2 * c + 1], W + (int64_t)b * wstride);
}

__global__ __launch_bounds__(256) void k_bss_scatter(const int* __restrict__ flag, const int64_t* __restrict__ pos,
                                                     const double* __restrict__ val, int64_t ldv, int64_t count,
                                                     unsigned nblk, double* __restrict__ W, int64_t wstride) {
  const unsigned b = blockIdx.x / nblk;
  if (flag[b] != INT_MAX) return;
  const int64_t i = (int64_t)(blockIdx.x % nblk) * 256 + threadIdx.x;
  if (i < count) W[(int64_t)b * wstride + pos[i]] = val[(int64_t)b * ldv + i];
}

template <int RB>
__global__ __launch_bounds__(256) void k_bss_gather(const int* __restrict__ flag, double* __restrict__ x, int64_t xstride,
                                                    int64_t ldx, const int* __restrict__ pos, int64_t nsel, int nv,
                                                    unsigned nblk, const double* __restrict__ W, int64_t wstride) {
  __shared__ double tile[64][RB + 1];
  const unsigned b = blockIdx.x / nblk;
  const int64_t t0 = (int64_t)(blockIdx.x % nblk) * 64;
  double* xb = x + (int64_t)b * xstride;
  if (flag[b] != INT_MAX) {   // (before any barrier)
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int e = threadIdx.x; e < 64 * RB; e += 256) {
      const int tt = e & 63, q = e >> 6;
      if (t0 + tt < nsel && q < nv) xb[(int64_t)q * ldx + t0 + tt] = nan;
    }
    return;
  }
  ss_gather_body<RB>(t0, xb, ldx, pos, nsel, nv, W + (int64_t)b * wstride, tile);
}

// part_b[chunk][i][j]; only the chunk's rows of member b's two workspaces are read
__global__ __launch_bounds__(256) void k_bss_gram(const int* __restrict__ flag, const int* __restrict__ chunks,
                                                  unsigned nchunk, const double* __restrict__ WI, int64_t wsI, int rbI,
                                                  const double* __restrict__ WJ, int64_t wsJ, int rbJ,
                                                  double* __restrict__ part) {
  __shared__ double red[4][32][33];
  const unsigned b = blockIdx.x / nchunk, c = blockIdx.x % nchunk;
  if (flag[b] != INT_MAX) return;
  ss_gram_body(chunks[2 * c], chunks[2 * c + 1], WI + (int64_t)b * wsI, rbI, WJ + (int64_t)b * wsJ, rbJ,
               part + ((int64_t)b * nchunk + c) * 1024, red);
}

__global__ __launch_bounds__(256) void k_bss_gram_reduce(const int* __restrict__ flag, const double* __restrict__ part,
                                                         int nchunk, int nvI, int nvJ, int diag, double* __restrict__ Gij,
                                                         double* __restrict__ Gji, int64_t gstride, int64_t ldg) {
  const unsigned b = blockIdx.x;
  double* gij = Gij + (int64_t)b * gstride;
  double* gji = Gji + (int64_t)b * gstride;
  if (flag[b] != INT_MAX) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int e = threadIdx.x; e < 1024; e += 256) {
      const int i = e >> 5, j = e & 31;
      if (i >= nvI || j >= nvJ || (diag && i < j)) continue;
      gij[(int64_t)j * ldg + i] = nan;
      gji[(int64_t)i * ldg + j] = nan;
    }
    return;
  }
  ss_gram_reduce_body(part + (int64_t)b * nchunk * 1024, nchunk, nvI, nvJ, diag, gij, gji, ldg);
}

// ---------------------------------------------------------------------------
// launch wrappers: launches made, or -1 (nothing launched) when ONE member's work items overflow a grid
// ---------------------------------------------------------------------------
int launch_bss_zero(hipStream_t st, const BssView& s, const int* chunks, int nchunk, int rb, double* W, int64_t wstride) {
  return batch_member_ranges(s.nbatch, nchunk, [&](int b0, int nb) {
    const dim3 g((unsigned)((int64_t)nchunk * nb)), b(256);
    double* Ws = W + (int64_t)b0 * wstride;
    if (rb == 32)
      hipLaunchKernelGGL((k_bss_zero<32>), g, b, 0, st, s.flag + b0, chunks, (unsigned)nchunk, Ws, wstride);
    else
      hipLaunchKernelGGL((k_bss_zero<16>), g, b, 0, st, s.flag + b0, chunks, (unsigned)nchunk, Ws, wstride);
  });
}

int launch_bss_scatter(hipStream_t st, const BssView& s, const int64_t* pos, const double* val, int64_t ldv,
                       int64_t count, double* W, int64_t wstride) {
  const int64_t nblk = (count + 255) / 256;
  return batch_member_ranges(s.nbatch, nblk, [&](int b0, int nb) {
    hipLaunchKernelGGL(k_bss_scatter, dim3((unsigned)(nblk * nb)), dim3(256), 0, st, s.flag + b0, pos,
                       val + (int64_t)b0 * ldv, ldv, count, (unsigned)nblk, W + (int64_t)b0 * wstride, wstride);
  });
}

int launch_bss_gather(hipStream_t st, const BssView& s, double* x, int64_t xstride, int64_t ldx, const int* pos,
                      int64_t nsel, int nv, int rb, const double* W, int64_t wstride) {
  if (nsel <= 0 || nv <= 0) return 0;
  const int64_t nblk = (nsel + 63) / 64;
  return batch_member_ranges(s.nbatch, nblk, [&](int b0, int nb) {
    const dim3 g((unsigned)(nblk * nb)), b(256);
    double* xs = x + (int64_t)b0 * xstride;
    const double* Ws = W + (int64_t)b0 * wstride;
    if (rb == 32)
      hipLaunchKernelGGL((k_bss_gather<32>), g, b, 0, st, s.flag + b0, xs, xstride, ldx, pos, nsel, nv, (unsigned)nblk, Ws, wstride);
    else
      hipLaunchKernelGGL((k_bss_gather<16>), g, b, 0, st, s.flag + b0, xs, xstride, ldx, pos, nsel, nv, (unsigned)nblk, Ws, wstride);
  });
}

int launch_bss_gram(hipStream_t st, const BssView& s, const int* chunks, int nchunk, const double* WI, int64_t wsI, int rbI,
                    const double* WJ, int64_t wsJ, int rbJ, double* part) {
  return batch_member_ranges(s.nbatch, nchunk, [&](int b0, int nb) {
    hipLaunchKernelGGL(k_bss_gram, dim3((unsigned)((int64_t)nchunk * nb)), dim3(256), 0, st, s.flag + b0, chunks,
                       (unsigned)nchunk, WI + (int64_t)b0 * wsI, wsI, rbI, WJ + (int64_t)b0 * wsJ, wsJ, rbJ,
                       part + (int64_t)b0 * nchunk * 1024);
  });
}

int launch_bss_gram_reduce(hipStream_t st, const BssView& s, const double* part, int nchunk, int nvI, int nvJ, bool diag,
                           double* Gij, double* Gji, int64_t gstride, int64_t ldg) {
  return batch_member_ranges(s.nbatch, 1, [&](int b0, int nb) {
    hipLaunchKernelGGL(k_bss_gram_reduce, dim3((unsigned)nb), dim3(256), 0, st, s.flag + b0,
                       part + (int64_t)b0 * nchunk * 1024, nchunk, nvI, nvJ, diag ? 1 : 0, Gij + (int64_t)b0 * gstride,
                       Gji + (int64_t)b0 * gstride, gstride, ldg);
  });
}

}  // namespace spx
