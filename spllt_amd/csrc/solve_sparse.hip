// Sparse right-hand sides and selected outputs on gfx950 (schedule.hpp SolveSparsePlan):
// what a restricted solve needs around the unchanged sweep kernels of solve_many.hip, on the same workspace
// W[p * RB + q] (pivot position p, right-hand side q < RB = 16 or 32).  No atomics in this translation unit.
//
//   k_ss_zero          the touched rows of W (a list of (first pivot position, length) chunks) set to zero
//   k_ss_scatter       the nonzeros of a group of columns of B stored into the zeroed rows
//   k_ss_gather        x[q * ldx + t] = W[pos[t] * RB + q], q < nv, transposed through LDS like k_sm_pack
//   k_ss_gram          per chunk of at most kSsChunkRows touched rows: the 32 x 32 product Y_I^T Y_J of two
//                      workspaces on v_mfma_f64_16x16x4_f64, stored to a scratch block
//   k_ss_gram_reduce   the blocks of one pair of groups added in ascending chunk order, written with the mirror
//
// MFMA operands as in solve_many.hip: lane l supplies A[l&15][l>>4] and B[l>>4][l&15] and receives
// C[(l>>4) + 4 r][l&15] in register r.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.hpp"

namespace spx {

typedef double d2 __attribute__((ext_vector_type(2)));
typedef double d4 __attribute__((ext_vector_type(4)));

// chunk c = rows [chunks[2 c], chunks[2 c] + chunks[2 c + 1]) of W: RB contiguous doubles per row, a multiple of
// 128 bytes from a 256-byte aligned base, cleared with 16-byte stores
template <int RB>
__global__ __launch_bounds__(256) void k_ss_zero(const int* __restrict__ chunks, double* __restrict__ W) {
  const int first = chunks[2 * blockIdx.x], len = chunks[2 * blockIdx.x + 1];
  d2* p = reinterpret_cast<d2*>(W + (int64_t)first * RB);
  const int total = len * (RB / 2);
  for (int i = threadIdx.x; i < total; i += 256) p[i] = d2{0.0, 0.0};
}

// W[pos[i]] = val[i]: the rows of a column are distinct, so no two threads share a destination
__global__ __launch_bounds__(256) void k_ss_scatter(const int64_t* __restrict__ pos, const double* __restrict__ val,
                                                    int64_t count, double* __restrict__ W) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < count) W[pos[i]] = val[i];
}

// 64 wanted entries per workgroup; only rows named by pos are read
template <int RB>
__global__ __launch_bounds__(256) void k_ss_gather(double* __restrict__ x, int64_t ldx, const int* __restrict__ pos,
                                                   int64_t nsel, int nv, const double* __restrict__ W) {
  __shared__ double tile[64][RB + 1];
  const int tid = threadIdx.x;
  const int64_t t0 = (int64_t)blockIdx.x * 64;
  for (int e = tid; e < 64 * RB; e += 256) {
    const int q = e % RB, tt = e / RB;
    if (t0 + tt < nsel) tile[tt][q] = W[(int64_t)pos[t0 + tt] * RB + q];
  }
  __syncthreads();
  for (int e = tid; e < 64 * RB; e += 256) {
    const int tt = e & 63, q = e >> 6;
    if (t0 + tt < nsel && q < nv) x[(int64_t)q * ldx + t0 + tt] = tile[tt][q];
  }
}

// part[chunk][i][j] = sum over the chunk's rows p of WI[p * rbI + i] * WJ[p * rbJ + j], i, j < 32 (tiles of 16
// behind rbI / rbJ stay zero).  Wavefront v takes the MFMA steps v, v + 4, ... of the chunk (4 rows each); the
// four partial products are added in wavefront order through LDS.  The last step of a chunk whose length is no
// multiple of 4 is padded with zeros: a row behind the chunk's end is never read.
__global__ __launch_bounds__(256) void k_ss_gram(const int* __restrict__ chunks, const double* __restrict__ WI, int rbI,
                                                 const double* __restrict__ WJ, int rbJ, double* __restrict__ part) {
  __shared__ double red[4][32][33];
  const int first = chunks[2 * blockIdx.x], len = chunks[2 * blockIdx.x + 1];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int g = lane >> 4, col = lane & 15;
  const int nI = rbI / 16, nJ = rbJ / 16;
  d4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = d4{0.0, 0.0, 0.0, 0.0};
  const int nstep = (len + 3) / 4;
  for (int s = wv; s < nstep; s += 4) {
    const int k = 4 * s + g;
    const bool ok = k < len;
    const int64_t p = first + min(k, len - 1);
    double av[2], bv[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      av[t] = (ok && t < nI) ? WI[p * rbI + 16 * t + col] : 0.0;
      bv[t] = (ok && t < nJ) ? WJ[p * rbJ + 16 * t + col] : 0.0;
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
        if (a < nI && b < nJ) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[a], bv[b], acc[a][b], 0, 0, 0);
  }
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[wv][16 * a + g + 4 * r][16 * b + col] = acc[a][b][r];
  __syncthreads();
  double* out = part + (int64_t)blockIdx.x * 1024;
  for (int e = tid; e < 1024; e += 256) {
    const int i = e >> 5, j = e & 31;
    out[e] = ((red[0][i][j] + red[1][i][j]) + red[2][i][j]) + red[3][i][j];
  }
}

// G_IJ[i][j] (rows of group I, columns of group J, column-major with ldg) = the sum of the nchunk blocks in
// ascending order, and the same number to G_JI[j][i]; diag: I = J, the lower triangle is computed and mirrored
__global__ __launch_bounds__(256) void k_ss_gram_reduce(const double* __restrict__ part, int nchunk, int nvI, int nvJ,
                                                        int diag, double* __restrict__ Gij, double* __restrict__ Gji,
                                                        int64_t ldg) {
  for (int e = threadIdx.x; e < 1024; e += 256) {
    const int i = e >> 5, j = e & 31;
    if (i >= nvI || j >= nvJ || (diag && i < j)) continue;
    double s = 0.0;
    for (int c = 0; c < nchunk; ++c) s += part[(int64_t)c * 1024 + e];
    Gij[(int64_t)j * ldg + i] = s;
    Gji[(int64_t)i * ldg + j] = s;
  }
}

// ---------------------------------------------------------------------------
// launch wrappers
// ---------------------------------------------------------------------------
void launch_ss_zero(hipStream_t st, const int* chunks, int nchunk, int rb, double* W) {
  if (nchunk <= 0) return;
  const dim3 g((unsigned)nchunk), b(256);
  if (rb == 32)
    hipLaunchKernelGGL((k_ss_zero<32>), g, b, 0, st, chunks, W);
  else
    hipLaunchKernelGGL((k_ss_zero<16>), g, b, 0, st, chunks, W);
}

void launch_ss_scatter(hipStream_t st, const int64_t* pos, const double* val, int64_t count, double* W) {
  if (count <= 0) return;
  const dim3 g((unsigned)((count + 255) / 256)), b(256);
  hipLaunchKernelGGL(k_ss_scatter, g, b, 0, st, pos, val, count, W);
}

void launch_ss_gather(hipStream_t st, double* x, int64_t ldx, const int* pos, int64_t nsel, int nv, int rb,
                      const double* W) {
  if (nsel <= 0 || nv <= 0) return;
  const dim3 g((unsigned)((nsel + 63) / 64)), b(256);
  if (rb == 32)
    hipLaunchKernelGGL((k_ss_gather<32>), g, b, 0, st, x, ldx, pos, nsel, nv, W);
  else
    hipLaunchKernelGGL((k_ss_gather<16>), g, b, 0, st, x, ldx, pos, nsel, nv, W);
}

void launch_ss_gram(hipStream_t st, const int* chunks, int nchunk, const double* WI, int rbI, const double* WJ, int rbJ,
                    double* part) {
  if (nchunk <= 0) return;
  hipLaunchKernelGGL(k_ss_gram, dim3((unsigned)nchunk), dim3(256), 0, st, chunks, WI, rbI, WJ, rbJ, part);
}

void launch_ss_gram_reduce(hipStream_t st, const double* part, int nchunk, int nvI, int nvJ, bool diag, double* Gij,
                           double* Gji, int64_t ldg) {
  hipLaunchKernelGGL(k_ss_gram_reduce, dim3(1), dim3(256), 0, st, part, nchunk, nvI, nvJ, diag ? 1 : 0, Gij, Gji, ldg);
}

}  // namespace spx
