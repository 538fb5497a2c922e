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
// The device bodies are in ss_body.hpp, shared with the kernels for the members of a batch (batch_solve_sparse.hip).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.hpp"
#include "ss_body.hpp"

namespace spx {

// chunk c = rows [chunks[2 c], chunks[2 c] + chunks[2 c + 1]) of W
template <int RB>
__global__ __launch_bounds__(256) void k_ss_zero(const int* __restrict__ chunks, double* __restrict__ W) {
  ss_zero_body<RB>(chunks[2 * blockIdx.x], chunks[2 * blockIdx.x + 1], W);
}

// W[pos[i]] = val[i]: the rows of a column are distinct, so no two threads share a destination
__global__ __launch_bounds__(256) void k_ss_scatter(const int64_t* __restrict__ pos, const double* __restrict__ val,
                                                    int64_t count, double* __restrict__ W) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < count) W[pos[i]] = val[i];
}

template <int RB>
__global__ __launch_bounds__(256) void k_ss_gather(double* __restrict__ x, int64_t ldx, const int* __restrict__ pos,
                                                   int64_t nsel, int nv, const double* __restrict__ W) {
  __shared__ double tile[64][RB + 1];
  ss_gather_body<RB>((int64_t)blockIdx.x * 64, x, ldx, pos, nsel, nv, W, tile);
}

// part[chunk][i][j] = the product of the chunk's rows of the two workspaces (ss_gram_body)
__global__ __launch_bounds__(256) void k_ss_gram(const int* __restrict__ chunks, const double* __restrict__ WI, int rbI,
                                                 const double* __restrict__ WJ, int rbJ, double* __restrict__ part) {
  __shared__ double red[4][32][33];
  ss_gram_body(chunks[2 * blockIdx.x], chunks[2 * blockIdx.x + 1], WI, rbI, WJ, rbJ,
               part + (int64_t)blockIdx.x * 1024, red);
}

__global__ __launch_bounds__(256) void k_ss_gram_reduce(const double* __restrict__ part, int nchunk, int nvI, int nvJ,
                                                        int diag, double* __restrict__ Gij, double* __restrict__ Gji,
                                                        int64_t ldg) {
  ss_gram_reduce_body(part, nchunk, nvI, nvJ, diag, Gij, Gji, ldg);
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
