// Sampled symmetric outer product on the analysed pattern (gfx950): for the k-th entry of the CSC-lower
// pattern, at row i >= column j in user variables,
//
//     out[k] = alpha * sum_q ( u_q[i] v_q[j] + [i != j] u_q[j] v_q[i] ),   q = 0 .. nvec - 1
//
// -- what the gradient of x = A^-1 b with respect to the stored values needs (u = the adjoint solution,
// v = x, alpha = -1; val_k stands for a_ij and a_ji).
//
//   k_pattern_outer   one lane per entry, lanes over consecutive entries: these share a column in runs, so
//                     u_q[j], v_q[j] are same-address (broadcast) reads and u_q[i], v_q[i] near-contiguous
//                     gathers.  The (row, column) pair is read once; the vectors are taken PO_NV at a time,
//                     their 4 PO_NV loads issued together.  Gather only: no atomics, no LDS.
// The sum over q is ONE chain of fma per entry in ascending q (first u_i v_j, then u_j v_i), alpha is applied
// once at the end: the chain does not depend on PO_NV, on the grid or on how the members of a batch are
// split into launches, so the same input bits give the same output bits.
// The work is 2 index loads and 4 nvec gathered doubles per entry against 4 nvec flops: gather-bound, nothing
// for the matrix cores.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "kernels.hpp"

namespace spx {

constexpr int PO_NV = 4;   // vectors per pass of the q loop

// member b of the launch: vectors at u + (b nvec + q) ldu, output at out + b ldout
__global__ __launch_bounds__(256) void k_pattern_outer(const int* __restrict__ prow, const int* __restrict__ pcol,
                                                       int64_t nnz, int64_t nblk, int nvec,
                                                       const double* __restrict__ u, int64_t ldu,
                                                       const double* __restrict__ v, int64_t ldv, double alpha,
                                                       double* __restrict__ out, int64_t ldout) {
  const int64_t b = (int64_t)blockIdx.x / nblk;
  const int64_t k = ((int64_t)blockIdx.x - b * nblk) * 256 + threadIdx.x;
  if (k >= nnz) return;
  const int i = prow[k], j = pcol[k];
  const bool off = i != j;
  const double* ub = u + b * nvec * ldu;
  const double* vb = v + b * nvec * ldv;
  double acc = 0.0;
  int q = 0;
  for (; q + PO_NV <= nvec; q += PO_NV) {
    double ui[PO_NV], uj[PO_NV], vi[PO_NV], vj[PO_NV];
#pragma unroll
    for (int t = 0; t < PO_NV; ++t) {
      const double* uq = ub + (int64_t)(q + t) * ldu;
      const double* vq = vb + (int64_t)(q + t) * ldv;
      ui[t] = uq[i]; vj[t] = vq[j];
      uj[t] = uq[j]; vi[t] = vq[i];
    }
#pragma unroll
    for (int t = 0; t < PO_NV; ++t) {
      acc = fma(ui[t], vj[t], acc);
      if (off) acc = fma(uj[t], vi[t], acc);
    }
  }
  for (; q < nvec; ++q) {
    const double* uq = ub + (int64_t)q * ldu;
    const double* vq = vb + (int64_t)q * ldv;
    const double ui = uq[i], vj = vq[j], uj = uq[j], vi = vq[i];
    acc = fma(ui, vj, acc);
    if (off) acc = fma(uj, vi, acc);
  }
  out[b * ldout + k] = alpha * acc;
}

// All members in one launch as long as (workgroups of one member) x (members) fits a grid (the limit of
// batch.hip, test hook included); beyond that the members are split into ranges.  Returns the number of
// kernel launches (-1, nothing launched: ONE member's entries overflow a grid).
int launch_pattern_outer(hipStream_t st, const int* prow, const int* pcol, int64_t nnz, int nbatch, int nvec,
                         const double* u, int64_t ldu, const double* v, int64_t ldv, double alpha, double* out,
                         int64_t ldout) {
  if (nnz <= 0 || nbatch <= 0) return 0;
  const int64_t nblk = (nnz + 255) / 256;
  if (nblk > batch_grid_limit_max()) return -1;
  const int step = (int)std::max<int64_t>(1, std::min<int64_t>(nbatch, batch_grid_limit() / nblk));
  int launches = 0;
  for (int b0 = 0; b0 < nbatch; b0 += step) {
    const int nb = std::min(step, nbatch - b0);
    hipLaunchKernelGGL(k_pattern_outer, dim3((unsigned)(nblk * nb)), dim3(256), 0, st, prow, pcol, nnz, nblk, nvec,
                       u + (int64_t)b0 * nvec * ldu, ldu, v + (int64_t)b0 * nvec * ldv, ldv, alpha,
                       out + (int64_t)b0 * ldout, ldout);
    ++launches;
  }
  return launches;
}

}  // namespace spx
