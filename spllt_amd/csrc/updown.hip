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
// The device bodies live in ud_body.hpp, shared with batch_updown.hip (the same sweep for the members of a batch).
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
#include "ud_body.hpp"

namespace spx {

namespace {

__global__ __launch_bounds__(256) void k_updown_scatter(const int64_t* __restrict__ pos, const double* __restrict__ val,
                                                        int64_t count, double* __restrict__ Wd, int* __restrict__ flag,
                                                        int reset_flag) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < count) Wd[pos[i]] = val[i];
  if (reset_flag && i == 0) *flag = INT_MAX;
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
  ud_gen_block<NV>(u, L, dinv, Wd, coefg, flag, sgn, ud_lds);
}

// The rows below the diagonal square of one block column: workgroup g takes rows [w + 256 g, w + 256 (g + 1)).
template <int NV>
__global__ __launch_bounds__(256) void k_updown_apply(const SolveUnit u, double* __restrict__ L,
                                                      const int* __restrict__ rlist, double* __restrict__ Wd,
                                                      const double* __restrict__ coefg, double sgn) {
  __shared__ __attribute__((aligned(16))) double tile[kUdApplyTile];
  __shared__ double coef[kUdApplyCoef];
  ud_apply_block<NV>(u, L, rlist, Wd, coefg, sgn, (int)blockIdx.x, tile, coef);
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
    (void)hipFuncSetAttribute((const void*)k_updown_gen<NV>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kUdGenLds);
    attr_dev = dev;
  }
  hipLaunchKernelGGL(k_updown_gen<NV>, dim3(1), dim3(256), kUdGenLds, st, u, L, dinv, Wd, coef, flag, (double)sign);
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
