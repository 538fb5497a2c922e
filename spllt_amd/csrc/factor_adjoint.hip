// Reverse-mode derivative of the sparse Cholesky factor on gfx950: from G = d loss / d L on the pattern of
// L (a second arena with L's layout) to d loss / d (P A P^T)_ij on every stored lower position, a stored
// lower entry standing for both a_ij and a_ji.  The sweep runs the SelinvProgram of the handle (schedule.hpp):
// the same panels, order, tiles, row descriptors, dinv slots and scratch offsets.  Per panel J with rows R:
//
//   SYMM    Y   = S L_RJ,  S = tril(G_RR) + tril(G_RR)^T (diagonal doubled)     k_selinv_symm<true> (selinv.hip)
//   SCALE   W   = (G_RJ - sum of the K slices of Y, in order) inv(L_JJ) -> G_RJ  k_fadj_scale
//           Q_t = W_t^T L_RJ,t of the 64-row tile t, into the scratch
//   DIAG    M   = tril(G_JJ) - tril(sum_t Q_t) (tiles in ascending order)        k_fadj_diag
//           N   = inv(L_JJ)^T sym(tril(L_JJ^T M)) inv(L_JJ),  G_JJ = Phi(N)
//           (Phi: lower triangle, diagonal halved; sym(tril X) = Phi(X) + Phi(X)^T)
//
//   k_fadj_seed   G (+)= alpha sum_q a_q[r_i] b_q[c_j] on every lower arena position
//
// Every 64-wide product runs on v_mfma_f64_16x16x4_f64 with LDS operands (lane l supplies A[l&15][l>>4] and
// B[l>>4][l&15] and receives C[(l>>4) + 4 r][l&15] in register r: the header of kernels.hip).
//
// LDS layout of the 64 x 64 operands.  ds_read_b64 is served per 32-lane half over 32 eight-byte banks:
//   the A operand is read as At[m = l&15][k = l>>4] (one half: 16 rows x 2 consecutive k): a row stride
//     = 2 (mod 32) doubles puts the 32 lanes on the banks 2 m + k, all distinct      -> FA_LDA = 66
//   the B operand is read as Bt[k = l>>4][n = l&15] (one half: 2 rows of 16 consecutive doubles): a row
//     stride = 16 (mod 32) puts the second row on the other 16 banks               -> FA_LDB = 80
// (a stride of 65 makes either read a 2-way conflict).  A product whose left operand is a transpose stores
// that transpose into At, so that every read has one of these two forms.  73 KiB per workgroup: two
// workgroups per CU, as many as the K-slice sums and the tile partials keep busy.
//
// No atomics, no loop bound or branch that depends on data, every sum in a fixed order: two sweeps over the
// same L and G bits give the same bits.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fa_body.hpp"
#include "kernels.hpp"

namespace spx {

// the bodies of the three kernels and the two product helpers: fa_body.hpp, shared with the per-member kernels of
// batch_adjoint.hip
__global__ __launch_bounds__(256) void k_fadj_seed(const UpdTile* __restrict__ tiles, const FadjCol* __restrict__ cols,
                                                   const int* __restrict__ rlist, const int* __restrict__ porder,
                                                   double* __restrict__ G, int nvec, const double* __restrict__ a,
                                                   const double* __restrict__ b, int64_t ld, double alpha,
                                                   int accumulate, int a_pivot, int b_pivot) {
  __shared__ double As[FA_NV][FA_T];
  __shared__ int Ra[FA_T];
  const UpdTile tl = tiles[blockIdx.x];
  fa_seed_body(tl, cols[tl.unit], rlist, porder, G, nvec, a, b, ld, alpha, accumulate, a_pivot, b_pivot, As, Ra);
}

__global__ __launch_bounds__(256) void k_fadj_scale(const UpdTile* __restrict__ tiles, const SelinvUnit* __restrict__ units,
                                                    const double* __restrict__ L, const double* __restrict__ dinv,
                                                    double* __restrict__ G, double* __restrict__ scratch) {
  __shared__ double At[FA_T][FA_LDA];   // T, then W^T
  __shared__ double Bt[FA_T][FA_LDB];   // inv(L_JJ), then the tile's rows of L_RJ
  const UpdTile t = tiles[blockIdx.x];
  fa_scale_body(t, units[t.unit], L, dinv, G, scratch, At, Bt);
}

__global__ __launch_bounds__(1024) void k_fadj_diag(const SelinvUnit* __restrict__ units, const double* __restrict__ L,
                                                    const double* __restrict__ dinv, double* __restrict__ G,
                                                    const double* __restrict__ scratch) {
  __shared__ double At[FA_T][FA_LDA];
  __shared__ double Bt[FA_T][FA_LDB];
  fa_diag_body(units[blockIdx.x], L, dinv, G, scratch, At, Bt);
}

void launch_fadj_seed(hipStream_t st, const UpdTile* tiles, int64_t ntiles, const FadjCol* cols, const int* rlist,
                      const int* porder, double* G, int nvec, const double* a, const double* b, int64_t ld, double alpha,
                      bool accumulate, int order_flags) {
  if (ntiles <= 0) return;
  hipLaunchKernelGGL(k_fadj_seed, dim3((unsigned)ntiles), dim3(256), 0, st, tiles, cols, rlist, porder, G, nvec, a, b, ld,
                     alpha, accumulate ? 1 : 0, order_flags & 1, (order_flags >> 1) & 1);
}

void launch_fadj(hipStream_t st, const SelinvLaunch& l, const SelinvUnit* units, const UpdTile* tiles,
                 const SelinvRow* rows, const int* relpos, const double* L, const double* dinv, double* G,
                 double* scratch) {
  if (l.count <= 0) return;
  const dim3 grid((unsigned)l.count);
  if (l.kind == SI_SYMM)
    launch_selinv_symm_doubled(st, l, units, tiles, rows, relpos, L, G, scratch);
  else if (l.kind == SI_SCALE)
    hipLaunchKernelGGL(k_fadj_scale, grid, dim3(256), 0, st, tiles + l.first, units, L, dinv, G, scratch);
  else
    hipLaunchKernelGGL(k_fadj_diag, grid, dim3(1024), 0, st, units + l.first, L, dinv, G, (const double*)scratch);
}

}  // namespace spx
