// Reverse-mode derivative of the factors of a batch on gfx950: for every member b of a batch (batch.hip) from
// G_b = d loss / d L_b on the pattern of L (an arena with L's layout, G + b lstride) to d loss / d (P A_b P^T)
// on every stored lower position.  The sweep runs the batch's SelinvProgram (built with pw = cb = 64: the
// panels and dinv slots of the batch factorization, shared with batch_selinv.hip); every launch carries all
// members: the grid is (work items) x (members), member b works on L + b lstride, dinv + b dstride,
// G + b lstride and scratch + b sstride, every table is read shared.  Every workgroup reads its member's
// not-positive-definite flag first and returns, before any barrier, when it is set: nothing of a failed member
// is read or written.
//
//   k_bfa_seed    k_fadj_seed for member b: vector q of member b at a[(b nvec + q) ld ..+ n)
//   SYMM          k_batch_selinv_symm<true> (batch_selinv.hip) with the adjoint arena in the place of Z
//   k_bfa_scale   k_fadj_scale for member b
//   k_bfa_diag    k_fadj_diag for member b
//   k_bfa_fused   a whole step (SYMM + SCALE + DIAG) of one unit with nR <= 64 and one K slice in one
//                 workgroup: six 64 x 64 products, no scratch traffic
//
// The bodies of seed, scale and diag are those of the single handle (fa_body.hpp): per member the same sums in
// the same order; the SYMM body and the gather of the fused kernel's first product are those of the selected
// inversion (si_body.hpp: si_symm_body<true>, si_small_gather_body<true, ..>).  Every product runs on v_mfma_f64_16x16x4_f64 with LDS operands in the layout of
// factor_adjoint.hip (FA_LDA = 66 for the A operand, FA_LDB = 80 for the B operand: its header has the bank
// argument).  No atomics, no waiting between workgroups, no loop bound or branch that depends on data: two
// sweeps over the same L_b and G_b bits give the same bits, whatever the other members hold.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "batch_split.hpp"
#include "fa_body.hpp"
#include "kernels.hpp"
#include "si_body.hpp"

namespace spx {

// s.Z is the adjoint arena G in this translation unit
__global__ __launch_bounds__(256) void k_bfa_seed(BatchSelinvView s, const UpdTile* __restrict__ tiles, int64_t count,
                                                  const FadjCol* __restrict__ cols, const int* __restrict__ rlist,
                                                  const int* __restrict__ porder, int nvec, const double* __restrict__ a,
                                                  const double* __restrict__ b, int64_t ld, double alpha, int accumulate,
                                                  int a_pivot, int b_pivot) {
  __shared__ double As[FA_NV][FA_T];
  __shared__ int Ra[FA_T];
  int m;
  int64_t wi;
  bsi_split(s.v, count, m, wi);
  if (s.v.flag[m] != INT_MAX) return;
  const UpdTile tl = tiles[wi];
  const int64_t voff = (int64_t)m * nvec * ld;
  fa_seed_body(tl, cols[tl.unit], rlist, porder, s.Z + (int64_t)m * s.v.lstride, nvec, a + voff, b + voff, ld, alpha,
               accumulate, a_pivot, b_pivot, As, Ra);
}

__global__ __launch_bounds__(256) void k_bfa_scale(BatchSelinvView s, const UpdTile* __restrict__ tiles, int64_t count,
                                                   const SelinvUnit* __restrict__ units) {
  __shared__ double At[FA_T][FA_LDA];
  __shared__ double Bt[FA_T][FA_LDB];
  int b;
  int64_t wi;
  bsi_split(s.v, count, b, wi);
  if (s.v.flag[b] != INT_MAX) return;
  const UpdTile t = tiles[wi];
  fa_scale_body(t, units[t.unit], s.v.L + (int64_t)b * s.v.lstride, s.v.dinv + (int64_t)b * s.v.dstride,
                s.Z + (int64_t)b * s.v.lstride, s.scratch + (int64_t)b * s.sstride, At, Bt);
}

__global__ __launch_bounds__(1024) void k_bfa_diag(BatchSelinvView s, const SelinvUnit* __restrict__ units, int64_t count) {
  __shared__ double At[FA_T][FA_LDA];
  __shared__ double Bt[FA_T][FA_LDB];
  int b;
  int64_t wi;
  bsi_split(s.v, count, b, wi);
  if (s.v.flag[b] != INT_MAX) return;
  fa_diag_body(units[wi], s.v.L + (int64_t)b * s.v.lstride, s.v.dinv + (int64_t)b * s.v.dstride,
               s.Z + (int64_t)b * s.v.lstride, s.scratch + (int64_t)b * s.sstride, At, Bt);
}

// ---------------------------------------------------------------------------
// One whole adjoint step of one unit (nR <= 64, one K slice) per workgroup and member, 4 wavefronts;
// wavefront w owns rows 16 w .. 16 w + 15 of every product and all (<= 4) 16-column blocks.  At carries the
// left operand (read as At[m][k]), Bt the right one (read as Bt[k][n]); a left operand that is a transpose
// is stored transposed.
//   1  At = S (gathered: tril(G_RR) mirrored, diagonal doubled)   Bt = L_RJ        Y = At Bt
//   2  At = G_RJ - Y                                              Bt = inv(L_JJ)   W = At Bt      -> G_RJ
//   3  At = W^T                                                   Bt = L_RJ        Q = At Bt
//   4  At = L_JJ^T                                                Bt = tril(G_JJ) - tril(Q)       X = At Bt
//   5  At = sym(tril X)                                           Bt = inv(L_JJ)   V = At Bt
//   6  At = inv(L_JJ)^T                                           Bt = V           N = At Bt
//      G_JJ = Phi(N): lower triangle stored, diagonal halved
// L_RJ, L_JJ and the dinv slot are read from memory once, into registers in the tile layout (element
// (t >> 6) + 4 q, t & 63 of thread t); L_JJ, G_JJ and the dinv slot are masked to their lower triangles.
// Both buffers are written in full (zero outside the unit's rows and columns) before every product: the K
// loops run to a multiple of 4 and must not meet stale LDS.  nR = 0 (a root's last panel): products 1 - 3
// are skipped, Q = 0.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void bfa_zero(d4 (&acc)[4]) {
#pragma unroll
  for (int c = 0; c < 4; ++c) acc[c] = d4{0.0, 0.0, 0.0, 0.0};
}

__global__ __launch_bounds__(256) void k_bfa_fused(BatchSelinvView s, const SelinvUnit* __restrict__ units, int64_t count,
                                                   const SelinvRow* __restrict__ rows, const int* __restrict__ relpos) {
  __shared__ double At[FA_T][FA_LDA];
  __shared__ double Bt[FA_T][FA_LDB];
  __shared__ SelinvRow Ri[FA_T];
  int b;
  int64_t wi;
  bsi_split(s.v, count, b, wi);
  if (s.v.flag[b] != INT_MAX) return;
  const SelinvUnit u = units[wi];
  const double* __restrict__ L = s.v.L + (int64_t)b * s.v.lstride;
  const double* __restrict__ D = s.v.dinv + (int64_t)b * s.v.dstride + u.dinv_off;
  double* __restrict__ G = s.Z + (int64_t)b * s.v.lstride;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int g = lane >> 4, col = lane & 15;
  const int tj = tid & 63, ti0 = tid >> 6;        // tile layout: element (ti0 + 4 q, tj)
  const int nR = u.nR, pn = u.pn;
  const int ncb = (pn + 15) >> 4, ksp = (pn + 3) >> 2;
  const double* Ljj = L + u.off + (int64_t)u.c0 * u.ld + u.c0;
  double* Gjj = G + u.off + (int64_t)u.c0 * u.ld + u.c0;
  double dreg[16], jreg[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int i = ti0 + 4 * q;
    const bool low = i < pn && tj <= i;
    dreg[q] = low ? D[(int64_t)i * u.dinv_ld + tj] : 0.0;
    jreg[q] = low ? Ljj[(int64_t)i * u.ld + tj] : 0.0;
  }
  d4 acc[4];
  bfa_zero(acc);
  if (nR > 0) {   // (the same for every thread of the workgroup)
    double* Grj = G + u.off + (int64_t)(u.c0 + pn) * u.ld + u.c0;
    double lreg[16];
    // 1: S (tril(G_RR) mirrored, the diagonal doubled) and L_RJ
    si_small_gather_body<true, FA_LDA, FA_LDB>(u, rows, relpos, L, G, At, Bt, Ri, lreg);
    __syncthreads();
    fadj_mm4(At, 16 * wv, Bt, (nR + 3) >> 2, ncb, lane, acc);   // Y = S L_RJ
    __syncthreads();
    // 2: T = G_RJ - Y in the accumulator layout (zero beyond nR x pn: Y is, its operands were), inv(L_JJ)
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * wv + g + 4 * r, cc = 16 * c + col;
        const double gv = (row < nR && cc < pn) ? Grj[(int64_t)row * u.ld + cc] : 0.0;
        At[row][cc] = gv - acc[c][r];
      }
#pragma unroll
    for (int q = 0; q < 16; ++q) Bt[ti0 + 4 * q][tj] = dreg[q];
    __syncthreads();
    bfa_zero(acc);
    fadj_mm4(At, 16 * wv, Bt, ksp, ncb, lane, acc);             // W = T inv(L_JJ)
    __syncthreads();
    // 3: W -> G_RJ, W^T, L_RJ again
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * wv + g + 4 * r, cc = 16 * c + col;
        const double w = acc[c][r];
        if (row < nR && cc < pn) Grj[(int64_t)row * u.ld + cc] = w;
        At[cc][row] = w;
      }
#pragma unroll
    for (int q = 0; q < 16; ++q) Bt[ti0 + 4 * q][tj] = lreg[q];
    __syncthreads();
    bfa_zero(acc);
    fadj_mm4(At, 16 * wv, Bt, (nR + 3) >> 2, ncb, lane, acc);   // Q = W^T L_RJ
    __syncthreads();
  }
  // 4: M = tril(G_JJ) - tril(Q) in the accumulator layout, L_JJ^T from the tile layout
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * wv + g + 4 * r, cc = 16 * c + col;
      Bt[row][cc] = (row < pn && cc <= row) ? Gjj[(int64_t)row * u.ld + cc] - acc[c][r] : 0.0;
    }
#pragma unroll
  for (int q = 0; q < 16; ++q) At[tj][ti0 + 4 * q] = jreg[q];
  __syncthreads();
  bfa_zero(acc);
  fadj_mm4(At, 16 * wv, Bt, ksp, ncb, lane, acc);               // X = L_JJ^T M
  __syncthreads();
  // 5: sym(tril X) = Phi(X) + Phi(X)^T (every entry of the 64 x 64 square is written by one of the two
  // stores: X is zero past pn), inv(L_JJ)
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * wv + g + 4 * r, cc = 16 * c + col;
      if (row >= cc) {
        At[row][cc] = acc[c][r];
        At[cc][row] = acc[c][r];
      }
    }
#pragma unroll
  for (int q = 0; q < 16; ++q) Bt[ti0 + 4 * q][tj] = dreg[q];
  __syncthreads();
  bfa_zero(acc);
  fadj_mm4(At, 16 * wv, Bt, ksp, ncb, lane, acc);               // V = sym(tril X) inv(L_JJ)
  __syncthreads();
  // 6: V, inv(L_JJ)^T
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int r = 0; r < 4; ++r) Bt[16 * wv + g + 4 * r][16 * c + col] = acc[c][r];
#pragma unroll
  for (int q = 0; q < 16; ++q) At[tj][ti0 + 4 * q] = dreg[q];
  __syncthreads();
  bfa_zero(acc);
  fadj_mm4(At, 16 * wv, Bt, ksp, ncb, lane, acc);               // N = inv(L_JJ)^T V
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * wv + g + 4 * r, cc = 16 * c + col;
      if (row < pn && cc <= row) Gjj[(int64_t)row * u.ld + cc] = row == cc ? 0.5 * acc[c][r] : acc[c][r];
    }
}

// ---------------------------------------------------------------------------
// launch wrappers: the conventions of batch_selinv.hip (the number of kernel launches made; -1, nothing
// launched, when ONE member's work items overflow a grid)
// ---------------------------------------------------------------------------
int launch_batch_fadj_seed(hipStream_t st, const BatchSelinvView& s, const UpdTile* tiles, int64_t ntiles,
                           const FadjCol* cols, const int* rlist, const int* porder, int nvec, const double* a,
                           const double* b, int64_t ld, double alpha, bool accumulate, int order_flags) {
  return bsi_member_ranges(s, ntiles, [&](const BatchSelinvView& r, int b0) {
    const int64_t voff = (int64_t)b0 * nvec * ld;
    hipLaunchKernelGGL(k_bfa_seed, dim3((unsigned)(ntiles * r.v.nbatch)), dim3(256), 0, st, r, tiles, ntiles, cols, rlist,
                       porder, nvec, a + voff, b + voff, ld, alpha, accumulate ? 1 : 0, order_flags & 1,
                       (order_flags >> 1) & 1);
  });
}

int launch_batch_fadj(hipStream_t st, const BatchSelinvView& s, const SelinvLaunch& l, const SelinvUnit* units,
                      const UpdTile* tiles, const SelinvRow* rows, const int* relpos) {
  if (l.kind == SI_SYMM) return launch_batch_selinv_symm_doubled(st, s, l, units, tiles, rows, relpos);
  return bsi_member_ranges(s, l.count, [&](const BatchSelinvView& r, int) {
    const dim3 grid((unsigned)(l.count * r.v.nbatch));
    if (l.kind == SI_SCALE)
      hipLaunchKernelGGL(k_bfa_scale, grid, dim3(256), 0, st, r, tiles + l.first, l.count, units);
    else
      hipLaunchKernelGGL(k_bfa_diag, grid, dim3(1024), 0, st, r, units + l.first, l.count);
  });
}

int launch_batch_fadj_fused(hipStream_t st, const BatchSelinvView& s, const SelinvUnit* units, int64_t count,
                            const SelinvRow* rows, const int* relpos) {
  return bsi_member_ranges(s, count, [&](const BatchSelinvView& r, int) {
    hipLaunchKernelGGL(k_bfa_fused, dim3((unsigned)(count * r.v.nbatch)), dim3(256), 0, st, r, units, count, rows, relpos);
  });
}

}  // namespace spx
