// Batched selected inversion on gfx950: Z_b = (P A_b P^T)^-1 on the pattern of L for the nbatch members of
// a batch (batch.hip), by ONE SelinvProgram of the pattern (schedule.hpp, built with pw = cb = 64: the
// panels and dinv slots of the batch factorization).  Every launch carries all members: the grid is
// (work items) x (members), member b works on L + b lstride, dinv + b dstride, Z + b lstride and
// scratch + b sstride, and every table is read shared.  A member whose not-positive-definite flag is set
// is skipped by every workgroup: nothing of it is read or written.
//
//   k_batch_selinv_symm / _scale / _diag   the three step kernels: si_symm_body, si_scale_body and si_diag_body
//                         of si_body.hpp (its header describes the steps) on the arenas of member b
//   k_batch_selinv_fused  a whole step (SYMM + SCALE + DIAG) of one unit with nR <= 64 and one K slice in
//                         one workgroup: Z_RR gathered into LDS (si_small_gather_body), the four products on
//                         v_mfma_f64_16x16x4_f64, no scratch traffic
//   k_batch_selinv_diag_gather   (A_b^-1)_ii in the user's variable order, NaN for a failed member
//   k_batch_selinv_pattern       (A_b^-1) at the entries of the caller's CSC-lower pattern, in the order of
//                                val (the value map of the analysis read backwards), NaN for a failed member
//
// No kernel uses atomics and every sum runs in a fixed order: two inversions of one batch give a
// bit-identical Z for every member.  Nothing is read or written outside the rows and columns a table
// entry names, so a member never touches its neighbour's arena.
//
// MFMA lane map (header of si_body.hpp): lane l supplies A[l&15][l>>4] and B[l>>4][l&15] and receives
// C[(l>>4) + 4 r][l&15] in register r.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>

#include "batch_split.hpp"
#include "kernels.hpp"
#include "si_body.hpp"

namespace spx {

constexpr int BI_LD = SI_T + 1;     // LDS row stride of the fused kernel's two operand buffers

// ---------------------------------------------------------------------------
// The step kernels: workgroup -> (member b, work item), the member's flag before any barrier, the member's
// arenas, the body.  kDoubleDiag = true is the SYMM step of the factor adjoint (batch_adjoint.hip: s.Z is then
// the adjoint arena).
// ---------------------------------------------------------------------------
template <bool kDoubleDiag>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_batch_selinv_symm(BatchSelinvView s, const UpdTile* __restrict__ tiles, int64_t count,
                                                           const SelinvUnit* __restrict__ units,
                                                           const SelinvRow* __restrict__ rows,
                                                           const int* __restrict__ relpos) {
  __shared__ double As[SI_T][SI_KC + 1];
  __shared__ double Bs[SI_KC][SI_T + 1];
  __shared__ SelinvRow Ri[SI_T];
  int b;
  int64_t wi;
  bsi_split(s.v, count, b, wi);
  if (s.v.flag[b] != INT_MAX) return;
  const UpdTile t = tiles[wi];
  si_symm_body<kDoubleDiag>(t, units[t.unit], rows, relpos, s.v.L + (int64_t)b * s.v.lstride,
                            s.Z + (int64_t)b * s.v.lstride, s.scratch + (int64_t)b * s.sstride, As, Bs, Ri);
}

__global__ __launch_bounds__(256) void k_batch_selinv_scale(BatchSelinvView s, const UpdTile* __restrict__ tiles, int64_t count,
                                                            const SelinvUnit* __restrict__ units) {
  __shared__ double Ys[SI_T][SI_T + 1];
  __shared__ double Ms[SI_T][SI_T + 1];
  int b;
  int64_t wi;
  bsi_split(s.v, count, b, wi);
  if (s.v.flag[b] != INT_MAX) return;
  const UpdTile t = tiles[wi];
  si_scale_body(t, units[t.unit], s.v.L + (int64_t)b * s.v.lstride, s.v.dinv + (int64_t)b * s.v.dstride,
                s.Z + (int64_t)b * s.v.lstride, s.scratch + (int64_t)b * s.sstride, Ys, Ms);
}

__global__ __launch_bounds__(1024) void k_batch_selinv_diag(BatchSelinvView s, const SelinvUnit* __restrict__ units, int64_t count) {
  __shared__ double Ds[SI_T][SI_T + 1];
  __shared__ double Ts[SI_T][SI_T + 1];
  int b;
  int64_t wi;
  bsi_split(s.v, count, b, wi);
  if (s.v.flag[b] != INT_MAX) return;
  si_diag_body(units[wi], s.v.dinv + (int64_t)b * s.v.dstride, s.Z + (int64_t)b * s.v.lstride,
               s.scratch + (int64_t)b * s.sstride, Ds, Ts);
}

// ---------------------------------------------------------------------------
// One whole step of one unit (nR <= 64, one K slice) per workgroup and member.  Two 64 x 64 LDS buffers
// (A, B) carry the operands of four products in turn; wavefront w owns rows 16 w .. 16 w + 15 of every
// product and all (<= 4) 16-column blocks.  What the next product needs from memory (inv(L_JJ), L_RJ) is
// loaded into registers before the current one starts.
//   1  A = Z_RR (gathered, symmetric), B = L_RJ          Y    = A B
//   2  A = Y,                          B = inv(L_JJ)     Z_RJ = -(A B)            -> Z arena
//   3  A = Z_RJ,                       B = L_RJ          P    = B^T A
//   4  A = inv(L_JJ) - P,              B = inv(L_JJ)     Z_JJ = B^T A (lower)     -> Z arena
// Both buffers are written in full (zero outside the unit's rows and columns) before every product: the K
// loops run to a multiple of 4 and must not meet stale LDS.  nR = 0: products 1 - 3 are skipped, P = 0.
// ---------------------------------------------------------------------------
template <bool TA>
__device__ __forceinline__ void bsi_mm(const double (*A)[BI_LD], const double (*B)[BI_LD], int K, int ncb, int wv, int g,
                                       int col, d4 (&acc)[4]) {
#pragma unroll
  for (int c = 0; c < 4; ++c) acc[c] = d4{0.0, 0.0, 0.0, 0.0};
  const int ks = (K + 3) >> 2;
  for (int st = 0; st < ks; ++st) {
    const double a = TA ? A[4 * st + g][16 * wv + col] : A[16 * wv + col][4 * st + g];
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < ncb) acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, B[4 * st + g][16 * c + col], acc[c], 0, 0, 0);
  }
}

__global__ __launch_bounds__(256) void k_batch_selinv_fused(BatchSelinvView s, const SelinvUnit* __restrict__ units, int64_t count,
                                                            const SelinvRow* __restrict__ rows,
                                                            const int* __restrict__ relpos) {
  __shared__ double Ab[SI_T][BI_LD];
  __shared__ double Bb[SI_T][BI_LD];
  __shared__ SelinvRow Ri[SI_T];
  int b;
  int64_t wi;
  bsi_split(s.v, count, b, wi);
  if (s.v.flag[b] != INT_MAX) return;
  const SelinvUnit u = units[wi];
  const double* __restrict__ L = s.v.L + (int64_t)b * s.v.lstride;
  const double* __restrict__ D = s.v.dinv + (int64_t)b * s.v.dstride + u.dinv_off;
  double* __restrict__ Z = s.Z + (int64_t)b * s.v.lstride;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int g = lane >> 4, col = lane & 15;
  const int tj = tid & 63, ti0 = tid >> 6;        // tile loads: element (ti0 + 4 q, tj)
  const int nR = u.nR, pn = u.pn;
  const int ncb = (pn + 15) >> 4;
  // inv(L_JJ): in the tile-load layout (for B) and in the accumulator layout (for inv(L_JJ) - P)
  double dreg[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int i = ti0 + 4 * q;
    dreg[q] = (i < pn && tj <= i) ? D[(int64_t)i * u.dinv_ld + tj] : 0.0;
  }
  d4 acc[4];
  if (nR > 0) {   // (the same for every thread of the workgroup)
    double lreg[16];
    // 1: Z_RR (symmetric) and L_RJ
    si_small_gather_body<false, BI_LD, BI_LD>(u, rows, relpos, L, Z, Ab, Bb, Ri, lreg);
    __syncthreads();
    bsi_mm<false>(Ab, Bb, nR, ncb, wv, g, col, acc);
    __syncthreads();
    // 2: Y (zero beyond the unit's rows and columns: the operands were) and inv(L_JJ)
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) Ab[16 * wv + g + 4 * r][16 * c + col] = c < ncb ? acc[c][r] : 0.0;
#pragma unroll
    for (int q = 0; q < 16; ++q) Bb[ti0 + 4 * q][tj] = dreg[q];
    __syncthreads();
    bsi_mm<false>(Ab, Bb, pn, ncb, wv, g, col, acc);
    double* Zrj = Z + u.off + (int64_t)(u.c0 + pn) * u.ld + u.c0;
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * wv + g + 4 * r, cc = 16 * c + col;
        acc[c][r] = -acc[c][r];
        if (c < ncb && row < nR && cc < pn) Zrj[(int64_t)row * u.ld + cc] = acc[c][r];
      }
    __syncthreads();
    // 3: Z_RJ and L_RJ again
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) Ab[16 * wv + g + 4 * r][16 * c + col] = c < ncb ? acc[c][r] : 0.0;
#pragma unroll
    for (int q = 0; q < 16; ++q) Bb[ti0 + 4 * q][tj] = lreg[q];
    __syncthreads();
    bsi_mm<true>(Bb, Ab, nR, ncb, wv, g, col, acc);
    __syncthreads();
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = d4{0.0, 0.0, 0.0, 0.0};
  }
  // 4: T = inv(L_JJ) - P in the accumulator layout, inv(L_JJ) in the tile layout
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * wv + g + 4 * r, cc = 16 * c + col;
      const double d = (c < ncb && row < pn && cc <= row) ? D[(int64_t)row * u.dinv_ld + cc] : 0.0;
      Ab[row][cc] = c < ncb ? d - acc[c][r] : 0.0;
    }
#pragma unroll
  for (int q = 0; q < 16; ++q) Bb[ti0 + 4 * q][tj] = dreg[q];
  __syncthreads();
  bsi_mm<true>(Bb, Ab, pn, ncb, wv, g, col, acc);
  double* Zjj = Z + u.off + (int64_t)u.c0 * u.ld + u.c0;
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * wv + g + 4 * r, cc = 16 * c + col;
      if (c < ncb && row < pn && cc <= row) Zjj[(int64_t)row * u.ld + cc] = acc[c][r];
    }
}

// ---------------------------------------------------------------------------
// readers.  flag == nullptr: one arena that is known to be valid (the single-handle inverse)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_batch_selinv_diag_gather(BatchSelinvView s, const int64_t* __restrict__ diag_pos,
                                                                  const int* __restrict__ order, int n, int64_t nblk,
                                                                  double* __restrict__ out, int64_t ldout) {
  int b;
  int64_t blk;
  bsi_split(s.v, nblk, b, blk);
  const int64_t i = blk * 256 + threadIdx.x;
  if (i >= n) return;
  const bool ok = !s.v.flag || s.v.flag[b] == INT_MAX;
  out[(int64_t)b * ldout + i] = ok ? s.Z[(int64_t)b * s.v.lstride + diag_pos[order[i]]] : NAN;
}

__global__ __launch_bounds__(256) void k_batch_selinv_pattern(BatchSelinvView s, const int64_t* __restrict__ map_dst,
                                                              const int64_t* __restrict__ map_src, int64_t nmap, int64_t nblk,
                                                              double* __restrict__ out, int64_t ldout) {
  int b;
  int64_t blk;
  bsi_split(s.v, nblk, b, blk);
  const int64_t e = blk * 256 + threadIdx.x;
  if (e >= nmap) return;
  const bool ok = !s.v.flag || s.v.flag[b] == INT_MAX;
  out[(int64_t)b * ldout + map_src[e]] = ok ? s.Z[(int64_t)b * s.v.lstride + map_dst[e]] : NAN;
}

// ---------------------------------------------------------------------------
// launch wrappers: one kernel launch per call as long as (work items) x (members) fits a grid (the limit
// of batch.hip, test hook included); beyond that the members are split into ranges.  Every wrapper returns
// the number of kernel launches it made (-1, nothing launched: ONE member's work items overflow a grid).
// ---------------------------------------------------------------------------

int launch_batch_selinv(hipStream_t st, const BatchSelinvView& s, const SelinvLaunch& l, const SelinvUnit* units,
                        const UpdTile* tiles, const SelinvRow* rows, const int* relpos) {
  return bsi_member_ranges(s, l.count, [&](const BatchSelinvView& r, int) {
    const dim3 grid((unsigned)(l.count * r.v.nbatch));
    if (l.kind == SI_SYMM)
      hipLaunchKernelGGL(k_batch_selinv_symm<false>, grid, dim3(256), 0, st, r, tiles + l.first, l.count, units, rows, relpos);
    else if (l.kind == SI_SCALE)
      hipLaunchKernelGGL(k_batch_selinv_scale, grid, dim3(256), 0, st, r, tiles + l.first, l.count, units);
    else
      hipLaunchKernelGGL(k_batch_selinv_diag, grid, dim3(1024), 0, st, r, units + l.first, l.count);
  });
}

int launch_batch_selinv_symm_doubled(hipStream_t st, const BatchSelinvView& s, const SelinvLaunch& l,
                                     const SelinvUnit* units, const UpdTile* tiles, const SelinvRow* rows,
                                     const int* relpos) {
  if (l.kind != SI_SYMM) return 0;
  return bsi_member_ranges(s, l.count, [&](const BatchSelinvView& r, int) {
    hipLaunchKernelGGL(k_batch_selinv_symm<true>, dim3((unsigned)(l.count * r.v.nbatch)), dim3(256), 0, st, r,
                       tiles + l.first, l.count, units, rows, relpos);
  });
}

int launch_batch_selinv_fused(hipStream_t st, const BatchSelinvView& s, const SelinvUnit* units, int64_t count,
                              const SelinvRow* rows, const int* relpos) {
  return bsi_member_ranges(s, count, [&](const BatchSelinvView& r, int) {
    hipLaunchKernelGGL(k_batch_selinv_fused, dim3((unsigned)(count * r.v.nbatch)), dim3(256), 0, st, r, units, count, rows,
                       relpos);
  });
}

int launch_batch_selinv_diag_gather(hipStream_t st, const BatchSelinvView& s, const int64_t* diag_pos, const int* order,
                                    int n, double* out, int64_t ldout) {
  const int64_t nblk = ((int64_t)n + 255) / 256;
  return bsi_member_ranges(s, nblk, [&](const BatchSelinvView& r, int b0) {
    hipLaunchKernelGGL(k_batch_selinv_diag_gather, dim3((unsigned)(nblk * r.v.nbatch)), dim3(256), 0, st, r, diag_pos, order,
                       n, nblk, out + (int64_t)b0 * ldout, ldout);
  });
}

int launch_batch_selinv_pattern(hipStream_t st, const BatchSelinvView& s, const int64_t* map_dst, const int64_t* map_src,
                                int64_t nmap, double* out, int64_t ldout) {
  const int64_t nblk = (nmap + 255) / 256;
  return bsi_member_ranges(s, nblk, [&](const BatchSelinvView& r, int b0) {
    hipLaunchKernelGGL(k_batch_selinv_pattern, dim3((unsigned)(nblk * r.v.nbatch)), dim3(256), 0, st, r, map_dst, map_src,
                       nmap, nblk, out + (int64_t)b0 * ldout, ldout);
  });
}

}  // namespace spx
