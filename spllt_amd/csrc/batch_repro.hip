// Bit-reproducible batch for gfx950: the deterministic form of the batched factorization (batch.hip) and of the
// blocked many-right-hand-side sweep (batch_solve_many.hip).  Nothing here adds into memory another workgroup of
// the same launch writes: every sum has an order fixed by the shared tables, so the bits of a member depend on its
// values alone -- not on the run, on nbatch, on the member's place in the batch, on the grid mapping or on the
// split of the members into ranges.  Built without -munsafe-fp-atomics.
//
//   k_bdet_update<T>          k_batch_update (the same product loop, bu_body.hpp) with the epilogues TRSM (store),
//                             DIRECT (subtract in place, exclusive owner) and BUFFER: the product of an inter-node
//                             unit stored at scratch_b[u.d_off + i N + j] (the deterministic batch program,
//                             build_batch_program(deterministic = true))
//   k_bdet_gather             k_gather (kernels.hip) for (gather tile, member): the items of a destination tile in
//                             table order through a 64 x 65 LDS tile, one read-modify-write of the destination
//   k_brsm_diag<BWD, RB>      the stored strip products subtracted in table order, then sm_diag_body
//   k_brsm_strip_fwd/bwd<RB>  the products of the strips of k_bsm_strip_*, stored (rsm_body.hpp)
//
// k_batch_init, k_batch_chain and k_batch_log_det of batch.hip and the pack / unpack of batch_solve_many.hip have no
// cross-workgroup adds and are used as they are.  Member b: arena L + b lstride, dinv + b dstride, flag + b,
// scratch + b sstride, workspace W + b RB n.  A workgroup whose member is flagged returns before any barrier.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>

#include "batch_split.hpp"
#include "bu_body.hpp"
#include "kernels.hpp"
#include "rsm_body.hpp"
#include "sm_body.hpp"
#include "sm_mm.hpp"

namespace spx {

// ---------------------------------------------------------------------------
// factorization
// ---------------------------------------------------------------------------
template <int T>
__global__ __launch_bounds__(256) void k_bdet_update(BatchReproView s, const UpdTile* __restrict__ tiles, int64_t count,
                                                     const UpdUnit* __restrict__ units,
                                                     const int64_t* __restrict__ bc_off, const int* __restrict__ bc_w) {
  constexpr int NC = T == 64 ? 4 : 1;
  __shared__ double As[T][BU_LD];
  __shared__ double Bs[T][BU_LD];
  int b;
  int64_t t;
  bsi_split(s.v, count, b, t);
  if (s.v.flag[b] != INT_MAX) return;   // (before any barrier)
  const UpdTile tl = tiles[t];
  const UpdUnit u = units[tl.unit];
  double* Lb = s.v.L + (int64_t)b * s.v.lstride;
  const double* Db = s.v.dinv + (int64_t)b * s.v.dstride;
  const int i0 = tl.ti * T, j0 = tl.tj * T;
  const int mi = min(T, u.M - i0), nj = min(T, u.N - j0);
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int g = lane >> 4, col = lane & 15;
  const int rb = T == 64 ? wv : (wv >> 1), cb0 = T == 64 ? 0 : (wv & 1);
  d4 acc[NC];
  bu_product<T>(u, i0, j0, mi, nj, Lb, Db, bc_off, bc_w, As, Bs, acc);
  // (every read of the tile's operands lies before the last barrier: the TRSM epilogue may overwrite them)
  double* D = u.mode == MODE_BUFFER ? s.scratch + (int64_t)b * s.sstride + u.d_off : Lb + u.d_off;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int j = j0 + 16 * (cb0 + c) + col;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + 16 * rb + g + 4 * r;
      if (i >= i0 + mi || j >= j0 + nj) continue;
      const double p = acc[c][r];
      if (u.mode == MODE_TRSM) {
        D[(int64_t)(u.d_row0 + i) * u.d_ld + u.d_col0 + j] = p;
        continue;
      }
      if (u.lower && u.src_r0 + i < u.src_c0 + j) continue;
      if (u.mode == MODE_DIRECT) D[(int64_t)(u.d_row0 + i) * u.d_ld + u.d_col0 + j] -= p;
      else D[(int64_t)i * u.N + j] = p;   // BUFFER: M x N row-major, what the gather reads
    }
  }
}

// destination tile -= sum over its items, in list order, of the buffered blocks: the arithmetic of k_gather
__global__ __launch_bounds__(256) void k_bdet_gather(BatchReproView s, const GatherTile* __restrict__ tiles, int64_t count,
                                                     const GatherItem* __restrict__ items,
                                                     const int* __restrict__ relpos, const int* __restrict__ rlist) {
  __shared__ double acc[64 * 65];
  int b;
  int64_t t;
  bsi_split(s.v, count, b, t);
  if (s.v.flag[b] != INT_MAX) return;   // (before any barrier)
  const GatherTile gt = tiles[t];
  const double* scratch = s.scratch + (int64_t)b * s.sstride;
  const int tid = threadIdx.x;
  for (int e = tid; e < 64 * 65; e += 256) acc[e] = 0.0;
  __syncthreads();
  for (int it = 0; it < gt.count; ++it) {
    const GatherItem g = items[gt.first + it];
    const int ni = g.i1 - g.i0, nj = g.j1 - g.j0;
    const double* buf = scratch + g.buf_off;
    for (int e = tid; e < ni * nj; e += 256) {
      const int i = g.i0 + e / nj, j = g.j0 + e % nj;
      if (g.lower && g.diag_shift + i < j) continue;
      const int r = relpos[g.relrow_off + i] - gt.drow_base - gt.row0;
      const int c = rlist[g.gcol_off + j] - gt.dcol_base - gt.col0;
      acc[r * 65 + c] += buf[(int64_t)i * g.ld + j];   // (i, j) -> (r, c) is injective inside an item
    }
    __syncthreads();   // the next item may hit the same entries
  }
  double* D = s.v.L + (int64_t)b * s.v.lstride + gt.d_off + (int64_t)gt.row0 * gt.d_ld + gt.col0;
  for (int e = tid; e < gt.rows * gt.cols; e += 256) {
    const int r = e / gt.cols, c = e % gt.cols;
    const double a = acc[r * 65 + c];
    if (a != 0.0) D[(int64_t)r * gt.d_ld + c] -= a;
  }
}

// ---------------------------------------------------------------------------
// blocked sweep
// ---------------------------------------------------------------------------
template <bool BWD, int RB>
__global__ __launch_bounds__(256) void k_brsm_diag(const BatchReproView s, const int* __restrict__ list,
                                                   const SolveUnit* __restrict__ units, const RsmTables tb, double* W,
                                                   int n) {
  __shared__ double T[64][RB + SM_PAD];
  int b;
  unsigned t;
  sm_member_split(s.v.member_fast, s.v.nbatch, b, t);
  if (s.v.flag[b] != INT_MAX) return;
  const int id = list[t];
  const SolveUnit u = units[id];
  double* Wb = W + (int64_t)b * RB * n;
  rsm_gather_body<BWD, RB>(u, id, tb, Wb, s.scratch + (int64_t)b * s.sstride);
  sm_diag_body<BWD, RB>(u, s.v.L + (int64_t)b * s.v.lstride, s.v.dinv + (int64_t)b * s.v.dstride, Wb, T);
}

template <int RB>
__global__ __launch_bounds__(256) void k_brsm_strip_fwd(const BatchReproView s, const UpdTile* __restrict__ tiles,
                                                        const SolveUnit* __restrict__ units, const RsmTables tb,
                                                        const double* W, int n) {
  int b;
  unsigned t;
  sm_member_split(s.v.member_fast, s.v.nbatch, b, t);
  if (s.v.flag[b] != INT_MAX) return;
  const UpdTile tl = tiles[t];
  rsm_strip_fwd_body<RB>((int)tl.ti, units[tl.unit], tb.fslot[tl.unit], s.v.L + (int64_t)b * s.v.lstride,
                         W + (int64_t)b * RB * n, s.scratch + (int64_t)b * s.sstride);
}

// (bslot: the entries of the launch's tiles, RsmTables::bslot + the launch's first tile)
template <int RB>
__global__ __launch_bounds__(256) void k_brsm_strip_bwd(const BatchReproView s, const UpdTile* __restrict__ tiles,
                                                        const SolveUnit* __restrict__ units,
                                                        const int* __restrict__ rlist, const int64_t* __restrict__ bslot,
                                                        const double* W, int n) {
  __shared__ double X[kSolveStripRows][RB + SM_PAD];
  int b;
  unsigned t;
  sm_member_split(s.v.member_fast, s.v.nbatch, b, t);
  if (s.v.flag[b] != INT_MAX) return;
  const UpdTile tl = tiles[t];
  rsm_strip_bwd_body<RB>((int)tl.ti, units[tl.unit], bslot[t], s.v.L + (int64_t)b * s.v.lstride, rlist,
                         W + (int64_t)b * RB * n, s.scratch + (int64_t)b * s.sstride, X);
}

// ---------------------------------------------------------------------------
// launch wrappers
// ---------------------------------------------------------------------------
namespace {
// fn(view of the members [b0, b0 + nbatch), b0) for every range of at most max_members members whose grid fits:
// L, dinv, flag AND the scratch move with b0
template <class Fn>
int brp_ranges(const BatchReproView& s, int64_t per_member, int max_members, Fn&& fn) {
  if (per_member <= 0 || s.v.nbatch <= 0) return 0;
  if (per_member > batch_grid_limit_max()) return -1;
  const int64_t fit = std::max<int64_t>(1, batch_grid_limit() / per_member);
  const int step = (int)std::min<int64_t>(std::min<int64_t>(s.v.nbatch, max_members), fit);
  int launches = 0;
  for (int b0 = 0; b0 < s.v.nbatch; b0 += step) {
    BatchReproView r = s;
    r.v.nbatch = std::min(step, s.v.nbatch - b0);
    r.v.L += (int64_t)b0 * s.v.lstride;
    r.v.dinv += (int64_t)b0 * s.v.dstride;
    r.v.flag += b0;
    if (r.scratch) r.scratch += (int64_t)b0 * s.sstride;   // (null: a program without inter-node updates)
    fn(r, b0);
    ++launches;
  }
  return launches;
}

template <int RB>
int launch_brsm_rb(hipStream_t st, const BatchReproView& s, const SolveLaunch& l, const int* list, const UpdTile* tiles,
                   const SolveUnit* units, const int* rlist, const RsmTables& tb, double* W, int n) {
  const dim3 b(256);
  // (65535: the y extent of a grid, the member axis of the default mapping)
  return brp_ranges(s, l.count, 65535, [&](const BatchReproView& r, int b0) {
    const dim3 g = r.v.member_fast ? dim3((unsigned)(l.count * r.v.nbatch)) : dim3((unsigned)l.count, (unsigned)r.v.nbatch);
    double* Ws = W + (int64_t)b0 * RB * n;
    switch (l.kind) {
      case SV_DIAG_FWD:
        hipLaunchKernelGGL((k_brsm_diag<false, RB>), g, b, 0, st, r, list + l.first, units, tb, Ws, n);
        break;
      case SV_DIAG_BWD:
        hipLaunchKernelGGL((k_brsm_diag<true, RB>), g, b, 0, st, r, list + l.first, units, tb, Ws, n);
        break;
      case SV_STRIP_FWD:
        hipLaunchKernelGGL((k_brsm_strip_fwd<RB>), g, b, 0, st, r, tiles + l.first, units, tb, Ws, n);
        break;
      default:
        hipLaunchKernelGGL((k_brsm_strip_bwd<RB>), g, b, 0, st, r, tiles + l.first, units, rlist, tb.bslot + l.first, Ws, n);
        break;
    }
  });
}
}  // namespace

int launch_bdet_update(hipStream_t st, const BatchReproView& s, int tile, const UpdTile* tiles, int64_t count,
                       const UpdUnit* units, const int64_t* bc_off, const int* bc_w) {
  return brp_ranges(s, count, INT_MAX, [&](const BatchReproView& r, int) {
    const dim3 g((unsigned)(count * r.v.nbatch)), b(256);
    if (tile == 64) hipLaunchKernelGGL(k_bdet_update<64>, g, b, 0, st, r, tiles, count, units, bc_off, bc_w);
    else hipLaunchKernelGGL(k_bdet_update<32>, g, b, 0, st, r, tiles, count, units, bc_off, bc_w);
  });
}

int launch_bdet_gather(hipStream_t st, const BatchReproView& s, const GatherTile* tiles, int64_t count,
                       const GatherItem* items, const int* relpos, const int* rlist) {
  return brp_ranges(s, count, INT_MAX, [&](const BatchReproView& r, int) {
    hipLaunchKernelGGL(k_bdet_gather, dim3((unsigned)(count * r.v.nbatch)), dim3(256), 0, st, r, tiles, count, items, relpos,
                       rlist);
  });
}

int launch_batch_solve_repro(hipStream_t st, const BatchReproView& s, const SolveLaunch& l, const int* list,
                             const UpdTile* tiles, const SolveUnit* units, const int* rlist, const RsmTables& tb,
                             double* W, int rb, int n) {
  if (l.count <= 0) return 0;
  return rb == 32 ? launch_brsm_rb<32>(st, s, l, list, tiles, units, rlist, tb, W, n)
                  : launch_brsm_rb<16>(st, s, l, list, tiles, units, rlist, tb, W, n);
}

}  // namespace spx
