// Blocked substitution for many right-hand sides for every member of a batch (batch.hip) on gfx950: the
// launches of the batch's solve program (pw = cb = 64) in the order of solve_batch, with the kernels of
// solve_many.hip -- a block of RB = 16 or 32 right-hand sides per member, every product on
// v_mfma_f64_16x16x4_f64 -- so that a member's arena is read once per RB vectors and not once per vector.
// The bodies are the SAME device functions (sm_body.hpp).
//
//   k_bsm_pack<RB, UNPACK>   caller's vectors x[b * xstride + q * ldx + i] <-> W_b[p(i) * RB + q]
//   k_bsm_diag<BWD, RB>      k_sm_diag for (block column, member)
//   k_bsm_strip_fwd<RB>      k_sm_strip_fwd for (strip, member)
//   k_bsm_strip_bwd<RB>      k_sm_strip_bwd for (strip, member)
//
// Member b: arena L + b * lstride, dinv scratch dinv + b * dstride (BatchView), workspace W + b * RB * n.  One
// launch carries all members, so the number of launches of a sweep does not depend on nbatch (unless the members
// are split into ranges).  A workgroup whose member is flagged (not positive definite) returns at once, before
// any barrier: the vectors of such a member are never touched, pack and unpack included.  The strips add with
// fp64 atomics, as in solve_many.hip: results repeat to rounding.  No inline assembly.
//
// Grid: the member is the slow axis (blockIdx.y) by default, as in batch_mult.hip: the workgroups of one member
// are consecutive and share its arena in L2.  member_fast = 1 makes the members of one work item consecutive
// on a linear grid.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>

#include "kernels.hpp"
#include "sm_body.hpp"
#include "sm_mm.hpp"

namespace spx {

// 64 rows of one member per workgroup (member blockIdx.y)
template <int RB, bool UNPACK>
__global__ __launch_bounds__(256) void k_bsm_pack(const BatchView v, double* __restrict__ x, int64_t xstride, int64_t ldx,
                                                  const int* __restrict__ order, int n, int nv, double* __restrict__ W) {
  __shared__ double tile[64][RB + 1];
  const int b = blockIdx.y;
  if (v.flag[b] != INT_MAX) return;   // (before any barrier)
  sm_pack_body<RB, UNPACK>((int)blockIdx.x * 64, x + (int64_t)b * xstride, ldx, order, n, nv,
                           W + (int64_t)b * RB * n, tile);
}

template <bool BWD, int RB>
__global__ __launch_bounds__(256) void k_bsm_diag(const BatchView v, const int* __restrict__ list,
                                                  const SolveUnit* __restrict__ units, double* W, int n) {
  __shared__ double T[64][RB + SM_PAD];
  int b;
  unsigned t;
  sm_member_split(v.member_fast, v.nbatch, b, t);
  if (v.flag[b] != INT_MAX) return;
  sm_diag_body<BWD, RB>(units[list[t]], v.L + (int64_t)b * v.lstride, v.dinv + (int64_t)b * v.dstride,
                        W + (int64_t)b * RB * n, T);
}

template <int RB>
__global__ __launch_bounds__(256) void k_bsm_strip_fwd(const BatchView v, const UpdTile* __restrict__ tiles,
                                                       const SolveUnit* __restrict__ units,
                                                       const int* __restrict__ rlist, double* W, int n) {
  int b;
  unsigned t;
  sm_member_split(v.member_fast, v.nbatch, b, t);
  if (v.flag[b] != INT_MAX) return;
  const UpdTile tl = tiles[t];
  sm_strip_fwd_body<RB>((int)tl.ti, units[tl.unit], v.L + (int64_t)b * v.lstride, rlist, W + (int64_t)b * RB * n);
}

template <int RB>
__global__ __launch_bounds__(256) void k_bsm_strip_bwd(const BatchView v, const UpdTile* __restrict__ tiles,
                                                       const SolveUnit* __restrict__ units,
                                                       const int* __restrict__ rlist, double* W, int n) {
  __shared__ double X[kSolveStripRows][RB + SM_PAD];
  int b;
  unsigned t;
  sm_member_split(v.member_fast, v.nbatch, b, t);
  if (v.flag[b] != INT_MAX) return;
  const UpdTile tl = tiles[t];
  sm_strip_bwd_body<RB>((int)tl.ti, units[tl.unit], v.L + (int64_t)b * v.lstride, rlist, W + (int64_t)b * RB * n, X);
}

// ---------------------------------------------------------------------------
// launch wrappers
// ---------------------------------------------------------------------------
namespace {
// fn(view of the member range, first member) for every range of members: at most 65535 members (the y extent of a
// grid) and at most batch_grid_limit() workgroups per launch; -1 (nothing launched) when ONE member's work items
// overflow a grid
template <class Fn>
int bsm_ranges(const BatchView& v, int64_t per_member, Fn&& fn) {
  if (per_member <= 0 || v.nbatch <= 0) return 0;
  if (per_member > batch_grid_limit_max()) return -1;
  const int64_t fit = std::max<int64_t>(1, batch_grid_limit() / per_member);
  const int step = (int)std::min<int64_t>(std::min<int64_t>(v.nbatch, 65535), fit);
  int launches = 0;
  for (int b0 = 0; b0 < v.nbatch; b0 += step) {
    BatchView s = v;
    s.nbatch = std::min(step, v.nbatch - b0);
    s.L += (int64_t)b0 * v.lstride;
    s.dinv += (int64_t)b0 * v.dstride;
    s.flag += b0;
    fn(s, b0);
    ++launches;
  }
  return launches;
}

dim3 bsm_grid(const BatchView& s, int64_t count) {
  return s.member_fast ? dim3((unsigned)(count * s.nbatch)) : dim3((unsigned)count, (unsigned)s.nbatch);
}

template <int RB>
int launch_bsm_rb(hipStream_t st, const BatchView& v, const SolveLaunch& l, const int* list, const UpdTile* tiles,
                  const SolveUnit* units, const int* rlist, double* W, int n) {
  const dim3 b(256);
  return bsm_ranges(v, l.count, [&](const BatchView& s, int b0) {
    const dim3 g = bsm_grid(s, l.count);
    double* Ws = W + (int64_t)b0 * RB * n;
    switch (l.kind) {
      case SV_DIAG_FWD:
        hipLaunchKernelGGL((k_bsm_diag<false, RB>), g, b, 0, st, s, list + l.first, units, Ws, n);
        break;
      case SV_DIAG_BWD:
        hipLaunchKernelGGL((k_bsm_diag<true, RB>), g, b, 0, st, s, list + l.first, units, Ws, n);
        break;
      case SV_STRIP_FWD:
        hipLaunchKernelGGL((k_bsm_strip_fwd<RB>), g, b, 0, st, s, tiles + l.first, units, rlist, Ws, n);
        break;
      default:
        hipLaunchKernelGGL((k_bsm_strip_bwd<RB>), g, b, 0, st, s, tiles + l.first, units, rlist, Ws, n);
        break;
    }
  });
}
}  // namespace

int launch_batch_solve_many(hipStream_t st, const BatchView& v, const SolveLaunch& l, const int* list,
                            const UpdTile* tiles, const SolveUnit* units, const int* rlist, double* W, int rb, int n) {
  if (l.count <= 0) return 0;
  return rb == 32 ? launch_bsm_rb<32>(st, v, l, list, tiles, units, rlist, W, n)
                  : launch_bsm_rb<16>(st, v, l, list, tiles, units, rlist, W, n);
}

int launch_batch_solve_many_pack(hipStream_t st, const BatchView& v, bool unpack, double* x, int64_t xstride, int64_t ldx,
                                 const int* order, int n, int nv, int rb, double* W) {
  if (n <= 0) return 0;
  const int64_t nblk = ((int64_t)n + 63) / 64;
  return bsm_ranges(v, nblk, [&](const BatchView& s, int b0) {
    const dim3 g((unsigned)nblk, (unsigned)s.nbatch), b(256);
    double* xs = x + (int64_t)b0 * xstride;
    double* Ws = W + (int64_t)b0 * rb * n;
    if (rb == 32) {
      if (unpack) hipLaunchKernelGGL((k_bsm_pack<32, true>), g, b, 0, st, s, xs, xstride, ldx, order, n, nv, Ws);
      else hipLaunchKernelGGL((k_bsm_pack<32, false>), g, b, 0, st, s, xs, xstride, ldx, order, n, nv, Ws);
    } else {
      if (unpack) hipLaunchKernelGGL((k_bsm_pack<16, true>), g, b, 0, st, s, xs, xstride, ldx, order, n, nv, Ws);
      else hipLaunchKernelGGL((k_bsm_pack<16, false>), g, b, 0, st, s, xs, xstride, ldx, order, n, nv, Ws);
    }
  });
}

}  // namespace spx
