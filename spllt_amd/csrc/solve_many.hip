// Blocked substitution for many right-hand sides on gfx950 (schedule.hpp, SolveProgram): the
// launches of the existing device solve in the same order, with kernels that take a block of
// RB = 16 or 32 right-hand sides and do every product on v_mfma_f64_16x16x4_f64, so that L is read
// once per RB vectors.
//
// Workspace layout: W[p * RB + q], pivot position p, right-hand side q < RB -- the RB values of one
// row are contiguous (128 or 256 bytes), so a row of W is a dense MFMA B operand and the scatter of
// a result row to idx[r] is RB contiguous doubles.
//
//   k_sm_pack / k_sm_unpack   caller's vectors (x[q * ldx + i], user or pivot order) <-> W,
//                             transposed through LDS; a short block is zero-filled in W only
//   k_sm_diag<BWD>            one block column per workgroup, panel by panel with the inverted
//                             diagonal panels of the dinv scratch; x stays in W (L2) between panels
//   k_sm_strip_fwd            W[idx[r]] -= L[r, :] x_J      for a strip of 64 rows
//   k_sm_strip_bwd            W[J]      -= L[R, J]^T x_R    for a strip of 64 rows
//
// Lane l of a wavefront supplies A[l&15][l>>4] and B[l>>4][l&15] and receives C[(l>>4) + 4 r][l&15]
// in register r.  The strips add with fp64 atomics (several block columns of a level hit the same
// rows): results are reproducible to rounding only, like the existing solve.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.hpp"
#include "sm_body.hpp"
#include "sm_mm.hpp"

namespace spx {

// The bodies live in sm_body.hpp (shared with batch_solve_many.hip); the kernels here only say which arena,
// which dinv scratch and which workspace.

// 64 rows per workgroup
template <int RB, bool UNPACK>
__global__ __launch_bounds__(256) void k_sm_pack(double* __restrict__ x, int64_t ldx, const int* __restrict__ order,
                                                 int n, int nv, double* __restrict__ W) {
  __shared__ double tile[64][RB + 1];
  sm_pack_body<RB, UNPACK>((int)blockIdx.x * 64, x, ldx, order, n, nv, W, tile);
}

// one block column per workgroup (single: the one block column u0 of the launch)
template <bool BWD, int RB>
__global__ __launch_bounds__(256) void k_sm_diag(const int* __restrict__ list, const SolveUnit* __restrict__ units,
                                                 const double* __restrict__ L, const double* __restrict__ dinv,
                                                 double* W, const SolveUnit u0, int single) {
  __shared__ double T[64][RB + SM_PAD];
  sm_diag_body<BWD, RB>(single ? u0 : units[list[blockIdx.x]], L, dinv, W, T);
}

// one strip of kSolveStripRows (64) rows per workgroup
// (single: all strips of the launch belong to ONE block column, strip i = workgroup i)
template <int RB>
__global__ __launch_bounds__(256) void k_sm_strip_fwd(const UpdTile* __restrict__ tiles,
                                                      const SolveUnit* __restrict__ units, const double* __restrict__ L,
                                                      const int* __restrict__ rlist, double* W, const SolveUnit u0,
                                                      int single) {
  const int ti = single ? (int)blockIdx.x : (int)tiles[blockIdx.x].ti;
  sm_strip_fwd_body<RB>(ti, single ? u0 : units[tiles[blockIdx.x].unit], L, rlist, W);
}

template <int RB>
__global__ __launch_bounds__(256) void k_sm_strip_bwd(const UpdTile* __restrict__ tiles,
                                                      const SolveUnit* __restrict__ units, const double* __restrict__ L,
                                                      const int* __restrict__ rlist, double* W, const SolveUnit u0,
                                                      int single) {
  __shared__ double X[kSolveStripRows][RB + SM_PAD];
  const int ti = single ? (int)blockIdx.x : (int)tiles[blockIdx.x].ti;
  sm_strip_bwd_body<RB>(ti, single ? u0 : units[tiles[blockIdx.x].unit], L, rlist, W, X);
}

// ---------------------------------------------------------------------------
// launch wrappers
// ---------------------------------------------------------------------------
template <int RB>
static void launch_solve_many_rb(hipStream_t st, const SolveTablesView& t, const SolveLaunch& l,
                                 const SolveLaunchInfo& li, double* W) {
  const dim3 g((unsigned)l.count), b(256);
  const int* list = t.list + l.first;          // DIAG launches: the block columns
  const UpdTile* tiles = t.tiles + l.first;    // STRIP launches: the (block column, strip) pairs
  const SolveUnit u0 = li.one ? *li.one : SolveUnit{};
  const int single = li.one ? 1 : 0;
  switch (l.kind) {
    case SV_DIAG_FWD:
      hipLaunchKernelGGL((k_sm_diag<false, RB>), g, b, 0, st, list, t.units, t.L, t.dinv, W, u0, single);
      break;
    case SV_DIAG_BWD:
      hipLaunchKernelGGL((k_sm_diag<true, RB>), g, b, 0, st, list, t.units, t.L, t.dinv, W, u0, single);
      break;
    case SV_STRIP_FWD:
      hipLaunchKernelGGL((k_sm_strip_fwd<RB>), g, b, 0, st, tiles, t.units, t.L, t.rlist, W, u0, single);
      break;
    default:
      hipLaunchKernelGGL((k_sm_strip_bwd<RB>), g, b, 0, st, tiles, t.units, t.L, t.rlist, W, u0, single);
      break;
  }
}

void launch_solve_many(hipStream_t st, const SolveTablesView& t, const SolveLaunch& l, const SolveLaunchInfo& li,
                       double* W, int rb) {
  if (l.count <= 0) return;
  if (rb == 32)
    launch_solve_many_rb<32>(st, t, l, li, W);
  else
    launch_solve_many_rb<16>(st, t, l, li, W);
}

void launch_solve_many_pack(hipStream_t st, const double* x, int64_t ldx, const int* order, int n, int nv, int rb,
                            double* W) {
  if (n <= 0) return;
  const dim3 g((unsigned)((n + 63) / 64)), b(256);
  double* xs = const_cast<double*>(x);   // (the pack instance only reads it)
  if (rb == 32)
    hipLaunchKernelGGL((k_sm_pack<32, false>), g, b, 0, st, xs, ldx, order, n, nv, W);
  else
    hipLaunchKernelGGL((k_sm_pack<16, false>), g, b, 0, st, xs, ldx, order, n, nv, W);
}

void launch_solve_many_unpack(hipStream_t st, double* x, int64_t ldx, const int* order, int n, int nv, int rb,
                              double* W) {
  if (n <= 0) return;
  const dim3 g((unsigned)((n + 63) / 64)), b(256);
  if (rb == 32)
    hipLaunchKernelGGL((k_sm_pack<32, true>), g, b, 0, st, x, ldx, order, n, nv, W);
  else
    hipLaunchKernelGGL((k_sm_pack<16, true>), g, b, 0, st, x, ldx, order, n, nv, W);
}

}  // namespace spx
