// Reproducible substitution: the launches of the SolveProgram (schedule.hpp) with no atomic add.  A strip
// launch STORES its products into a scratch vector (one per right-hand side of the sweep); the diagonal
// launch that owns a row subtracts the stored products in the order of the RsolveTables before it runs the
// arithmetic of the plain diagonal solve (solve_diag.hpp, shared with kernels.hip).  Every sum therefore
// has an order fixed by the symbolic structure and the launch geometry: the same factor bits and the same
// right-hand-side bits give the same solution bits.
//
// Group independence: every operation on vector q reads and writes values of vector q only, in an order that
// does not depend on NR -- the NR = 1, 2 and 4 instances differ in how many such independent chains a thread
// carries.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "kernels.hpp"
#include "solve_diag.hpp"

namespace spx {

// Forward: own row j of the block column, pivot position p = gcol0 + j:
//   xb[j] = y[p] - sum16( lane sub: scratch[gsrc[k]] for k = gptr[p] + sub, + 16, ... added in that order )
// 16 lanes per row, 16 rows per pass (the geometry of the diagonal solve itself): the lists are short at the
// leaves and hundreds long at the top of the tree, where one thread per row would walk them alone.  Four
// index loads, then four value loads per vector, are in flight per lane.
template <int NR>
__device__ __forceinline__ void gather_fwd(const SolveUnit& u, const RsolveView& rv, const double* __restrict__ y,
                                           int64_t ldy, double* xb, int xs) {
  const int sub = threadIdx.x & 15, rr = threadIdx.x >> 4;
  const int w = u.w;
  for (int j0 = 0; j0 < w; j0 += 16) {
    const int j = j0 + rr;
    const int p = u.gcol0 + min(j, w - 1);
    const int64_t g0 = rv.gptr[p], g1 = rv.gptr[p + 1];
    double acc[NR];
#pragma unroll
    for (int q = 0; q < NR; ++q) acc[q] = 0.0;
    for (int64_t k = g0 + sub; k < g1; k += 64) {
      int64_t s[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) s[e] = rv.gsrc[k + 16 * e < g1 ? k + 16 * e : g1 - 1];
#pragma unroll
      for (int q = 0; q < NR; ++q) {
        double v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = rv.scratch[q * rv.stride + s[e]];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[q] += k + 16 * e < g1 ? v[e] : 0.0;
      }
    }
#pragma unroll
    for (int q = 0; q < NR; ++q) {
      const double tot = sum16(acc[q]);
      if (sub == 0 && j < w) xb[q * xs + j] = y[q * ldy + p] - tot;
    }
  }
}

// Backward: xb[j] = y[p] - partial(strip 0)[j] - partial(strip 1)[j] - ...  in ascending strip index
template <int NR>
__device__ __forceinline__ void gather_bwd(const SolveUnit& u, const RsolveView& rv, int64_t bfirst,
                                           const double* __restrict__ y, int64_t ldy, double* xb, int xs) {
  const int w = u.w;
  const int ns = (u.nrow - w + kSolveStripRows - 1) / kSolveStripRows;
  for (int j = threadIdx.x; j < w; j += 256) {
    const int p = u.gcol0 + j;
#pragma unroll
    for (int q = 0; q < NR; ++q) {
      double v = y[q * ldy + p];
      const double* part = rv.scratch + q * rv.stride + bfirst + j;
#pragma unroll 4
      for (int t = 0; t < ns; ++t) v -= part[(int64_t)t * w];
      xb[q * xs + j] = v;
    }
  }
}

template <bool BWD, bool FOUR, int NR>
__global__ __launch_bounds__(256) void k_rsolve_diag(const int* __restrict__ list, const SolveUnit* __restrict__ units,
                                                     const double* __restrict__ L, const double* __restrict__ dinv,
                                                     double* __restrict__ y, int64_t ldy, const SolveUnit u0, int single,
                                                     const RsolveView rv) {
  const int id = list[blockIdx.x];
  const SolveUnit u = single ? u0 : units[id];
  auto fill = [&](double* xb, int xs) {
    if (BWD) gather_bwd<NR>(u, rv, rv.bfirst[id], y, ldy, xb, xs);
    else gather_fwd<NR>(u, rv, y, ldy, xb, xs);
  };
  if (FOUR) solve_diag4_body<BWD, NR>(u, L, dinv, y, ldy, fill);
  else solve_diag_body<BWD, NR>(u, L, dinv, y, ldy, fill);
}

// Rows below the diagonal tile, one strip of kSolveStripRows rows per workgroup: the products of
// k_solve_strip (kernels.hip), stored.
//   forward : scratch[fslot + r - w] = sum_k L[r][k] x_k
//   backward: scratch[bslot + k]     = sum_r L[r][k] x[idx[r]]   (r over the strip's rows, ascending)
template <bool BWD, int NR>
__global__ __launch_bounds__(256) void k_rsolve_strip(const UpdTile* __restrict__ tiles, const SolveUnit* __restrict__ units,
                                                      const double* __restrict__ L, const int* __restrict__ rlist,
                                                      const double* __restrict__ y, int64_t ldy, const SolveUnit u0, int single,
                                                      const RsolveView rv, const int64_t* __restrict__ bslot) {
  __shared__ double xb[NR * kXS];
  const UpdTile tl = tiles[blockIdx.x];
  const int ti = tl.ti;
  const SolveUnit u = single ? u0 : units[tl.unit];
  const int tid = threadIdx.x;
  const int w = u.w;
  const int r0 = w + ti * kSolveStripRows;
  const int nr = min(kSolveStripRows, u.nrow - r0);
  const double* A = L + u.off + (int64_t)r0 * w;
  if (!BWD) {
    for (int k = tid; k < w; k += 256) {
      const int gi = u.gcol0 + k;
#pragma unroll
      for (int q = 0; q < NR; ++q) xb[q * kXS + k] = y[q * ldy + gi];
    }
    __syncthreads();
    const int sub = tid & 15, rr = tid >> 4;
    double acc[4][NR];
#pragma unroll
    for (int r = 0; r < 4; ++r)
      dot16<NR, kXS>(A + (int64_t)min(rr + 16 * r, nr - 1) * w, xb, w, sub, acc[r]);
    double* out = rv.scratch + rv.fslot[tl.unit] + (r0 - w);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = rr + 16 * r;
#pragma unroll
      for (int q = 0; q < NR; ++q) {
        const double sacc = sum16(acc[r][q]);
        if (sub == 0 && row < nr) out[q * rv.stride + row] = sacc;
      }
    }
  } else {
    const int* idx = rlist + u.idx_off;
    for (int r = tid; r < nr; r += 256) {
      const int gi = idx[r0 + r];
#pragma unroll
      for (int q = 0; q < NR; ++q) xb[q * kXS + r] = y[q * ldy + gi];
    }
    __syncthreads();
    double* out = rv.scratch + bslot[blockIdx.x];
    for (int k = tid; k < w; k += 256) {
      double sa[NR];
#pragma unroll
      for (int q = 0; q < NR; ++q) sa[q] = 0.0;
      for (int q0 = 0; q0 < nr; q0 += 8) {
        double v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = A[(int64_t)min(q0 + e, nr - 1) * w + k];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const double a = q0 + e < nr ? v[e] : 0.0;
#pragma unroll
          for (int q = 0; q < NR; ++q) sa[q] = __builtin_fma(a, xb[q * kXS + min(q0 + e, nr - 1)], sa[q]);
        }
      }
#pragma unroll
      for (int q = 0; q < NR; ++q) out[q * rv.stride + k] = sa[q];
    }
  }
}

template <int NR>
static void launch_rsolve_nr(hipStream_t st, const SolveTablesView& t, const SolveLaunch& l, const SolveLaunchInfo& li,
                             double* y, int64_t ldy, const RsolveView& rv) {
  const dim3 g((unsigned)l.count), b(256);
  const int* list = t.list + l.first;          // DIAG launches: the block columns
  const UpdTile* tiles = t.tiles + l.first;    // STRIP launches: the (block column, strip) pairs
  const SolveUnit u0 = li.one ? *li.one : SolveUnit{};
  const int single = li.one ? 1 : 0;
  switch (l.kind) {
    case SV_DIAG_FWD:
      if (li.four)
        hipLaunchKernelGGL((k_rsolve_diag<false, true, NR>), g, b, 0, st, list, t.units, t.L, t.dinv, y, ldy, u0, single, rv);
      else
        hipLaunchKernelGGL((k_rsolve_diag<false, false, NR>), g, b, 0, st, list, t.units, t.L, t.dinv, y, ldy, u0, single, rv);
      break;
    case SV_DIAG_BWD:
      if (li.four)
        hipLaunchKernelGGL((k_rsolve_diag<true, true, NR>), g, b, 0, st, list, t.units, t.L, t.dinv, y, ldy, u0, single, rv);
      else
        hipLaunchKernelGGL((k_rsolve_diag<true, false, NR>), g, b, 0, st, list, t.units, t.L, t.dinv, y, ldy, u0, single, rv);
      break;
    case SV_STRIP_FWD:
      hipLaunchKernelGGL((k_rsolve_strip<false, NR>), g, b, 0, st, tiles, t.units, t.L, t.rlist, y, ldy, u0, single, rv,
                         rv.bslot + l.first);
      break;
    default:
      hipLaunchKernelGGL((k_rsolve_strip<true, NR>), g, b, 0, st, tiles, t.units, t.L, t.rlist, y, ldy, u0, single, rv,
                         rv.bslot + l.first);
      break;
  }
}

void launch_solve_repro(hipStream_t st, const SolveTablesView& t, const SolveLaunch& l, const SolveLaunchInfo& li,
                        double* y, int nr, int64_t ldy, const RsolveView& rv) {
  if (l.count <= 0) return;
  if (nr >= 4)
    launch_rsolve_nr<4>(st, t, l, li, y, ldy, rv);
  else if (nr >= 2)
    launch_rsolve_nr<2>(st, t, l, li, y, ldy, rv);
  else
    launch_rsolve_nr<1>(st, t, l, li, y, ldy, rv);
}

}  // namespace spx
