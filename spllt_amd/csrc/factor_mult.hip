// Products with the factor on gfx950: Y = L X and Y = L^T X for a block of RB = 16 or 32 vectors in the
// workspace layout of solve_many.hip (W[p * RB + q], pivot position p, vector q), out of place between two
// workspaces, every product on v_mfma_f64_16x16x4_f64 (sm_mm.hpp).  A product has no dependency chain:
// every (block column, strip) tile of the SolveProgram is independent, so a direction is TWO launches
// whatever the tree looks like:
//
//   k_fm_strip<T>   one workgroup per tile of "solve_tiles": the product of the strip's 64 rows with the
//                   block column's own rows of X (L X), or of its transpose with the strip's rows of X
//                   (L^T X), STORED into the scratch at the slots of the RsolveTables (schedule.hpp)
//   k_fm_diag<T>    one workgroup per 64 pivot positions of a block column: the product with the diagonal
//                   tile, read from the arena and masked to its lower triangle (the strict upper part of a
//                   diagonal tile is never written), plus the stored products that belong to these
//                   positions, added in table order
//
// Scratch layout: slot s of the tables (an offset in doubles inside the scratch of ONE vector of the
// reproducible solve) is the row scratch[s * RB .. s * RB + RB): one 128- or 256-byte row per slot.
//
// No atomic add.  For vector q every sum runs in an order fixed by the tables and by K, never by RB or by
// q's place in the block: the same factor bits and vector bits give the same result bits.
//
// The noise of the samplers: Philox4x32-10, counter (pivot position, 0, sample lo, sample hi), key (seed
// lo, seed hi); Box-Muller on the two 53-bit uniforms of that one block, one value per block.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fm_body.hpp"
#include "kernels.hpp"
#include "sm_mm.hpp"

namespace spx {

// ---------------------------------------------------------------------------
// the kernels: the bodies of fm_body.hpp (shared with batch_mult.hip) on the one arena of the handle
// ---------------------------------------------------------------------------
template <bool T, int RB>
__global__ __launch_bounds__(256) void k_fm_strip(const UpdTile* __restrict__ tiles, const SolveUnit* __restrict__ units,
                                                  const double* __restrict__ L, const int* __restrict__ rlist,
                                                  const double* __restrict__ X, const FmultView fv) {
  __shared__ double Xs[T ? kSolveStripRows : 1][RB + SM_PAD];
  const UpdTile tl = tiles[blockIdx.x];
  fm_strip_body<T, RB>(tl, blockIdx.x, units[tl.unit], L, rlist, X, fv, Xs);
}

template <bool T, int RB>
__global__ __launch_bounds__(256) void k_fm_diag(const UpdTile* __restrict__ chunks, const SolveUnit* __restrict__ units,
                                                 const double* __restrict__ L, const double* __restrict__ X,
                                                 double* __restrict__ Y, const FmultView fv) {
  __shared__ double Ts[T ? 1 : 64][RB + SM_PAD];
  const UpdTile ch = chunks[blockIdx.x];
  fm_diag_body<T, RB>(ch, units[ch.unit], L, X, Y, fv, Ts);
}

// ---------------------------------------------------------------------------
// noise and mean (fm_normal: fm_body.hpp; the single handle draws from stream 0)
// ---------------------------------------------------------------------------
// z[q * ldz + i] = normal(pivot position of i, first + q): order null -- i IS the pivot position
__global__ __launch_bounds__(256) void k_fm_noise(double* __restrict__ z, int64_t ldz, const int* __restrict__ order, int n,
                                                  uint64_t seed, uint64_t first) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int p = order ? order[i] : i;
  z[(int64_t)blockIdx.y * ldz + i] = fm_normal((uint32_t)p, 0u, first + blockIdx.y, seed);
}

__global__ __launch_bounds__(256) void k_fm_add_mean(double* __restrict__ x, int64_t ldx, const double* __restrict__ mean,
                                                     int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) x[(int64_t)blockIdx.y * ldx + i] += mean[i];
}

// ---------------------------------------------------------------------------
// launch wrappers
// ---------------------------------------------------------------------------
template <int RB>
static void launch_fmult_rb(hipStream_t st, const SolveTablesView& t, int64_t ntiles, const UpdTile* chunks,
                            int64_t nchunks, bool transpose, const double* X, double* Y, const FmultView& fv) {
  const dim3 b(256);
  if (transpose) {
    if (ntiles > 0)
      hipLaunchKernelGGL((k_fm_strip<true, RB>), dim3((unsigned)ntiles), b, 0, st, t.tiles, t.units, t.L, t.rlist, X, fv);
    hipLaunchKernelGGL((k_fm_diag<true, RB>), dim3((unsigned)nchunks), b, 0, st, chunks, t.units, t.L, X, Y, fv);
  } else {
    if (ntiles > 0)
      hipLaunchKernelGGL((k_fm_strip<false, RB>), dim3((unsigned)ntiles), b, 0, st, t.tiles, t.units, t.L, t.rlist, X, fv);
    hipLaunchKernelGGL((k_fm_diag<false, RB>), dim3((unsigned)nchunks), b, 0, st, chunks, t.units, t.L, X, Y, fv);
  }
}

void launch_factor_mult(hipStream_t st, const SolveTablesView& t, int64_t ntiles, const UpdTile* chunks, int64_t nchunks,
                        bool transpose, const double* X, double* Y, int rb, const FmultView& fv) {
  if (nchunks <= 0) return;
  if (rb == 32)
    launch_fmult_rb<32>(st, t, ntiles, chunks, nchunks, transpose, X, Y, fv);
  else
    launch_fmult_rb<16>(st, t, ntiles, chunks, nchunks, transpose, X, Y, fv);
}

void launch_white_noise(hipStream_t st, double* z, int64_t ldz, const int* order, int n, int nsamp, uint64_t seed,
                        uint64_t first) {
  if (n <= 0) return;
  for (int done = 0; done < nsamp; done += 32768) {   // (the y extent of a grid is 16 bits)
    const int cur = nsamp - done < 32768 ? nsamp - done : 32768;
    hipLaunchKernelGGL(k_fm_noise, dim3((unsigned)((n + 255) / 256), (unsigned)cur), dim3(256), 0, st,
                       z + (int64_t)done * ldz, ldz, order, n, seed, first + (uint64_t)done);
  }
}

void launch_add_mean(hipStream_t st, double* x, int64_t ldx, const double* mean, int n, int nvec) {
  if (n <= 0) return;
  for (int done = 0; done < nvec; done += 32768) {
    const int cur = nvec - done < 32768 ? nvec - done : 32768;
    hipLaunchKernelGGL(k_fm_add_mean, dim3((unsigned)((n + 255) / 256), (unsigned)cur), dim3(256), 0, st,
                       x + (int64_t)done * ldx, ldx, mean, n);
  }
}

}  // namespace spx
