// Products with the factors of a batch on gfx950: Y_b = L_b X_b and Y_b = L_b^T X_b for every member b of a
// batch (batch.hip) and a block of RB = 16 or 32 vectors per member, plus the noise and the mean of the
// batched samplers.  The work is that of factor_mult.hip, the bodies are the SAME device functions
// (fm_body.hpp): a member's arena has the layout of the single arena, so the handle's solve_units /
// solve_tiles and the RsolveTables apply to it unchanged, and for the same arena bits and vector bits a
// member's result has the bits of the single-handle product.
//
//   k_bm_pack<RB, UNPACK>  caller's vectors x[b * xstride + q * ldx + i] <-> W_b[p(i) * RB + q]
//   k_bm_strip<T, RB>      k_fm_strip for (tile, member)
//   k_bm_diag<T, RB>       k_fm_diag for (chunk, member)
//   k_bm_noise             k_fm_noise for (position, sample, member): stream = stream0 + b * stream_step
//   k_bm_add_mean          k_fm_add_mean for (position, vector, member)
//
// A product has no dependency chain, so a direction is TWO launches whatever the tree looks like and however
// many members the batch has.  Member b: L = arena0 + b * lstride, X / Y + b * wstride, scratch + b * sstride.
// A workgroup whose member is flagged (not positive definite) returns at once, before any barrier: the
// vectors of such a member are never touched.  No atomic add, no inline assembly.
//
// Grid: the member is the slow axis (blockIdx.y) by default, as in batch.hip: the workgroups of one member
// are consecutive and share its arena in L2.  member_fast = 1 (the experiment of DESIGN) makes the
// members of one work item consecutive on a linear grid.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>

#include "fm_body.hpp"
#include "kernels.hpp"
#include "sm_mm.hpp"

namespace spx {

template <bool T, int RB>
__global__ __launch_bounds__(256) void k_bm_strip(const BmultView v, const UpdTile* __restrict__ tiles,
                                                  const SolveUnit* __restrict__ units, const int* __restrict__ rlist,
                                                  const double* __restrict__ X, FmultView fv) {
  __shared__ double Xs[T ? kSolveStripRows : 1][RB + SM_PAD];
  int b;
  unsigned t;
  sm_member_split(v.member_fast, v.nbatch, b, t);
  if (v.flag[b] != INT_MAX) return;   // (before any barrier)
  fv.scratch += (int64_t)b * v.sstride;
  const UpdTile tl = tiles[t];
  fm_strip_body<T, RB>(tl, t, units[tl.unit], v.L + (int64_t)b * v.lstride, rlist, X + (int64_t)b * v.wstride, fv, Xs);
}

template <bool T, int RB>
__global__ __launch_bounds__(256) void k_bm_diag(const BmultView v, const UpdTile* __restrict__ chunks,
                                                 const SolveUnit* __restrict__ units, const double* __restrict__ X,
                                                 double* __restrict__ Y, FmultView fv) {
  __shared__ double Ts[T ? 1 : 64][RB + SM_PAD];
  int b;
  unsigned t;
  sm_member_split(v.member_fast, v.nbatch, b, t);
  if (v.flag[b] != INT_MAX) return;
  fv.scratch += (int64_t)b * v.sstride;
  const UpdTile ch = chunks[t];
  fm_diag_body<T, RB>(ch, units[ch.unit], v.L + (int64_t)b * v.lstride, X + (int64_t)b * v.wstride,
                      Y + (int64_t)b * v.wstride, fv, Ts);
}

// k_sm_pack of solve_many.hip for member blockIdx.y (sm_pack_body): 64 rows per workgroup
template <int RB, bool UNPACK>
__global__ __launch_bounds__(256) void k_bm_pack(const BmultView v, double* __restrict__ x, int64_t xstride, int64_t ldx,
                                                 const int* __restrict__ order, int n, int nv, double* __restrict__ W) {
  __shared__ double tile[64][RB + 1];
  const int b = blockIdx.y;
  if (v.flag[b] != INT_MAX) return;   // (before any barrier)
  sm_pack_body<RB, UNPACK>((int)blockIdx.x * 64, x + (int64_t)b * xstride, ldx, order, n, nv,
                           W + (int64_t)b * v.wstride, tile);
}

// grid: (positions / 256, samples, members).  member0: the first member of this launch in the batch.
__global__ __launch_bounds__(256) void k_bm_noise(const BmultView v, double* __restrict__ z, int64_t zstride, int64_t ldz,
                                                  const int* __restrict__ order, int n, uint64_t seed, uint64_t first,
                                                  uint32_t stream0, int stream_step, int member0) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int b = blockIdx.z;
  const int p = order ? order[i] : i;
  const uint32_t stream = stream0 + (uint32_t)(member0 + b) * (uint32_t)stream_step;
  z[(int64_t)b * zstride + (int64_t)blockIdx.y * ldz + i] =
      v.flag[b] != INT_MAX ? (double)NAN : fm_normal((uint32_t)p, stream, first + blockIdx.y, seed);
}

__global__ __launch_bounds__(256) void k_bm_add_mean(double* __restrict__ x, int64_t xstride, int64_t ldx,
                                                     const double* __restrict__ mean, int64_t ldmean, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) x[(int64_t)blockIdx.z * xstride + (int64_t)blockIdx.y * ldx + i] += mean[(int64_t)blockIdx.z * ldmean + i];
}

// ---------------------------------------------------------------------------
// launch wrappers
// ---------------------------------------------------------------------------
namespace {
// fn(view of the member range, first member) for every range of members: at most 65535 members (the y and z
// extents of a grid) and at most batch_grid_limit() workgroups per launch
template <class Fn>
int bm_ranges(const BmultView& v, int64_t per_member, Fn&& fn) {
  if (per_member <= 0 || v.nbatch <= 0) return 0;
  const int64_t fit = std::max<int64_t>(1, batch_grid_limit() / per_member);
  const int step = (int)std::min<int64_t>(std::min<int64_t>(v.nbatch, 65535), fit);
  int launches = 0;
  for (int b0 = 0; b0 < v.nbatch; b0 += step) {
    BmultView s = v;
    s.nbatch = std::min(step, v.nbatch - b0);
    s.L += (int64_t)b0 * v.lstride;
    s.flag += b0;
    fn(s, b0);
    ++launches;
  }
  return launches;
}

dim3 bm_grid(const BmultView& s, int64_t count) {
  return s.member_fast ? dim3((unsigned)(count * s.nbatch)) : dim3((unsigned)count, (unsigned)s.nbatch);
}

template <int RB>
int launch_bmult_rb(hipStream_t st, const BmultView& v, const SolveTablesView& t, int64_t ntiles, const UpdTile* chunks,
                    int64_t nchunks, bool transpose, const double* X, double* Y, const FmultView& fv) {
  const dim3 b(256);
  int launches = 0;
  launches += bm_ranges(v, ntiles, [&](const BmultView& s, int b0) {
    FmultView f = fv;
    f.scratch += (int64_t)b0 * v.sstride;
    const double* Xs = X + (int64_t)b0 * v.wstride;
    if (transpose)
      hipLaunchKernelGGL((k_bm_strip<true, RB>), bm_grid(s, ntiles), b, 0, st, s, t.tiles, t.units, t.rlist, Xs, f);
    else
      hipLaunchKernelGGL((k_bm_strip<false, RB>), bm_grid(s, ntiles), b, 0, st, s, t.tiles, t.units, t.rlist, Xs, f);
  });
  launches += bm_ranges(v, nchunks, [&](const BmultView& s, int b0) {
    FmultView f = fv;
    f.scratch += (int64_t)b0 * v.sstride;
    const double* Xs = X + (int64_t)b0 * v.wstride;
    double* Ys = Y + (int64_t)b0 * v.wstride;
    if (transpose)
      hipLaunchKernelGGL((k_bm_diag<true, RB>), bm_grid(s, nchunks), b, 0, st, s, chunks, t.units, Xs, Ys, f);
    else
      hipLaunchKernelGGL((k_bm_diag<false, RB>), bm_grid(s, nchunks), b, 0, st, s, chunks, t.units, Xs, Ys, f);
  });
  return launches;
}
}  // namespace

int launch_batch_mult(hipStream_t st, const BmultView& v, const SolveTablesView& t, int64_t ntiles, const UpdTile* chunks,
                      int64_t nchunks, bool transpose, const double* X, double* Y, int rb, const FmultView& fv) {
  if (nchunks <= 0) return 0;
  return rb == 32 ? launch_bmult_rb<32>(st, v, t, ntiles, chunks, nchunks, transpose, X, Y, fv)
                  : launch_bmult_rb<16>(st, v, t, ntiles, chunks, nchunks, transpose, X, Y, fv);
}

int launch_batch_mult_pack(hipStream_t st, const BmultView& v, bool unpack, double* x, int64_t xstride, int64_t ldx,
                           const int* order, int n, int nv, int rb, double* W) {
  if (n <= 0) return 0;
  const int64_t nblk = ((int64_t)n + 63) / 64;
  return bm_ranges(v, nblk, [&](const BmultView& s, int b0) {
    const dim3 g((unsigned)nblk, (unsigned)s.nbatch), b(256);
    double* xs = x + (int64_t)b0 * xstride;
    double* Ws = W + (int64_t)b0 * v.wstride;
    if (rb == 32) {
      if (unpack) hipLaunchKernelGGL((k_bm_pack<32, true>), g, b, 0, st, s, xs, xstride, ldx, order, n, nv, Ws);
      else hipLaunchKernelGGL((k_bm_pack<32, false>), g, b, 0, st, s, xs, xstride, ldx, order, n, nv, Ws);
    } else {
      if (unpack) hipLaunchKernelGGL((k_bm_pack<16, true>), g, b, 0, st, s, xs, xstride, ldx, order, n, nv, Ws);
      else hipLaunchKernelGGL((k_bm_pack<16, false>), g, b, 0, st, s, xs, xstride, ldx, order, n, nv, Ws);
    }
  });
}

int launch_batch_white_noise(hipStream_t st, const BmultView& v, double* z, int64_t zstride, int64_t ldz, const int* order,
                             int n, int nsamp, uint64_t seed, uint64_t first, uint32_t stream0, int stream_step) {
  if (n <= 0) return 0;
  const int64_t nblk = ((int64_t)n + 255) / 256;
  int launches = 0;
  for (int done = 0; done < nsamp; done += 32768) {   // (the y extent of a grid is 16 bits)
    const int cur = std::min(32768, nsamp - done);
    launches += bm_ranges(v, nblk * cur, [&](const BmultView& s, int b0) {
      hipLaunchKernelGGL(k_bm_noise, dim3((unsigned)nblk, (unsigned)cur, (unsigned)s.nbatch), dim3(256), 0, st, s,
                         z + (int64_t)b0 * zstride + (int64_t)done * ldz, zstride, ldz, order, n, seed,
                         first + (uint64_t)done, stream0, stream_step, b0);
    });
  }
  return launches;
}

int launch_batch_add_mean(hipStream_t st, const BmultView& v, double* x, int64_t xstride, int64_t ldx, const double* mean,
                          int64_t ldmean, int n, int nvec) {
  if (n <= 0) return 0;
  const int64_t nblk = ((int64_t)n + 255) / 256;
  int launches = 0;
  for (int done = 0; done < nvec; done += 32768) {
    const int cur = std::min(32768, nvec - done);
    launches += bm_ranges(v, nblk * cur, [&](const BmultView& s, int b0) {
      hipLaunchKernelGGL(k_bm_add_mean, dim3((unsigned)nblk, (unsigned)cur, (unsigned)s.nbatch), dim3(256), 0, st,
                         x + (int64_t)b0 * xstride + (int64_t)done * ldx, xstride, ldx, mean + (int64_t)b0 * ldmean, ldmean,
                         n);
    });
  }
  return launches;
}

}  // namespace spx
