// Batched factorization and solve for gfx950: nbatch value sets on ONE sparsity pattern (schedule.hpp:
// the single-stream, unfused Program and the SolveProgram of the pattern, built once and shared by
// every member).  One launch of the program is one kernel launch for the whole batch: the grid is
// (work items of the launch) x (members), and a workgroup offsets L, dinv and the flag by the member
// strides and reads the SHARED tables.
//
//   k_batch_init          member arenas cleared, A_b copied in through the shared value map, flags INT_MAX
//   k_batch_chain         ChainUnit: Cholesky of a panel of order <= 64 in LDS + its inverse into the dinv slot
//   k_batch_update<T>     UpdTile / UpdUnit, T = 32 or 64: C (-)= A B^T on v_mfma_f64_16x16x4_f64,
//                         epilogues TRSM (store), DIRECT (subtract in place), SCATTER (atomic subtract)
//   k_batch_pack          caller's vectors <-> the pivot-order workspace Y[(b nrhs + q) n + p]
//   k_batch_solve_diag    SV_DIAG_FWD / SV_DIAG_BWD for one vector of one member per workgroup
//   k_batch_solve_strip_* SV_STRIP_FWD / SV_STRIP_BWD, 64 rows per workgroup
//   k_batch_log_det       out[b] = 2 sum_j log L_b[diag_pos[j]], in a fixed order
//
// No workgroup reads what another workgroup of the same launch writes; the only cross-workgroup
// traffic inside a launch are the atomic adds of the SCATTER epilogue and of the strips, and the
// atomicMin on a member's flag.  Ragged edges are masked: nothing is read outside the rows and columns
// a table entry names, so a member never touches its neighbour's arena.  The atomic adds are fp64
// atomics: two runs agree to rounding, not bit for bit (the default engine's reproducibility).
//
// MFMA lane map (header of kernels.hip): lane l supplies A[l&15][l>>4] and B[l>>4][l&15] and receives
// C[(l>>4) + 4 r][l&15] in register r.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>

#include "bu_body.hpp"
#include "kernels.hpp"

namespace spx {

// workgroup -> (member, work item).  member_fast = 0: the workgroups of one member are consecutive
// (they share that member's operands in L2); 1: the members of one work item are consecutive (they
// share the table entries and index lists).
__device__ __forceinline__ void batch_split(const BatchView& v, int64_t count, int members, int& b, int64_t& t) {
  // (a grid holds fewer than 2^24 workgroups, launch wrappers below: 32-bit division)
  const unsigned wg = blockIdx.x;
  if (v.member_fast) {
    b = (int)(wg % (unsigned)members);
    t = wg / (unsigned)members;
  } else {
    b = (int)(wg / (unsigned)count);
    t = wg % (unsigned)count;
  }
}

__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  return x;
}

// ---------------------------------------------------------------------------
// initialisation: one chunk of kInitChunk doubles of one member's arena per workgroup, built in LDS
// (zero + the entries of A that land in it: the value map bucketed by chunk, kernels.hpp) and stored once
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_batch_init(BatchView v, int64_t arena, int64_t nchunk,
                                                    const double* __restrict__ val, int64_t ldval,
                                                    const int64_t* __restrict__ cptr,
                                                    const unsigned short* __restrict__ loc,
                                                    const int* __restrict__ src) {
  __shared__ double buf[kInitChunk];
  int b;
  int64_t c;
  batch_split(v, nchunk, v.nbatch, b, c);
  const int tid = threadIdx.x;
  for (int e = tid; e < kInitChunk; e += 256) buf[e] = 0.0;
  __syncthreads();
  const double* vb = val + (int64_t)b * ldval;
  for (int64_t i = cptr[c] + tid; i < cptr[c + 1]; i += 256) buf[loc[i]] = vb[src[i]];
  __syncthreads();
  const int64_t base = c * kInitChunk;
  const int64_t len = arena - base < kInitChunk ? arena - base : kInitChunk;
  double* Lb = v.L + (int64_t)b * v.lstride + base;
  for (int e = tid; e < len; e += 256) Lb[e] = buf[e];
  if (c == 0 && tid == 0) v.flag[b] = INT_MAX;
}

// ---------------------------------------------------------------------------
// one panel of the chain per workgroup and member: A_pp = L_pp L_pp^T in LDS (right-looking, the columns
// stay unscaled until the end: step j subtracts a_ij a_kj / a_jj), then inv(L_pp) column by column.
// The slot gets the whole pn x pn inverse (zero above the diagonal), row stride ce - cs: the layout
// k_chain_potrf leaves (schedule.hpp winv_offset / winv_ld), which the solve reads.
// A pivot that is not positive and finite reports atomicMin(flag, its 1-based pivot position); the
// workgroup carries on with whatever values result.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_batch_chain(BatchView v, const ChainUnit* __restrict__ units, int64_t count) {
  __shared__ double A[64][65];
  __shared__ double Lm[64][65];
  int b;
  int64_t t;
  batch_split(v, count, v.nbatch, b, t);
  const ChainUnit u = units[t];
  const int tid = threadIdx.x;
  const int pn = u.pn, ld = u.ld;
  double* Lb = v.L + (int64_t)b * v.lstride + u.off + (int64_t)u.c0 * ld + u.c0;
  for (int e = tid; e < 64 * 64; e += 256) {
    const int i = e >> 6, j = e & 63;
    A[i][j] = (i < pn && j <= i) ? Lb[(int64_t)i * ld + j] : 0.0;
  }
  __syncthreads();
  const int k = tid & 63, iph = tid >> 6;
  for (int j = 0; j < pn; ++j) {
    const double d = A[j][j];
    if (tid == 0 && !(d > 0.0 && d < INFINITY)) atomicMin(v.flag + b, u.gcol + j + 1);
    const double rinv = 1.0 / d;
    if (k > j && k < pn) {
      const double akj = A[k][j];
      for (int i = ((j + 1) & ~3) + iph; i < pn; i += 4)
        if (i >= k) A[i][k] -= A[i][j] * rinv * akj;
    }
    __syncthreads();
  }
  for (int e = tid; e < 64 * 64; e += 256) {
    const int i = e >> 6, j = e & 63;
    if (i < pn && j <= i) {
      const double s = sqrt(A[j][j]);
      const double l = i == j ? s : A[i][j] / s;
      Lm[i][j] = l;
      Lb[(int64_t)i * ld + j] = l;
    }
  }
  __syncthreads();
  // inv(L_pp): thread c solves L x = e_c by forward substitution; x goes to A[.][c]
  if (tid < pn) {
    const int c = tid;
    for (int i = 0; i < c; ++i) A[i][c] = 0.0;
    for (int i = c; i < pn; ++i) {
      double s = i == c ? 1.0 : 0.0;
      for (int q = c; q < i; ++q) s -= Lm[i][q] * A[q][c];
      A[i][c] = s / Lm[i][i];
    }
  }
  __syncthreads();
  const int ldw = u.ce - u.cs, cq = u.c0 - u.cs;
  double* W = v.dinv + (int64_t)b * v.dstride + u.winv_off + cq;
  for (int e = tid; e < pn * pn; e += 256) {
    const int i = e / pn, j = e - i * pn;
    W[(int64_t)i * ldw + j] = A[i][j];
  }
}

// ---------------------------------------------------------------------------
// one tile (T x T, T = 32 or 64) of one update unit per workgroup and member:
//   P = sum_seg A_seg B_seg^T  over the unit's K segments (tests/emulate.py reads them the same way),
// operands staged through LDS in chunks of 32 columns of K, products on the fp64 matrix cores.
// T = 64: wavefront v owns rows 16 v .. 16 v + 15 and all four 16-column blocks; T = 32: wavefront v
// owns the 16 x 16 block (v >> 1, v & 1).
// ---------------------------------------------------------------------------
template <int T>
__global__ __launch_bounds__(256) void k_batch_update(BatchView v, const UpdTile* __restrict__ tiles, int64_t count,
                                                      const UpdUnit* __restrict__ units,
                                                      const int64_t* __restrict__ bc_off, const int* __restrict__ bc_w,
                                                      const int* __restrict__ relpos, const int* __restrict__ rlist) {
  constexpr int NC = T == 64 ? 4 : 1;
  __shared__ double As[T][BU_LD];
  __shared__ double Bs[T][BU_LD];
  int b;
  int64_t t;
  batch_split(v, count, v.nbatch, b, t);
  const UpdTile tl = tiles[t];
  const UpdUnit u = units[tl.unit];
  double* Lb = v.L + (int64_t)b * v.lstride;
  const double* Db = v.dinv + (int64_t)b * v.dstride;
  const int i0 = tl.ti * T, j0 = tl.tj * T;
  const int mi = min(T, u.M - i0), nj = min(T, u.N - j0);
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int g = lane >> 4, col = lane & 15;
  const int rb = T == 64 ? wv : (wv >> 1), cb0 = T == 64 ? 0 : (wv & 1);
  d4 acc[NC];
  bu_product<T>(u, i0, j0, mi, nj, Lb, Db, bc_off, bc_w, As, Bs, acc);
  // (every read of the tile's operands lies before the last barrier: the TRSM epilogue may overwrite them)
  double* D = Lb + u.d_off;
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
      if (u.mode == MODE_DIRECT) {
        D[(int64_t)(u.d_row0 + i) * u.d_ld + u.d_col0 + j] -= p;
      } else {
        const int dr = relpos[u.relrow_off + i] - u.d_row0;
        const int dc = rlist[u.gcol_off + j] - u.d_col0;
        unsafeAtomicAdd(D + (int64_t)dr * u.d_ld + dc, -p);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// solve.  Workspace Y[(b nrhs + q) n + p]: vector q of member b in pivot order.  A member whose flag is
// set is skipped by every kernel, pack and unpack included: its vectors stay as they were.
// ---------------------------------------------------------------------------
template <bool UNPACK>
__global__ __launch_bounds__(256) void k_batch_pack(BatchView v, double* __restrict__ x, int64_t ldx, int nrhs,
                                                    const int* __restrict__ order, int n, int64_t nblk,
                                                    double* __restrict__ Y) {
  int vec;
  int64_t blk;
  batch_split(v, nblk, v.nbatch * nrhs, vec, blk);
  if (v.flag[vec / nrhs] != INT_MAX) return;
  const int64_t i = blk * 256 + threadIdx.x;
  if (i >= n) return;
  const int p = order ? order[i] : (int)i;
  if (UNPACK) x[(int64_t)vec * ldx + i] = Y[(int64_t)vec * n + p];
  else Y[(int64_t)vec * n + p] = x[(int64_t)vec * ldx + i];
}

// diagonal tile of one block column, one vector: panel by panel (64 columns, the dinv slots of the batch
// program: slot p at dinv_off + 4096 p, row stride = the panel's width)
//   forward   x_p = inv(L_pp)   (y_p - L_p,<p x_<p)
//   backward  x_p = inv(L_pp)^T (y_p - L_>p,p^T x_>p)
template <bool BWD>
__global__ __launch_bounds__(256) void k_batch_solve_diag(BatchView v, const int* __restrict__ list, int64_t count,
                                                          const SolveUnit* __restrict__ units, int nrhs, int n,
                                                          double* __restrict__ Y) {
  __shared__ double xs[1024];
  __shared__ double ts[64];
  __shared__ double red[4][64];
  int vec;
  int64_t t;
  batch_split(v, count, v.nbatch * nrhs, vec, t);
  const int b = vec / nrhs;
  if (v.flag[b] != INT_MAX) return;
  const SolveUnit u = units[list[t]];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int w = u.w;
  const double* A = v.L + (int64_t)b * v.lstride + u.off;
  const double* Dall = v.dinv + (int64_t)b * v.dstride + u.dinv_off;
  double* y = Y + (int64_t)vec * n + u.gcol0;
  for (int q = tid; q < w; q += 256) xs[q] = y[q];
  __syncthreads();
  const int np = (w + 63) / 64;
  for (int pp = 0; pp < np; ++pp) {
    const int p = BWD ? np - 1 - pp : pp;
    const int c0 = p * 64, pn = min(64, w - c0);
    const double* D = Dall + (int64_t)p * 4096;
    if (!BWD) {
      for (int r = wv; r < pn; r += 4) {
        const double* arow = A + (int64_t)(c0 + r) * w;
        double s = 0.0;
        for (int q = lane; q < c0; q += 64) s += arow[q] * xs[q];
        s = wave_sum(s);
        if (lane == 0) ts[r] = xs[c0 + r] - s;
      }
      __syncthreads();
      for (int r = wv; r < pn; r += 4) {
        const double s = wave_sum(lane <= r ? D[(int64_t)r * pn + lane] * ts[lane] : 0.0);
        if (lane == 0) xs[c0 + r] = s;
      }
      __syncthreads();
    } else {
      double s = 0.0;
      if (lane < pn)
        for (int q = c0 + pn + wv; q < w; q += 4) s += A[(int64_t)q * w + c0 + lane] * xs[q];
      red[wv][lane] = s;
      __syncthreads();
      if (tid < pn) ts[tid] = xs[c0 + tid] - (red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid]);
      __syncthreads();
      s = 0.0;
      if (lane < pn)
        for (int q = lane + ((wv - lane) & 3); q < pn; q += 4) s += D[(int64_t)q * pn + lane] * ts[q];
      red[wv][lane] = s;
      __syncthreads();
      if (tid < pn) xs[c0 + tid] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
      __syncthreads();
    }
  }
  for (int q = tid; q < w; q += 256) y[q] = xs[q];
}

// forward: y[idx[r]] -= L[r, :] x_J for a strip of kSolveStripRows rows below the diagonal tile
__global__ __launch_bounds__(256) void k_batch_solve_strip_fwd(BatchView v, const UpdTile* __restrict__ tiles,
                                                               int64_t count, const SolveUnit* __restrict__ units,
                                                               const int* __restrict__ rlist, int nrhs, int n,
                                                               double* __restrict__ Y) {
  __shared__ double xs[1024];
  int vec;
  int64_t t;
  batch_split(v, count, v.nbatch * nrhs, vec, t);
  const int b = vec / nrhs;
  if (v.flag[b] != INT_MAX) return;
  const SolveUnit u = units[tiles[t].unit];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int w = u.w;
  const int r0 = w + tiles[t].ti * kSolveStripRows;
  const int nr = min(kSolveStripRows, u.nrow - r0);
  double* Yv = Y + (int64_t)vec * n;
  for (int q = tid; q < w; q += 256) xs[q] = Yv[u.gcol0 + q];
  __syncthreads();
  const double* A = v.L + (int64_t)b * v.lstride + u.off + (int64_t)r0 * w;
  const int* idx = rlist + u.idx_off + r0;
  for (int r = wv; r < nr; r += 4) {
    double s = 0.0;
    for (int q = lane; q < w; q += 64) s += A[(int64_t)r * w + q] * xs[q];
    s = wave_sum(s);
    if (lane == 0) unsafeAtomicAdd(Yv + idx[r], -s);
  }
}

// backward: y[gcol0 + k] -= sum_r L[r][k] x[idx[r]] for the strip's rows
__global__ __launch_bounds__(256) void k_batch_solve_strip_bwd(BatchView v, const UpdTile* __restrict__ tiles,
                                                               int64_t count, const SolveUnit* __restrict__ units,
                                                               const int* __restrict__ rlist, int nrhs, int n,
                                                               double* __restrict__ Y) {
  __shared__ double xr[kSolveStripRows];
  int vec;
  int64_t t;
  batch_split(v, count, v.nbatch * nrhs, vec, t);
  const int b = vec / nrhs;
  if (v.flag[b] != INT_MAX) return;
  const SolveUnit u = units[tiles[t].unit];
  const int tid = threadIdx.x;
  const int w = u.w;
  const int r0 = w + tiles[t].ti * kSolveStripRows;
  const int nr = min(kSolveStripRows, u.nrow - r0);
  double* Yv = Y + (int64_t)vec * n;
  const int* idx = rlist + u.idx_off + r0;
  if (tid < nr) xr[tid] = Yv[idx[tid]];
  __syncthreads();
  const double* A = v.L + (int64_t)b * v.lstride + u.off + (int64_t)r0 * w;
  for (int q = tid; q < w; q += 256) {
    double s = 0.0;
    for (int r = 0; r < nr; ++r) s += A[(int64_t)r * w + q] * xr[r];
    unsafeAtomicAdd(Yv + u.gcol0 + q, -s);
  }
}

// out[b] = 2 sum_j log L_b[diag_pos[j]] (NaN for a member whose flag is set): thread t sums j = t, t + 256,
// ..., the 256 partial sums are added pairwise in LDS -- the same order every time
__global__ __launch_bounds__(256) void k_batch_log_det(BatchView v, const int64_t* __restrict__ diag_pos, int n,
                                                       double* __restrict__ out) {
  __shared__ double part[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const double* Lb = v.L + (int64_t)b * v.lstride;
  double s = 0.0;
  for (int j = tid; j < n; j += 256) s += log(Lb[diag_pos[j]]);
  part[tid] = s;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) part[tid] += part[tid + h];
    __syncthreads();
  }
  if (tid == 0) out[b] = v.flag[b] != INT_MAX ? NAN : 2.0 * part[0];
}

// ---------------------------------------------------------------------------
// launch wrappers.  One kernel launch per call as long as (work items) x (members) fits a grid; beyond
// that the members are split into ranges.  Every wrapper returns the number of kernel launches it made
// (-1, and launches nothing, when the work items of ONE member already exceed a grid).
// ---------------------------------------------------------------------------
namespace {
// a launch holds at most 2^32 - 1 work-items (the dispatch packet's grid size), i.e. this many workgroups of 256
constexpr int64_t kGridMax = 4294967295LL / 256;
int64_t g_grid_limit = kGridMax;   // (test hook: set_batch_grid_limit lowers the point at which members are split)
// fn(view of the member range, first member) for every range whose grid fits; -1: one member alone does not fit
template <class Fn>
int for_member_ranges(const BatchView& v, int64_t per_member, int group, Fn&& fn) {
  if (per_member <= 0 || v.nbatch <= 0) return 0;
  const int64_t per = per_member * group;           // (group: vectors per member in the solve)
  if (per > kGridMax) return -1;
  const int step = (int)std::max<int64_t>(1, std::min<int64_t>(v.nbatch, g_grid_limit / per));
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
}  // namespace

void set_batch_grid_limit(int64_t workgroups) {
  g_grid_limit = workgroups > 0 ? std::min(workgroups, kGridMax) : kGridMax;
}

int64_t batch_grid_limit() { return g_grid_limit; }
int64_t batch_grid_limit_max() { return kGridMax; }

int launch_batch_init(hipStream_t st, const BatchView& v, int64_t arena, const double* val, int64_t ldval,
                      const int64_t* cptr, const unsigned short* loc, const int* src) {
  const int64_t nchunk = std::max<int64_t>(1, (arena + kInitChunk - 1) / kInitChunk);
  return for_member_ranges(v, nchunk, 1, [&](const BatchView& s, int b0) {
    hipLaunchKernelGGL(k_batch_init, dim3((unsigned)(nchunk * s.nbatch)), dim3(256), 0, st, s, arena, nchunk,
                       val + (int64_t)b0 * ldval, ldval, cptr, loc, src);
  });
}

int launch_batch_chain(hipStream_t st, const BatchView& v, const ChainUnit* units, int64_t count) {
  return for_member_ranges(v, count, 1, [&](const BatchView& s, int) {
    hipLaunchKernelGGL(k_batch_chain, dim3((unsigned)(count * s.nbatch)), dim3(256), 0, st, s, units, count);
  });
}

int launch_batch_update(hipStream_t st, const BatchView& v, int tile, const UpdTile* tiles, int64_t count,
                        const UpdUnit* units, const int64_t* bc_off, const int* bc_w, const int* relpos,
                        const int* rlist) {
  return for_member_ranges(v, count, 1, [&](const BatchView& s, int) {
    const dim3 g((unsigned)(count * s.nbatch)), b(256);
    if (tile == 64)
      hipLaunchKernelGGL(k_batch_update<64>, g, b, 0, st, s, tiles, count, units, bc_off, bc_w, relpos, rlist);
    else
      hipLaunchKernelGGL(k_batch_update<32>, g, b, 0, st, s, tiles, count, units, bc_off, bc_w, relpos, rlist);
  });
}

int launch_batch_pack(hipStream_t st, const BatchView& v, bool unpack, double* x, int64_t ldx, int nrhs,
                      const int* order, int n, double* Y) {
  const int64_t nblk = ((int64_t)n + 255) / 256;
  return for_member_ranges(v, nblk, nrhs, [&](const BatchView& s, int b0) {
    const dim3 g((unsigned)(nblk * s.nbatch * nrhs)), b(256);
    double* xs = x + (int64_t)b0 * nrhs * ldx;
    double* Ys = Y + (int64_t)b0 * nrhs * n;
    if (unpack) hipLaunchKernelGGL(k_batch_pack<true>, g, b, 0, st, s, xs, ldx, nrhs, order, n, nblk, Ys);
    else hipLaunchKernelGGL(k_batch_pack<false>, g, b, 0, st, s, xs, ldx, nrhs, order, n, nblk, Ys);
  });
}

int launch_batch_solve(hipStream_t st, const BatchView& v, int kind, const int* list, const UpdTile* tiles,
                       int64_t first, int64_t count, const SolveUnit* units, const int* rlist, double* Y, int nrhs,
                       int n) {
  return for_member_ranges(v, count, nrhs, [&](const BatchView& s, int b0) {
    const dim3 g((unsigned)(count * s.nbatch * nrhs)), b(256);
    double* Ys = Y + (int64_t)b0 * nrhs * n;
    switch (kind) {
      case SV_DIAG_FWD:
        hipLaunchKernelGGL(k_batch_solve_diag<false>, g, b, 0, st, s, list + first, count, units, nrhs, n, Ys);
        break;
      case SV_DIAG_BWD:
        hipLaunchKernelGGL(k_batch_solve_diag<true>, g, b, 0, st, s, list + first, count, units, nrhs, n, Ys);
        break;
      case SV_STRIP_FWD:
        hipLaunchKernelGGL(k_batch_solve_strip_fwd, g, b, 0, st, s, tiles + first, count, units, rlist, nrhs, n, Ys);
        break;
      default:
        hipLaunchKernelGGL(k_batch_solve_strip_bwd, g, b, 0, st, s, tiles + first, count, units, rlist, nrhs, n, Ys);
        break;
    }
  });
}

int launch_batch_log_det(hipStream_t st, const BatchView& v, const int64_t* diag_pos, int n, double* out) {
  if (v.nbatch <= 0) return 0;
  hipLaunchKernelGGL(k_batch_log_det, dim3((unsigned)v.nbatch), dim3(256), 0, st, v, diag_pos, n, out);
  return 1;
}

}  // namespace spx
