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

#include "kernels.hpp"

namespace spx {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int FA_T = kSelinvTile;   // 64
constexpr int FA_LDA = 66;
constexpr int FA_LDB = 80;
constexpr int FA_NV = 32;           // vectors per pass of k_fadj_seed

// ---------------------------------------------------------------------------
// One workgroup per (block column, 64-row strip).  Thread t: column (t & 63) of the current 64-column
// chunk, rows (t >> 6) + 4 k.  Per entry ONE chain acc = fma(a_q[r], b_q[c], acc) over q ascending, whatever
// nvec is (the passes of FA_NV vectors keep their accumulators), alpha applied once at the end: a vector's
// contribution does not depend on nvec or on its place among the others.  a_q[r] comes from LDS as a
// same-address read of the wavefront, b_q[c] sits in registers, the stores run along the arena's rows.
// The strict upper triangle of a diagonal tile is not written.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_fadj_seed(const UpdTile* __restrict__ tiles, const FadjCol* __restrict__ cols,
                                                   const int* __restrict__ rlist, const int* __restrict__ porder,
                                                   double* __restrict__ G, int nvec, const double* __restrict__ a,
                                                   const double* __restrict__ b, int64_t ld, double alpha,
                                                   int accumulate, int a_pivot, int b_pivot) {
  __shared__ double As[FA_NV][FA_T];
  __shared__ int Ra[FA_T];
  const UpdTile tl = tiles[blockIdx.x];
  const FadjCol u = cols[tl.unit];
  const int tid = threadIdx.x, cl = tid & 63, rg = tid >> 6;
  const int r0 = tl.ti * FA_T;
  const int nr = min(FA_T, u.nrow - r0);
  if (tid < FA_T) {
    const int p = rlist[u.idx_off + r0 + min(tid, nr - 1)];
    Ra[tid] = a_pivot ? p : porder[p];
  }
  for (int c0 = 0; c0 < u.w; c0 += FA_T) {
    const int col = c0 + cl;
    const bool cin = col < u.w;
    const int pc = u.gcol0 + min(col, u.w - 1);
    const int jb = b_pivot ? pc : porder[pc];
    double acc[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) acc[k] = 0.0;
    for (int q0 = 0; q0 < nvec; q0 += FA_NV) {
      const int nq = min(FA_NV, nvec - q0);
      __syncthreads();   // (Ra written; the last pass read)
      for (int e = tid; e < FA_NV * FA_T; e += 256) {
        const int q = e >> 6, r = e & 63;
        As[q][r] = (q < nq && r < nr) ? a[(int64_t)(q0 + q) * ld + Ra[r]] : 0.0;
      }
      double bq[FA_NV];
#pragma unroll
      for (int q = 0; q < FA_NV; ++q) bq[q] = q < nq ? b[(int64_t)(q0 + q) * ld + jb] : 0.0;
      __syncthreads();
#pragma unroll
      for (int q = 0; q < FA_NV; ++q) {
        if (q < nq) {
#pragma unroll
          for (int k = 0; k < 16; ++k) acc[k] = fma(As[q][rg + 4 * k], bq[q], acc[k]);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int r = r0 + rg + 4 * k;   // row of the block column: r < w is pivot gcol0 + r
      if (rg + 4 * k < nr && cin && (r >= u.w || r >= col)) {
        double* g = G + u.off + (int64_t)r * u.w + col;
        const double v = alpha * acc[k];
        *g = accumulate ? *g + v : v;
      }
    }
  }
}

// acc[c] += A B for the wavefront's 16 rows arow .. arow + 15 and the column blocks c < ncb; K = 4 ks
__device__ __forceinline__ void fadj_mm4(const double (*At)[FA_LDA], int arow, const double (*Bt)[FA_LDB], int ks,
                                         int ncb, int lane, d4 (&acc)[4]) {
  const int g = lane >> 4, col = lane & 15;
  for (int s = 0; s < ks; ++s) {
    const double av = At[arow + col][4 * s + g];
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < ncb) acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, Bt[4 * s + g][16 * c + col], acc[c], 0, 0, 0);
  }
}

// ---------------------------------------------------------------------------
// one 64-row tile of R, 4 wavefronts; wavefront w owns rows 16 w .. 16 w + 15 of each product
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_fadj_scale(const UpdTile* __restrict__ tiles, const SelinvUnit* __restrict__ units,
                                                    const double* __restrict__ L, const double* __restrict__ dinv,
                                                    double* __restrict__ G, double* __restrict__ scratch) {
  __shared__ double At[FA_T][FA_LDA];   // T, then W^T
  __shared__ double Bt[FA_T][FA_LDB];   // inv(L_JJ), then the tile's rows of L_RJ
  const UpdTile t = tiles[blockIdx.x];
  const SelinvUnit u = units[t.unit];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int j = lane, g = lane >> 4, col = lane & 15;
  const int nR = u.nR, pn = u.pn;
  const int i0 = t.ti * FA_T;
  const int nr = min(FA_T, nR - i0);
  double* Grj = G + u.off + (int64_t)(u.c0 + pn + i0) * u.ld + u.c0;
  const double* Lrj = L + u.off + (int64_t)(u.c0 + pn + i0) * u.ld + u.c0;
  for (int q = 0; q < 16; ++q) {
    const int i = wv + 4 * q;
    double tv = 0.0, dv = 0.0;
    if (j < pn) {
      if (i < nr) {
        double y = 0.0;
        for (int s = 0; s < u.nsplit; ++s) y += scratch[u.y_off + ((int64_t)s * nR + i0 + i) * pn + j];
        tv = Grj[(int64_t)i * u.ld + j] - y;
      }
      if (i < pn && j <= i) dv = dinv[u.dinv_off + (int64_t)i * u.dinv_ld + j];
    }
    At[i][j] = tv;
    Bt[i][j] = dv;
  }
  __syncthreads();
  const int ncb = (pn + 15) >> 4;
  d4 acc[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) acc[c] = d4{0.0, 0.0, 0.0, 0.0};
  fadj_mm4(At, 16 * wv, Bt, (pn + 3) >> 2, ncb, lane, acc);   // W = T inv(L_JJ)
  __syncthreads();
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = 16 * wv + g + 4 * r, jj = 16 * c + col;
      const double w = acc[c][r];   // (0 outside nr x pn: T and inv(L_JJ) are zero there)
      if (i < nr && jj < pn) Grj[(int64_t)i * u.ld + jj] = w;
      At[jj][i] = w;
    }
  for (int q = 0; q < 16; ++q) {
    const int i = wv + 4 * q;
    Bt[i][j] = (i < nr && j < pn) ? Lrj[(int64_t)i * u.ld + j] : 0.0;
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < 4; ++c) acc[c] = d4{0.0, 0.0, 0.0, 0.0};
  fadj_mm4(At, 16 * wv, Bt, (nr + 3) >> 2, ncb, lane, acc);    // Q = W^T L_RJ over the tile's rows
  double* Q = scratch + u.p_off + (int64_t)t.ti * pn * pn;
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int a = 16 * wv + g + 4 * r, bb = 16 * c + col;
      if (a < pn && bb < pn) Q[a * pn + bb] = acc[c][r];
    }
}

// the wavefront's 16 x 16 block (bi, bj) of At Bt, K = 4 ks
__device__ __forceinline__ d4 fadj_mm1(const double (*At)[FA_LDA], const double (*Bt)[FA_LDB], int bi, int bj, int ks,
                                       int lane) {
  const int g = lane >> 4, col = lane & 15;
  d4 acc = d4{0.0, 0.0, 0.0, 0.0};
  for (int s = 0; s < ks; ++s)
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(At[16 * bi + col][4 * s + g], Bt[4 * s + g][16 * bj + col], acc, 0, 0, 0);
  return acc;
}

// ---------------------------------------------------------------------------
// one panel, 16 wavefronts: wavefront w owns the 16 x 16 block (w >> 2, w & 3) of each of the three products.
// L_JJ and G_JJ are masked to their lower triangles (the upper halves of the arenas are unspecified), the
// dinv slot as well; rows and columns past pn are zero in every operand.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_fadj_diag(const SelinvUnit* __restrict__ units, const double* __restrict__ L,
                                                    const double* __restrict__ dinv, double* __restrict__ G,
                                                    const double* __restrict__ scratch) {
  __shared__ double At[FA_T][FA_LDA];
  __shared__ double Bt[FA_T][FA_LDB];
  const SelinvUnit u = units[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int b = lane, g = lane >> 4, col = lane & 15;
  const int bi = wv >> 2, bj = wv & 3;
  const int pn = u.pn, ks = (pn + 3) >> 2;
  const double* Ljj = L + u.off + (int64_t)u.c0 * u.ld + u.c0;
  double* Gjj = G + u.off + (int64_t)u.c0 * u.ld + u.c0;
  double d[4];
  for (int q = 0; q < 4; ++q) {
    const int a = wv + 16 * q;
    double lv = 0.0, mv = 0.0;
    d[q] = 0.0;
    if (a < pn && b <= a) {
      lv = Ljj[(int64_t)a * u.ld + b];
      d[q] = dinv[u.dinv_off + (int64_t)a * u.dinv_ld + b];
      const double* p = scratch + u.p_off + (int64_t)a * pn + b;
      double s = 0.0;
#pragma unroll 8
      for (int ti = 0; ti < u.ntile; ++ti) s += p[(int64_t)ti * pn * pn];
      mv = Gjj[(int64_t)a * u.ld + b] - s;
    }
    At[b][a] = lv;   // L_JJ^T
    Bt[a][b] = mv;   // M
  }
  __syncthreads();
  d4 x = fadj_mm1(At, Bt, bi, bj, ks, lane);   // L_JJ^T M
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = 16 * bi + g + 4 * r, cc = 16 * bj + col;
    if (row >= cc) {   // sym(tril(.)): Phi + Phi^T
      At[row][cc] = x[r];
      At[cc][row] = x[r];
    }
  }
  for (int q = 0; q < 4; ++q) Bt[wv + 16 * q][b] = d[q];
  __syncthreads();
  x = fadj_mm1(At, Bt, bi, bj, ks, lane);      // (P + P^T) inv(L_JJ)
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) Bt[16 * bi + g + 4 * r][16 * bj + col] = x[r];
  for (int q = 0; q < 4; ++q) At[b][wv + 16 * q] = d[q];   // inv(L_JJ)^T
  __syncthreads();
  x = fadj_mm1(At, Bt, bi, bj, ks, lane);      // N
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = 16 * bi + g + 4 * r, cc = 16 * bj + col;
    if (row < pn && cc <= row) Gjj[(int64_t)row * u.ld + cc] = row == cc ? 0.5 * x[r] : x[r];
  }
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
