// Device bodies of the sparse right-hand-side kernels, shared by solve_sparse.hip (one factor) and
// batch_solve_sparse.hip (every member of a batch), as sm_body.hpp is for the blocked sweeps: the kernels of the two
// files differ only in where a workgroup's workspace, values, output and partial buffer lie.  No atomics.
//
// MFMA operands as in solve_many.hip: lane l supplies A[l&15][l>>4] and B[l>>4][l&15] and receives
// C[(l>>4) + 4 r][l&15] in register r.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace spx {

typedef double ss_d2 __attribute__((ext_vector_type(2)));
typedef double ss_d4 __attribute__((ext_vector_type(4)));

// rows [first, first + len) of W: RB contiguous doubles per row, a multiple of 128 bytes from a 256-byte aligned
// base, cleared with 16-byte stores
template <int RB>
__device__ __forceinline__ void ss_zero_body(int first, int len, double* __restrict__ W) {
  ss_d2* p = reinterpret_cast<ss_d2*>(W + (int64_t)first * RB);
  const int total = len * (RB / 2);
  for (int i = threadIdx.x; i < total; i += 256) p[i] = ss_d2{0.0, 0.0};
}

// 64 wanted entries (t0 ..) per workgroup; only rows named by pos are read
template <int RB>
__device__ __forceinline__ void ss_gather_body(int64_t t0, double* __restrict__ x, int64_t ldx,
                                               const int* __restrict__ pos, int64_t nsel, int nv,
                                               const double* __restrict__ W, double (*tile)[RB + 1]) {
  const int tid = threadIdx.x;
  for (int e = tid; e < 64 * RB; e += 256) {
    const int q = e % RB, tt = e / RB;
    if (t0 + tt < nsel) tile[tt][q] = W[(int64_t)pos[t0 + tt] * RB + q];
  }
  __syncthreads();
  for (int e = tid; e < 64 * RB; e += 256) {
    const int tt = e & 63, q = e >> 6;
    if (t0 + tt < nsel && q < nv) x[(int64_t)q * ldx + t0 + tt] = tile[tt][q];
  }
}

// out[i][j] = sum over the rows p of [first, first + len) of WI[p * rbI + i] * WJ[p * rbJ + j], i, j < 32 (tiles of
// 16 behind rbI / rbJ stay zero).  Wavefront v takes the MFMA steps v, v + 4, ... of the chunk (4 rows each); the
// four partial products are added in wavefront order through LDS.  The last step of a chunk whose length is no
// multiple of 4 is padded with zeros: a row behind the chunk's end is never read.
__device__ __forceinline__ void ss_gram_body(int first, int len, const double* __restrict__ WI, int rbI,
                                             const double* __restrict__ WJ, int rbJ, double* __restrict__ out,
                                             double (*red)[32][33]) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int g = lane >> 4, col = lane & 15;
  const int nI = rbI / 16, nJ = rbJ / 16;
  ss_d4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = ss_d4{0.0, 0.0, 0.0, 0.0};
  const int nstep = (len + 3) / 4;
  for (int s = wv; s < nstep; s += 4) {
    const int k = 4 * s + g;
    const bool ok = k < len;
    const int64_t p = first + min(k, len - 1);
    double av[2], bv[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      av[t] = (ok && t < nI) ? WI[p * rbI + 16 * t + col] : 0.0;
      bv[t] = (ok && t < nJ) ? WJ[p * rbJ + 16 * t + col] : 0.0;
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
        if (a < nI && b < nJ) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[a], bv[b], acc[a][b], 0, 0, 0);
  }
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[wv][16 * a + g + 4 * r][16 * b + col] = acc[a][b][r];
  __syncthreads();
  for (int e = tid; e < 1024; e += 256) {
    const int i = e >> 5, j = e & 31;
    out[e] = ((red[0][i][j] + red[1][i][j]) + red[2][i][j]) + red[3][i][j];
  }
}

// G_IJ[i][j] (rows of group I, columns of group J, column-major with ldg) = the sum of the nchunk blocks in
// ascending order, and the same number to G_JI[j][i]; diag: I = J, the lower triangle is computed and mirrored
__device__ __forceinline__ void ss_gram_reduce_body(const double* __restrict__ part, int nchunk, int nvI, int nvJ,
                                                    int diag, double* __restrict__ Gij, double* __restrict__ Gji,
                                                    int64_t ldg) {
  for (int e = threadIdx.x; e < 1024; e += 256) {
    const int i = e >> 5, j = e & 31;
    if (i >= nvI || j >= nvJ || (diag && i < j)) continue;
    double s = 0.0;
    for (int c = 0; c < nchunk; ++c) s += part[(int64_t)c * 1024 + e];
    Gij[(int64_t)j * ldg + i] = s;
    Gji[(int64_t)i * ldg + j] = s;
  }
}

}  // namespace spx
