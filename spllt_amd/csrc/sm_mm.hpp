// The fp64 matrix-core product of the blocked kernels (solve_many.hip, factor_mult.hip): a 16-row tile of A
// times rows of a workspace W[p * RB + q] (or an LDS image of such rows) on v_mfma_f64_16x16x4_f64.
// Lane l of a wavefront supplies A[l&15][l>>4] and B[l>>4][l&15] and receives C[(l>>4) + 4 r][l&15] in
// register r.  Column q of the result depends on column q of B alone, and its sum runs over k in an order
// that depends on K only: not on RB, and not on the column's place in the block.
// Also what every blocked translation unit needs besides (solve_many.hip, batch_solve_many.hip, batch_mult.hip; no
// atomic add in this header): the pack / unpack of a block of vectors, the workgroup -> (member, work item) split.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace spx {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int SM_PAD = 16;   // LDS row stride RB + 16 doubles: the four k rows of an MFMA step fall into two bank halves

// acc[c] += sum_{k0 <= k < k0 + 16 U} a(k) * B[k][16 c + (l&15)]: every load of the chunk is requested
// before the first product (a chunk is ONE round trip to memory)
template <int RB, int U>
__device__ __forceinline__ void sm_mm_chunk(const double* arow, int64_t sa, int k0, const double* Bp, int ldb,
                                            int g, int col, d4 (&acc)[RB / 16]) {
  constexpr int NC = RB / 16;
  double a[4 * U], b[4 * U][NC];
#pragma unroll
  for (int j = 0; j < 4 * U; ++j) {
    const int k = k0 + 4 * j + g;
    a[j] = arow[(int64_t)k * sa];
#pragma unroll
    for (int c = 0; c < NC; ++c) b[j][c] = Bp[(int64_t)k * ldb + 16 * c + col];
  }
#pragma unroll
  for (int j = 0; j < 4 * U; ++j)
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[j], b[j][c], acc[c], 0, 0, 0);
}

// acc[c] += sum_{k < K} a(k) * B[k][16 c + (l&15)], a(k) = arow[k * sa]: the lane's row of a row-major A
// (sa = 1) or its column (sa = lda).  B row k at Bp + k * ldb (rows of W, or an LDS image).  K need
// not be a multiple of 4: what lies behind it is neither used nor read.  The sweeps are bound by
// dependent round trips to memory, not by bandwidth: 64 columns of K per trip.
template <int RB>
__device__ __forceinline__ void sm_mm(const double* arow, int64_t sa, int K, const double* Bp, int ldb,
                                      int lane, d4 (&acc)[RB / 16]) {
  constexpr int NC = RB / 16;
  const int g = lane >> 4, col = lane & 15;
  int k0 = 0;
  for (; k0 + 64 <= K; k0 += 64) sm_mm_chunk<RB, 4>(arow, sa, k0, Bp, ldb, g, col, acc);
  for (; k0 + 16 <= K; k0 += 16) sm_mm_chunk<RB, 1>(arow, sa, k0, Bp, ldb, g, col, acc);
  for (; k0 < K; k0 += 4) {
    const int k = k0 + g;
    const int kc = min(k, K - 1);
    const double av = arow[(int64_t)kc * sa];
    const double a = k < K ? av : 0.0;
#pragma unroll
    for (int c = 0; c < NC; ++c)
      acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Bp[(int64_t)kc * ldb + 16 * c + col], acc[c], 0, 0, 0);
  }
}

// ---------------------------------------------------------------------------
// pack: W[p(i) * RB + q] = q < nv ? x[q * ldx + i] : 0,  p(i) = order[i] (user order) or i (order = null)
// unpack: x[q * ldx + i] = W[p(i) * RB + q] for q < nv only.  Rows i0 .. i0 + 63, transposed through `tile`.
// ---------------------------------------------------------------------------
template <int RB, bool UNPACK>
__device__ __forceinline__ void sm_pack_body(int i0, double* __restrict__ x, int64_t ldx, const int* __restrict__ order,
                                             int n, int nv, double* __restrict__ W, double (*tile)[RB + 1]) {
  const int tid = threadIdx.x;
  if (!UNPACK) {
    for (int e = tid; e < 64 * RB; e += 256) {
      const int ii = e & 63, q = e >> 6, i = i0 + ii;
      tile[ii][q] = (i < n && q < nv) ? x[(int64_t)q * ldx + i] : 0.0;
    }
    __syncthreads();
    for (int e = tid; e < 64 * RB; e += 256) {
      const int q = e % RB, ii = e / RB, i = i0 + ii;
      if (i < n) W[(int64_t)(order ? order[i] : i) * RB + q] = tile[ii][q];
    }
  } else {
    for (int e = tid; e < 64 * RB; e += 256) {
      const int q = e % RB, ii = e / RB, i = i0 + ii;
      if (i < n) tile[ii][q] = W[(int64_t)(order ? order[i] : i) * RB + q];
    }
    __syncthreads();
    for (int e = tid; e < 64 * RB; e += 256) {
      const int ii = e & 63, q = e >> 6, i = i0 + ii;
      if (i < n && q < nv) x[(int64_t)q * ldx + i] = tile[ii][q];
    }
  }
}

// workgroup -> (member b, work item t) of a batched launch over nbatch members: the member is the slow grid axis
// (blockIdx.y), or with member_fast the fast index of a linear grid
__device__ __forceinline__ void sm_member_split(int member_fast, int nbatch, int& b, unsigned& t) {
  if (member_fast) {
    b = (int)(blockIdx.x % (unsigned)nbatch);
    t = blockIdx.x / (unsigned)nbatch;
  } else {
    b = (int)blockIdx.y;
    t = blockIdx.x;
  }
}

}  // namespace spx
