// The product loop of the batched update kernels (batch.hip: k_batch_update, epilogues TRSM / DIRECT / SCATTER;
// batch_repro.hip: k_bdet_update, epilogues TRSM / DIRECT / BUFFER).  One tile (T x T, T = 32 or 64) of one update
// unit of one member per workgroup:
//   P = sum_seg A_seg B_seg^T  over the unit's K segments (tests/emulate.py reads them the same way),
// operands staged through LDS in chunks of 32 columns of K, products on the fp64 matrix cores.
// T = 64: wavefront v owns rows 16 v .. 16 v + 15 and all four 16-column blocks; T = 32: wavefront v
// owns the 16 x 16 block (v >> 1, v & 1).  The sum over K runs in an order fixed by the unit alone.  No atomic
// add in this header.
//
// MFMA lane map (header of kernels.hip): lane l supplies A[l&15][l>>4] and B[l>>4][l&15] and receives
// C[(l>>4) + 4 r][l&15] in register r.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.hpp"

namespace spx {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int BU_KC = 32;   // columns of K per LDS step
constexpr int BU_LD = 34;   // LDS row stride in doubles: the 16 rows x 2 k that one 32-lane half reads in a
                            // ds_read_b64 fall on banks 4 row + 2 k (mod 64 dwords), all distinct

// acc[c][r] = P[16 rb + (lane >> 4) + 4 r][16 (cb0 + c) + (lane & 15)] of the tile at (i0, j0) with mi x nj entries
// inside the unit; every read of the tile's operands lies before the last barrier
template <int T>
__device__ __forceinline__ void bu_product(const UpdUnit& u, int i0, int j0, int mi, int nj, const double* Lb,
                                           const double* Db, const int64_t* __restrict__ bc_off,
                                           const int* __restrict__ bc_w, double (*As)[BU_LD], double (*Bs)[BU_LD],
                                           d4 (&acc)[T == 64 ? 4 : 1]) {
  constexpr int NC = T == 64 ? 4 : 1;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int g = lane >> 4, col = lane & 15;
  const int rb = T == 64 ? wv : (wv >> 1), cb0 = T == 64 ? 0 : (wv & 1);
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[c] = d4{0.0, 0.0, 0.0, 0.0};
  for (int sg = 0; sg < u.nseg; ++sg) {
    const int abc = u.src_bcol0 + sg;
    const int aw = bc_w[abc];
    const int kbeg = u.nseg == 1 ? u.k0 : 0;
    const int klen = (u.nseg == 1 && u.klen >= 0) ? u.klen : aw;
    const double* Ap = Lb + bc_off[abc] + (int64_t)(u.src_r0 + i0 - (u.seg_r0 + sg * u.seg_stride)) * aw + kbeg;
    const double* Bp;
    int bw;
    if (u.mode == MODE_TRSM) {
      // B = rows j0 .. of the inverted panel (N x dinv_ld in the dinv scratch), K = dinv_ld
      bw = u.dinv_ld;
      Bp = Db + u.dinv_off + (int64_t)j0 * bw;
    } else {
      const int bbc = (u.b_bcol0 >= 0 ? u.b_bcol0 : u.src_bcol0) + sg;
      const int bsh = (u.b_bcol0 >= 0 ? u.b_seg_r0 : u.seg_r0) + sg * u.seg_stride;
      bw = bc_w[bbc];
      Bp = Lb + bc_off[bbc] + (int64_t)(u.src_c0 + j0 - bsh) * bw + kbeg;
    }
    for (int kc = 0; kc < klen; kc += BU_KC) {
      for (int e = tid; e < T * BU_KC; e += 256) {
        const int r = e / BU_KC, kk = e % BU_KC;
        const bool kin = kc + kk < klen;
        As[r][kk] = (kin && r < mi) ? Ap[(int64_t)r * aw + kc + kk] : 0.0;
        Bs[r][kk] = (kin && r < nj) ? Bp[(int64_t)r * bw + kc + kk] : 0.0;
      }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < BU_KC / 4; ++q) {
        const double a = As[16 * rb + col][4 * q + g];
#pragma unroll
        for (int c = 0; c < NC; ++c)
          acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Bs[16 * (cb0 + c) + col][4 * q + g], acc[c], 0, 0, 0);
      }
      __syncthreads();
    }
  }
}

}  // namespace spx
