// Device code shared by the substitution kernels of kernels.hip and solve_repro.hip: the 16-lane dot
// products and the solve with the diagonal tile of one block column.  Included by HIP translation units only.
#pragma once
#include <hip/hip_runtime.h>

#include "schedule.hpp"

namespace spx {

// 16 lanes per row: partial dot products of row[0..len) with NR vectors
// x[q * XS + 0..len) for this lane's residues (k = sub, sub+16, ...), sixteen
// independent loads in flight; every loaded entry of L serves all NR right-hand sides
template <int NR, int XS>
__device__ inline void dot16(const double* __restrict__ row, const double* x, int len, int sub,
                             double (&out)[NR]) {
#pragma unroll
  for (int q = 0; q < NR; ++q) out[q] = 0.0;
  for (int k0 = 0; k0 < len; k0 += 256) {
    double v[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) v[e] = row[min(k0 + sub + 16 * e, len - 1)];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int k = k0 + sub + 16 * e;
      const double a = k < len ? v[e] : 0.0;
      const int kc = min(k, len - 1);
#pragma unroll
      for (int q = 0; q < NR; ++q) out[q] = __builtin_fma(a, x[q * XS + kc], out[q]);
    }
  }
}
__device__ inline double sum16(double v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 16);
  return v;
}

constexpr int kXS = 1024;  // LDS stride between right-hand sides (block column width <= 1024)

// Solve with the diagonal tile of one block column per workgroup, using the
// inverted 64x64 diagonal panels:  forward  x_p = inv(L_pp) (y_p - L_p,<p x_<p),
// backward x_p = inv(L_pp)^T (y_p - L_>p,p^T x_>p).  NR right-hand sides at once
// (y[q * ldy + i]).
// (the body of k_solve_diag; fill(xb, stride) puts the right-hand sides of the block column's own rows into
// xb[q * stride + j] -- the plain kernel copies y, the reproducible one subtracts the stored strip products)
template <bool BWD, int NR, class Fill>
__device__ __forceinline__ void solve_diag_body(const SolveUnit& u, const double* __restrict__ L,
                                                const double* __restrict__ dinv, double* __restrict__ y,
                                                int64_t ldy, Fill fill) {
  __shared__ double xb[NR * kXS];
  __shared__ double tb[NR * 64];
  __shared__ double part[4][NR * 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int sub = tid & 15, rr = tid >> 4;   // 16 lanes per row, 16 rows per pass
  const int w = u.w, pw = u.pw;
  const double* A = L + u.off;
  fill(xb, kXS);
  __syncthreads();
  const int np = (w + pw - 1) / pw;
  for (int pp = 0; pp < np; ++pp) {
    const int p = BWD ? np - 1 - pp : pp;
    const int c0 = p * pw, pn = min(pw, w - c0);
    // inv(L_pp) inside the inverse of its chain block (schedule.hpp winv_offset / winv_ld): the
    // chain block's cw x cw matrix, rows from c0 - g0, columns from c0 - g0
    const int g0 = (c0 / u.cb) * u.cb, ldw = min(u.cb, w - g0);
    int64_t slot = u.dinv_off;
    for (int t = 0; t < g0; t += u.cb) {
      const int64_t cwt = min(u.cb, w - t);
      slot += cwt * cwt;
    }
    const double* D = dinv + slot + (int64_t)(c0 - g0) * ldw + (c0 - g0);
    if (!BWD) {
      // rows of inv(L_pp) for the second half, requested before the first half's loads
      double dv[4][4];
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          dv[r][e] = D[(int64_t)min(rr + 16 * r, pn - 1) * ldw + min(sub + 16 * e, pn - 1)];
      // t_j = y_j - sum_{k<c0} L[c0+j][k] x_k
      if (c0 > 0) {
        double acc[4][NR];
#pragma unroll
        for (int r = 0; r < 4; ++r)
          dot16<NR, kXS>(A + (int64_t)(c0 + min(rr + 16 * r, pn - 1)) * w, xb, c0, sub, acc[r]);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int q = 0; q < NR; ++q) {
            const double sacc = sum16(acc[r][q]);
            const int j = rr + 16 * r;
            if (sub == 0 && j < pn) tb[q * 64 + j] = xb[q * kXS + c0 + j] - sacc;
          }
      } else if (tid < pn) {
#pragma unroll
        for (int q = 0; q < NR; ++q) tb[q * 64 + tid] = xb[q * kXS + tid];
      }
      __syncthreads();
      // x_j = sum_{k<=j} Dinv[j][k] t_k   (Dinv is lower triangular, zeros above)
      {
        double acc[4][NR];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int q = 0; q < NR; ++q) {
            double sa = 0.0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int k = sub + 16 * e;
              sa = __builtin_fma(k < pn ? dv[r][e] : 0.0, tb[q * 64 + min(k, pn - 1)], sa);
            }
            acc[r][q] = sa;
          }
        __syncthreads();   // every read of tb is done before xb/tb change
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int q = 0; q < NR; ++q) {
            const double sacc = sum16(acc[r][q]);
            const int j = rr + 16 * r;
            if (sub == 0 && j < pn) xb[q * kXS + c0 + j] = sacc;
          }
      }
      __syncthreads();
    } else {
      // t_j = y_j - sum_{k>=c0+pn} L[k][c0+j] x_k : lane = column j, waves split k
      {
        double sa[NR];
#pragma unroll
        for (int q = 0; q < NR; ++q) sa[q] = 0.0;
        const int kbeg = c0 + pn, cj = c0 + min(lane, pn - 1);
        for (int k0 = kbeg + wave; k0 < w; k0 += 32) {
          double v[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = A[(int64_t)min(k0 + 4 * e, w - 1) * w + cj];
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const int k = k0 + 4 * e;
            const double a = k < w ? v[e] : 0.0;
#pragma unroll
            for (int q = 0; q < NR; ++q) sa[q] = __builtin_fma(a, xb[q * kXS + min(k, w - 1)], sa[q]);
          }
        }
#pragma unroll
        for (int q = 0; q < NR; ++q) part[wave][q * 64 + lane] = sa[q];
      }
      __syncthreads();
      if (tid < pn) {
#pragma unroll
        for (int q = 0; q < NR; ++q)
          tb[q * 64 + tid] = xb[q * kXS + c0 + tid] - (part[0][q * 64 + tid] + part[1][q * 64 + tid] +
                                                       part[2][q * 64 + tid] + part[3][q * 64 + tid]);
      }
      __syncthreads();
      // x_j = sum_{k>=j} Dinv[k][j] t_k
      {
        double sa[NR];
#pragma unroll
        for (int q = 0; q < NR; ++q) sa[q] = 0.0;
        const int cj = min(lane, pn - 1);
        for (int k0 = wave; k0 < pn; k0 += 32) {
          double v[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = D[(int64_t)min(k0 + 4 * e, pn - 1) * ldw + cj];
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const int k = k0 + 4 * e;
            const double a = k < pn ? v[e] : 0.0;
#pragma unroll
            for (int q = 0; q < NR; ++q) sa[q] = __builtin_fma(a, tb[q * 64 + min(k, pn - 1)], sa[q]);
          }
        }
#pragma unroll
        for (int q = 0; q < NR; ++q) part[wave][q * 64 + lane] = sa[q];
      }
      __syncthreads();
      if (tid < pn) {
#pragma unroll
        for (int q = 0; q < NR; ++q)
          xb[q * kXS + c0 + tid] = part[0][q * 64 + tid] + part[1][q * 64 + tid] +
                                   part[2][q * 64 + tid] + part[3][q * 64 + tid];
      }
      __syncthreads();
    }
  }
  for (int j = tid; j < w; j += 256) {
    const int gi = u.gcol0 + j;          // (the block column's own columns are consecutive pivot positions)
#pragma unroll
    for (int q = 0; q < NR; ++q) y[q * ldy + gi] = xb[q * kXS + j];
  }
}

// The same for block columns of at most four 64-wide panels (pw = cb = 64, w <= 256: the bench
// configuration's nb = 256) with ONE round trip to memory: the panel steps are a dependent sequence,
// but what they read of L does not depend on them -- every thread requests its share of the whole
// strictly lower part of the diagonal block (96 values) when the kernel starts, and the inverse of the
// next panel while it works on the current one, so a step is LDS reads, FMAs, a 16-lane reduction and
// barriers.  (The general kernel above pays a global round trip per panel step: 24.6 us per 256-wide
// block column forward, 14.1 backward, on the bench workload; 238 dependent launches per solve.)
template <bool BWD, int NR, class Fill>
__device__ __forceinline__ void solve_diag4_body(const SolveUnit& u, const double* __restrict__ L,
                                                 const double* __restrict__ dinv, double* __restrict__ y,
                                                 int64_t ldy, Fill fill) {
  __shared__ double xb[NR * 256];
  __shared__ double tb[NR * 64];
  __shared__ double part[4][NR * 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int sub = tid & 15, rr = tid >> 4;   // forward: 16 lanes per row, 16 rows per pass
  const int w = u.w;
  const int np = (w + 63) >> 6;
  const double* A = L + u.off;
  // ---- everything of L the steps will read ------------------------------------------------
  double lv[3][4][12];       // forward: panel p + 1, row rr + 16 r, columns sub + 16 e (e < 4 (p + 1))
  double bv[3][48];          // backward: panel p, column lane, rows 64 (p + 1) + wave + 4 i (i < 16 (3 - p))
  if (!BWD) {
#pragma unroll
    for (int p = 1; p < 4; ++p) {
      if (p >= np) break;
      const int c0 = 64 * p, pn = min(64, w - c0);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double* row = A + (int64_t)(c0 + min(rr + 16 * r, pn - 1)) * w;
#pragma unroll
        for (int e = 0; e < 4 * p; ++e) lv[p - 1][r][e] = row[sub + 16 * e];
      }
    }
  } else {
#pragma unroll
    for (int p = 0; p < 3; ++p) {
      if (p + 1 >= np) break;
      const int cj = 64 * p + lane;               // (a full panel: p + 1 < np)
#pragma unroll
      for (int i = 0; i < 16 * (3 - p); ++i) {
        const int k = 64 * (p + 1) + wave + 4 * i;
        bv[p][i] = A[(int64_t)min(k, w - 1) * w + cj];
      }
    }
  }
  // inverse of a panel: slot of panel p = dinv_off + sum of the squares of the panels before it (all 64 wide)
  auto wload = [&](int p, double (&dv)[16]) {
    const int pn = min(64, w - 64 * p);
    const double* D = dinv + u.dinv_off + (int64_t)p * 4096;
    if (!BWD) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int e = 0; e < 4; ++e) dv[4 * r + e] = D[(int64_t)min(rr + 16 * r, pn - 1) * pn + min(sub + 16 * e, pn - 1)];
    } else {
#pragma unroll
      for (int e = 0; e < 16; ++e) dv[e] = D[(int64_t)min(wave + 4 * e, pn - 1) * pn + min(lane, pn - 1)];
    }
  };
  double dv[16], dvn[16];
  wload(BWD ? np - 1 : 0, dv);
  fill(xb, 256);
  __syncthreads();
#pragma unroll
  for (int pp = 0; pp < 4; ++pp) {
    if (pp >= np) break;
    const int p = BWD ? np - 1 - pp : pp;
    const int c0 = 64 * p, pn = min(64, w - c0);
    if (pp + 1 < np) wload(BWD ? p - 1 : p + 1, dvn);
    if (!BWD) {
      // t_j = y_j - sum_{k < c0} L[c0 + j][k] x_k
      if (pp > 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int q = 0; q < NR; ++q) {
            double sa = 0.0;
#pragma unroll
            for (int e = 0; e < 4 * pp; ++e) sa = __builtin_fma(lv[pp - 1][r][e], xb[q * 256 + sub + 16 * e], sa);
            sa = sum16(sa);
            const int j = rr + 16 * r;
            if (sub == 0 && j < pn) tb[q * 64 + j] = xb[q * 256 + c0 + j] - sa;
          }
      } else if (tid < pn) {
#pragma unroll
        for (int q = 0; q < NR; ++q) tb[q * 64 + tid] = xb[q * 256 + tid];
      }
      __syncthreads();
      // x_j = sum_{k <= j} Dinv[j][k] t_k
      double acc[4][NR];
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int q = 0; q < NR; ++q) {
          double sa = 0.0;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int k = sub + 16 * e;
            sa = __builtin_fma(k < pn ? dv[4 * r + e] : 0.0, tb[q * 64 + min(k, pn - 1)], sa);
          }
          acc[r][q] = sum16(sa);
        }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = rr + 16 * r;
        if (sub == 0 && j < pn) {
#pragma unroll
          for (int q = 0; q < NR; ++q) xb[q * 256 + c0 + j] = acc[r][q];
        }
      }
      __syncthreads();
    } else {
      // t_j = y_j - sum_{k >= c0 + pn} L[k][c0 + j] x_k : lane = column j, the waves split k
      if (pp > 0) {
        double sa[NR];
#pragma unroll
        for (int q = 0; q < NR; ++q) sa[q] = 0.0;
        // (p = np - 1 - pp: the rows below are those of the pp panels behind it; bv[p] was loaded for
        // i < 16 (3 - p), of which the first 16 pp exist)
#pragma unroll
        for (int pc = 0; pc < 3; ++pc) {
          if (pc != p) continue;
#pragma unroll
          for (int i = 0; i < 16 * (3 - pc); ++i) {
            const int k = 64 * (pc + 1) + wave + 4 * i;
            const double a = k < w ? bv[pc][i] : 0.0;
#pragma unroll
            for (int q = 0; q < NR; ++q) sa[q] = __builtin_fma(a, xb[q * 256 + min(k, w - 1)], sa[q]);
          }
        }
#pragma unroll
        for (int q = 0; q < NR; ++q) part[wave][q * 64 + lane] = sa[q];
        __syncthreads();
        if (tid < pn) {
#pragma unroll
          for (int q = 0; q < NR; ++q)
            tb[q * 64 + tid] = xb[q * 256 + c0 + tid] - (part[0][q * 64 + tid] + part[1][q * 64 + tid] +
                                                         part[2][q * 64 + tid] + part[3][q * 64 + tid]);
        }
      } else if (tid < pn) {
#pragma unroll
        for (int q = 0; q < NR; ++q) tb[q * 64 + tid] = xb[q * 256 + c0 + tid];
      }
      __syncthreads();
      // x_j = sum_{k >= j} Dinv[k][j] t_k
      {
        double sa[NR];
#pragma unroll
        for (int q = 0; q < NR; ++q) sa[q] = 0.0;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int k = wave + 4 * e;
          const double a = k < pn ? dv[e] : 0.0;
#pragma unroll
          for (int q = 0; q < NR; ++q) sa[q] = __builtin_fma(a, tb[q * 64 + min(k, pn - 1)], sa[q]);
        }
#pragma unroll
        for (int q = 0; q < NR; ++q) part[wave][q * 64 + lane] = sa[q];
      }
      __syncthreads();
      if (tid < pn) {
#pragma unroll
        for (int q = 0; q < NR; ++q)
          xb[q * 256 + c0 + tid] = part[0][q * 64 + tid] + part[1][q * 64 + tid] +
                                   part[2][q * 64 + tid] + part[3][q * 64 + tid];
      }
      __syncthreads();
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) dv[e] = dvn[e];
  }
  for (int j = tid; j < w; j += 256) {
    const int gi = u.gcol0 + j;          // (the block column's own columns are consecutive pivot positions)
#pragma unroll
    for (int q = 0; q < NR; ++q) y[q * ldy + gi] = xb[q * 256 + j];
  }
}

}  // namespace spx
