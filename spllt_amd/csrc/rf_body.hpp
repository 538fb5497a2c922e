// Device bodies that refine.hip and batch_refine.hip share: the row body of the sparse product, the workgroup
// sums, the bodies of the vector kernels and the scalar step behind every reduction.  A kernel of either file
// resolves its (vector) or (member, vector) to base pointers and calls the body, so that a member of a batch
// gets the arithmetic of the single handle, sum for sum.
//
// Partial sums: a workgroup's two sums of one vector go to part[0] and part[pstride] of the address the caller
// resolved; refine.hip: part + (slot * 2) * RF_G + q with pstride = RF_G, batch_refine.hip: the same with the
// number of (member, vector) pairs of the pass in place of RF_G.
//
// sc: a power of two by which an entry of a residual-like vector (b, r: of the size of max |a_ij| |x|) is multiplied
// before it is squared.  refine.hip passes the constant 1 (the product folds away); batch_refine.hip passes member
// b's 2^-exponent(max |a_ij|), so that the squares of a member scaled by 2^600 do not overflow.  A power of two
// commutes with every rounding: without overflow or underflow the scaled error has the bits of the unscaled one.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "refine.hpp"

namespace spx {

__device__ __forceinline__ bool rf_selected(const int* sel, int want, int q) { return !sel || sel[q] == want; }

// sum over the wavefront (butterfly: every lane ends with the same bits)
__device__ __forceinline__ double rf_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// the workgroup's sums of a and b to part[0] and part[pstride]; every thread of the 256 calls it
__device__ __forceinline__ void rf_block_sum2(double a, double b, double* part, int64_t pstride) {
  __shared__ double red[2][4];
  a = rf_wave_sum(a);
  b = rf_wave_sum(b);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { red[0][wave] = a; red[1][wave] = b; }
  __syncthreads();
  if (threadIdx.x < 2) {
    const int w = threadIdx.x;
    part[(int64_t)w * pstride] = ((red[w][0] + red[w][1]) + red[w][2]) + red[w][3];
  }
}

// ---------------------------------------------------------------------------------------------------
// Row block `rblock` of one length class for the vectors q0 .. q0 + nq (bit j of act: vector q0 + j takes part):
// workgroup = 4 wavefronts x (64 / LPR) rows.  Lane `sub` of a row's LPR lanes takes entries sub, sub + LPR, ...
// in order, the LPR sums meet in a butterfly.  x, b and y point at vector 0 of the caller's set; part (may be
// null) at the workgroup's slot for vector 0.
// ---------------------------------------------------------------------------------------------------
template <int LPR, bool RES>
__device__ __forceinline__ void rf_spmv_body(int rblock, int q0, int nq, unsigned act, const int* __restrict__ rows,
                                             int nrows, const int64_t* __restrict__ rowptr,
                                             const int* __restrict__ col, const int* __restrict__ src,
                                             const double* __restrict__ val, const double* __restrict__ x, int64_t ldx,
                                             const double* __restrict__ b, double* __restrict__ y, int64_t ldy,
                                             double* __restrict__ part, int64_t pstride, double sc,
                                             double (*red)[2 * RF_NV]) {
  constexpr int RPW = 64 / LPR, RPB = 4 * RPW;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sub = lane % LPR;
  const int ri = rblock * RPB + wave * RPW + lane / LPR;
  const bool has = ri < nrows;
  const int row = has ? rows[ri] : 0;
  const int64_t k0 = has ? rowptr[row] : 0, k1 = has ? rowptr[row + 1] : 0;
  double acc[RF_NV];
#pragma unroll
  for (int j = 0; j < RF_NV; ++j) acc[j] = 0.0;
  for (int64_t k = k0 + sub; k < k1; k += LPR) {
    const int c = col[k];
    const double a = val[src[k]];
#pragma unroll
    for (int j = 0; j < RF_NV; ++j)
      if (j < nq) acc[j] = fma(a, x[(int64_t)(q0 + j) * ldx + c], acc[j]);
  }
#pragma unroll
  for (int j = 0; j < RF_NV; ++j)
#pragma unroll
    for (int off = LPR / 2; off >= 1; off >>= 1) acc[j] += __shfl_xor(acc[j], off, 64);
  const bool lead = has && sub == 0;
  double p0[RF_NV], p1[RF_NV];
#pragma unroll
  for (int j = 0; j < RF_NV; ++j) {
    p0[j] = 0.0;
    p1[j] = 0.0;
    if (lead && ((act >> j) & 1u)) {
      const double xr = x[(int64_t)(q0 + j) * ldx + row];
      const double out = RES ? b[(int64_t)(q0 + j) * ldy + row] - acc[j] : acc[j];
      y[(int64_t)(q0 + j) * ldy + row] = out;
      const double os = sc * out;
      p0[j] = RES ? os * os : xr * out;
      p1[j] = RES ? xr * xr : 0.0;
    }
  }
  if (!part) return;   // (the same for every thread of the workgroup)
#pragma unroll
  for (int j = 0; j < RF_NV; ++j) {
    p0[j] = rf_wave_sum(p0[j]);
    p1[j] = rf_wave_sum(p1[j]);
    if (lane == 0) { red[wave][2 * j] = p0[j]; red[wave][2 * j + 1] = p1[j]; }
  }
  __syncthreads();
  if (threadIdx.x < 2 * RF_NV) {
    const int j = threadIdx.x >> 1, w = threadIdx.x & 1;
    if (j < nq)
      part[(int64_t)w * pstride + q0 + j] =
          ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
  }
}

// ---------------------------------------------------------------------------------------------------
// vector kernels: slot `slot` of RF_VROWS rows of ONE vector, thread t takes rows i0 + t + 256 k; the pointers
// are those of the vector
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ void rf_axpy_body(int n, int slot, double a, double* __restrict__ x,
                                             const double* __restrict__ p, double* __restrict__ r,
                                             const double* __restrict__ qv, double sc, double& rr, double& xx) {
  rr = 0.0;
  xx = 0.0;
#pragma unroll
  for (int k = 0; k < RF_VROWS / 256; ++k) {
    const int i = slot * RF_VROWS + k * 256 + threadIdx.x;
    if (i < n) {
      const double xv = fma(a, p[i], x[i]);
      x[i] = xv;
      xx = fma(xv, xv, xx);
      if (qv) {
        const double rv = fma(-a, qv[i], r[i]);
        r[i] = rv;
        const double rs = sc * rv;
        rr = fma(rs, rs, rr);
      }
    }
  }
}

__device__ __forceinline__ void rf_pupdate_body(int n, int slot, double bt, double* __restrict__ p,
                                                const double* __restrict__ z) {
#pragma unroll
  for (int k = 0; k < RF_VROWS / 256; ++k) {
    const int i = slot * RF_VROWS + k * 256 + threadIdx.x;
    if (i < n) p[i] = bt == 0.0 ? z[i] : fma(bt, p[i], z[i]);
  }
}

__device__ __forceinline__ double rf_dot_body(int n, int slot, const double* __restrict__ a,
                                              const double* __restrict__ b, double sc) {
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < RF_VROWS / 256; ++k) {
    const int i = slot * RF_VROWS + k * 256 + threadIdx.x;
    if (i < n) s = fma(sc * a[i], sc * b[i], s);
  }
  return s;
}

// dst = src (mine) or 0
__device__ __forceinline__ void rf_copy_body(int n, int slot, bool mine, double* __restrict__ dst,
                                             const double* __restrict__ src) {
#pragma unroll
  for (int k = 0; k < RF_VROWS / 256; ++k) {
    const int i = slot * RF_VROWS + k * 256 + threadIdx.x;
    if (i < n) dst[i] = mine ? src[i] : 0.0;
  }
}

// max that a NaN wins: once m is a NaN no comparison replaces it
__device__ __forceinline__ double rf_nanmax(double m, double a) { return (a > m || a != a) ? a : m; }

// part[0] = max |val| of workgroup wg's share of a grid of nwg (a NaN wins); red: 4 doubles of LDS
__device__ __forceinline__ void rf_absmax_body(const double* __restrict__ val, int64_t nnz, int wg, int nwg,
                                               double* __restrict__ part, double* red) {
  double m = 0.0;
  for (int64_t k = (int64_t)wg * 256 + threadIdx.x; k < nnz; k += (int64_t)nwg * 256) m = rf_nanmax(m, fabs(val[k]));
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) m = rf_nanmax(m, __shfl_xor(m, off, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) part[0] = rf_nanmax(rf_nanmax(rf_nanmax(red[0], red[1]), red[2]), red[3]);
}

// the max of nslots partial maxima (one workgroup of 256; mred: 256 doubles of LDS); valid in thread 0
__device__ __forceinline__ double rf_absmax_final(const double* __restrict__ part, int nslots, double* mred) {
  const int t = threadIdx.x;
  double m = 0.0;
  for (int s = t; s < nslots; s += 256) m = rf_nanmax(m, part[s]);
  mred[t] = m;
  __syncthreads();
  if (t == 0)
    for (int s = 1; s < 256; ++s) m = rf_nanmax(m, mred[s]);
  return m;
}

__device__ __forceinline__ bool rf_finite(double v) { return v == v && fabs(v) <= 1.79769313486231570e308; }

// ---------------------------------------------------------------------------------------------------
// Second stage of a reduction: thread t of 256 adds the partials of vector t & 31 in slots (t >> 5),
// (t >> 5) + 8, ... (part points at slot 0 of vector 0; a slot is 2 * pstride doubles); the eight slices of a
// vector are then added in order.  s0 / s1 are valid in the threads t < 32 on return.
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ void rf_second_stage(bool sum, const double* __restrict__ part, int64_t pstride, int nslots,
                                                bool live, double (*red)[8][RF_G], double& s0, double& s1) {
  const int t = threadIdx.x, q = t & (RF_G - 1), sl = t >> 5;
  s0 = 0.0;
  s1 = 0.0;
  if (sum && live)
    for (int s = sl; s < nslots; s += 8) {
      s0 += part[((int64_t)s * 2) * pstride + q];
      s1 += part[((int64_t)s * 2 + 1) * pstride + q];
    }
  red[0][sl][q] = s0;
  red[1][sl][q] = s1;
  __syncthreads();
  if (t >= RF_G) return;
  s0 = red[0][0][q];
  s1 = red[1][0][q];
  for (int s = 1; s < 8; ++s) { s0 += red[0][s][q]; s1 += red[1][s][q]; }
}

// the scalars and the state of one vector
struct RfScalars {
  double *alpha, *beta, *rz, *bnorm, *ebest, *out_err, *out_st;
  int *st, *decl, *restart, *improve;
};

// the scalar step of `stage` for one vector (RfStage; amax = max |a_ij| of its matrix)
__device__ __forceinline__ void rf_scalar_step(int stage, double s0, double s1, double tol, int flag, double amax,
                                               const RfScalars& v) {
  int st = *v.st;
  switch (stage) {
    case RFS_BNORM:   // s0 = |b|^2: the start of a group
      *v.bnorm = sqrt(s0);
      *v.ebest = -1.0;
      *v.rz = 0.0;
      *v.alpha = 0.0;
      *v.beta = 0.0;
      st = 0;
      *v.decl = 0;
      *v.restart = 1;
      *v.improve = 0;
      break;
    case RFS_TRUE: {  // s0 = |b - A x|^2, s1 = |x|^2 of the vectors with st == 0 (flag = 0) / decl == 1 (flag = 1)
      const bool mine = flag ? *v.decl == 1 : st == 0;
      int improve = 0;
      if (mine) {
        const double e = s0 == 0.0 ? 0.0 : sqrt(s0) / (*v.bnorm + amax * sqrt(s1));
        const double eb = *v.ebest;
        if (eb < 0.0 || e < eb) { improve = 1; *v.ebest = e; }
        if (!rf_finite(e)) st = 2;
        else if (e <= tol) st = 1;
        else *v.restart = 1;   // (PCG: go on from the true residual with a fresh direction)
        *v.decl = 0;
      }
      *v.improve = improve;
      break;
    }
    case RFS_ALPHA:   // s0 = p.q
      if (st == 0) {
        const double a = *v.rz / s0;
        if (!rf_finite(a)) st = 2;
        *v.alpha = rf_finite(a) ? a : 0.0;
      }
      break;
    case RFS_REC:     // s0 = |r|^2 of the recurrence, s1 = |x|^2
      if (st == 0) {
        const double e = s0 == 0.0 ? 0.0 : sqrt(s0) / (*v.bnorm + amax * sqrt(s1));
        if (!rf_finite(e)) st = 2;
        else if (e <= tol) *v.decl = 1;
      }
      break;
    case RFS_BETA:    // s0 = r.z
      if (st == 0) {
        const double bt = *v.restart ? 0.0 : s0 / *v.rz;
        if (!rf_finite(bt) || !rf_finite(s0)) st = 2;
        *v.beta = rf_finite(bt) ? bt : 0.0;
        *v.rz = s0;
        *v.restart = 0;
      }
      break;
    case RFS_FINAL:   // what still iterates gets one true residual before the call returns
      *v.decl = st == 0 ? 1 : 0;
      break;
    default: break;
  }
  *v.st = st;
  *v.out_err = *v.ebest;
  *v.out_st = (double)st;
}

}  // namespace spx
