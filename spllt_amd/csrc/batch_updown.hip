// Low-rank update / downdate of the factors of a batch on gfx950: L_b L_b^T + sign W_b W_b^T in place for every
// member, ONE pattern of W for all members, each member its own values.  The arithmetic is
// that of updown.hip -- the same device bodies, ud_body.hpp -- with the member taken from the workgroup index
// (bsi_split), so a launch carries all members and the chain of dependent launches is as long as for one factor.
//
//   k_bupdown_scatter  grid (entries x members): Wd[b * wstride + pos[i]] = wval[b * ldw + ent[i]]; the word of a
//                      failed downdate is merged into the batch's flag between passes
//   k_bupdown_gen      one workgroup per member: the diagonal square of one block column (ud_gen_block)
//   k_bupdown_apply    (strips x members) workgroups: the rows below the square (ud_apply_block)
//
// Two exits, both uniform per workgroup and taken before L is read: a member whose flag is set (not positive
// definite at factor_batch, or after an earlier pass), and a block column whose own columns hold only zeros in the
// member's work array -- every rotation would be c = 1, t = 0.  The generate workgroup stores kBupdownSkip in the
// member's coefficient scratch for the apply workgroups; arena and dinv slots stay bit for bit.  No loop bound
// depends on data otherwise.  No atomics: built without -munsafe-fp-atomics.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>

#include "batch_split.hpp"
#include "kernels.hpp"
#include "ud_body.hpp"

namespace spx {

namespace {

__global__ __launch_bounds__(256) void k_bupdown_scatter(BupdownView s, const int64_t* __restrict__ pos,
                                                         const int* __restrict__ ent, int64_t count, int64_t nblk,
                                                         const double* __restrict__ wval, int64_t ldw, int reset) {
  int b;
  int64_t t;
  bsi_split(s.v, nblk, b, t);
  const int64_t i = t * 256 + threadIdx.x;
  const int fl = s.v.flag[b];
  const int uf = reset ? INT_MAX : s.udflag[b];
  if (i == 0) {
    if (reset) s.udflag[b] = INT_MAX;
    else if (uf != INT_MAX && fl == INT_MAX) s.v.flag[b] = uf;
  }
  if (fl != INT_MAX || uf != INT_MAX) return;
  if (i < count) s.Wd[(int64_t)b * s.wstride + pos[i]] = wval[(int64_t)b * ldw + ent[i]];
}

template <int NV>
__global__ __launch_bounds__(256) void k_bupdown_gen(BupdownView s, const SolveUnit u, double sgn) {
  extern __shared__ __attribute__((aligned(16))) double bud_lds[];
  int b;
  int64_t t;
  bsi_split(s.v, 1, b, t);
  if (s.v.flag[b] != INT_MAX) return;
  double* Wd = s.Wd + (int64_t)b * s.wstride;
  double* coefg = s.coef + (int64_t)b * s.cstride;
  // all kUpdownVec slots of the block column's own columns (consecutive pivot positions)
  const double* own = Wd + (int64_t)u.gcol0 * kUdKK;
  int nz = 0;
  for (int e = threadIdx.x; e < u.w * kUdKK; e += 256) nz |= own[e] != 0.0;
  if (!__syncthreads_or(nz)) {
    if (threadIdx.x == 0) coefg[0] = kBupdownSkip;
    return;
  }
  ud_gen_block<NV>(u, s.v.L + (int64_t)b * s.v.lstride, s.v.dinv + (int64_t)b * s.v.dstride, Wd, coefg, s.udflag + b,
                   sgn, bud_lds);
}

template <int NV>
__global__ __launch_bounds__(256) void k_bupdown_apply(BupdownView s, const SolveUnit u, int64_t strips,
                                                       const int* __restrict__ rlist, double sgn) {
  __shared__ __attribute__((aligned(16))) double tile[kUdApplyTile];
  __shared__ double coef[kUdApplyCoef];
  int b;
  int64_t g;
  bsi_split(s.v, strips, b, g);
  if (s.v.flag[b] != INT_MAX) return;
  const double* coefg = s.coef + (int64_t)b * s.cstride;
  if (coefg[0] == kBupdownSkip) return;
  ud_apply_block<NV>(u, s.v.L + (int64_t)b * s.v.lstride, rlist, s.Wd + (int64_t)b * s.wstride, coefg, sgn, (int)g,
                     tile, coef);
}

// fn(view of the members [b0, b0 + r.v.nbatch), b0) once per range
template <class Fn>
int bupdown_ranges(const BupdownView& s, int64_t per_member, Fn&& fn) {
  return batch_member_ranges(s.v.nbatch, per_member, [&](int b0, int nb) {
    BupdownView r = s;
    r.v.nbatch = nb;
    r.v.L += (int64_t)b0 * s.v.lstride;
    r.v.dinv += (int64_t)b0 * s.v.dstride;
    r.v.flag += b0;
    r.Wd += (int64_t)b0 * s.wstride;
    r.coef += (int64_t)b0 * s.cstride;
    r.udflag += b0;
    fn(r, b0);
  });
}

template <int NV>
void gen_nv(hipStream_t st, const BupdownView& r, const SolveUnit& u, int sign) {
  thread_local int attr_dev = -1;      // (more than 64 KiB of dynamic LDS: allowed per device)
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (dev != attr_dev) {
    (void)hipFuncSetAttribute((const void*)k_bupdown_gen<NV>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kUdGenLds);
    attr_dev = dev;
  }
  hipLaunchKernelGGL(k_bupdown_gen<NV>, dim3((unsigned)r.v.nbatch), dim3(256), kUdGenLds, st, r, u, (double)sign);
}

}  // namespace

int launch_bupdown_scatter(hipStream_t st, const BupdownView& s, const int64_t* pos, const int* ent, int64_t count,
                           const double* wval, int64_t ldw, bool reset) {
  const int64_t nblk = std::max<int64_t>(1, (count + 255) / 256);
  return bupdown_ranges(s, nblk, [&](const BupdownView& r, int b0) {
    hipLaunchKernelGGL(k_bupdown_scatter, dim3((unsigned)(nblk * r.v.nbatch)), dim3(256), 0, st, r, pos, ent, count, nblk,
                       wval + (int64_t)b0 * ldw, ldw, reset ? 1 : 0);
  });
}

// nv: the vectors of the pass; the kernels are built for 1, 2, 4 and 8 (the next of these: the vectors beyond
// nv are zero in Wd, and a zero vector is the identity)
int launch_bupdown_gen(hipStream_t st, const BupdownView& s, const SolveUnit& u, int sign, int nv) {
  return bupdown_ranges(s, 1, [&](const BupdownView& r, int) {
    if (nv <= 1) gen_nv<1>(st, r, u, sign);
    else if (nv == 2) gen_nv<2>(st, r, u, sign);
    else if (nv <= 4) gen_nv<4>(st, r, u, sign);
    else gen_nv<8>(st, r, u, sign);
  });
}

int launch_bupdown_apply(hipStream_t st, const BupdownView& s, const SolveUnit& u, const int* rlist, int sign, int nv) {
  const int below = u.nrow - u.w;
  if (below <= 0) return 0;
  const int64_t strips = (below + kUpdownRows - 1) / kUpdownRows;
  const double sgn = (double)sign;
  return bupdown_ranges(s, strips, [&](const BupdownView& r, int) {
    const dim3 grid((unsigned)(strips * r.v.nbatch));
    if (nv <= 1) hipLaunchKernelGGL(k_bupdown_apply<1>, grid, dim3(256), 0, st, r, u, strips, rlist, sgn);
    else if (nv == 2) hipLaunchKernelGGL(k_bupdown_apply<2>, grid, dim3(256), 0, st, r, u, strips, rlist, sgn);
    else if (nv <= 4) hipLaunchKernelGGL(k_bupdown_apply<4>, grid, dim3(256), 0, st, r, u, strips, rlist, sgn);
    else hipLaunchKernelGGL(k_bupdown_apply<8>, grid, dim3(256), 0, st, r, u, strips, rlist, sgn);
  });
}

}  // namespace spx
