// What the batched translation units share (batch_selinv.hip, batch_adjoint.hip, batch_refine.hip): the map from a
// workgroup to (member, work item), and the split of the members of a launch into ranges.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "kernels.hpp"

namespace spx {

// workgroup -> (member, work item), as in batch.hip
__device__ __forceinline__ void bsi_split(const BatchView& v, int64_t count, int& b, int64_t& t) {
  const unsigned wg = blockIdx.x;
  if (v.member_fast) {
    b = (int)(wg % (unsigned)v.nbatch);
    t = wg / (unsigned)v.nbatch;
  } else {
    b = (int)(wg / (unsigned)count);
    t = wg % (unsigned)count;
  }
}

// fn(first member b0, members of the range) once per range: one range as long as (work items) x (members) fits a
// grid (the limit of batch.hip, test hook included).  Returns the number of ranges (-1, fn never called: ONE member's
// work items overflow a grid).
template <class Fn>
int batch_member_ranges(int nbatch, int64_t per_member, Fn&& fn) {
  if (per_member <= 0 || nbatch <= 0) return 0;
  if (per_member > batch_grid_limit_max()) return -1;
  const int step = (int)std::max<int64_t>(1, std::min<int64_t>(nbatch, batch_grid_limit() / per_member));
  int launches = 0;
  for (int b0 = 0; b0 < nbatch; b0 += step) {
    fn(b0, std::min(step, nbatch - b0));
    ++launches;
  }
  return launches;
}

// the same with fn(view of the members [b0, b0 + r.v.nbatch), b0)
template <class Fn>
int bsi_member_ranges(const BatchSelinvView& s, int64_t per_member, Fn&& fn) {
  return batch_member_ranges(s.v.nbatch, per_member, [&](int b0, int nb) {
    BatchSelinvView r = s;
    r.v.nbatch = nb;
    r.v.L += (int64_t)b0 * s.v.lstride;
    r.v.dinv += (int64_t)b0 * s.v.dstride;
    if (r.v.flag) r.v.flag += b0;
    r.Z += (int64_t)b0 * s.v.lstride;
    if (r.scratch) r.scratch += (int64_t)b0 * s.sstride;
    fn(r, b0);
  });
}

}  // namespace spx
