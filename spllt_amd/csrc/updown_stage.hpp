// The staging of one update / downdate call, host only and without a device (tests/native/updown_stage_test.cpp):
// the non-empty columns of W cut into passes of `vec` columns, per pass the positions of its entries in the work
// array with the CSC entry each comes from, and the plan of the pass.  W's pattern is shared by the members of a
// batch, so one staging serves them all; the values stay where the caller has them.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace spx {

struct UpdownStage {
  std::vector<int> cols;           // the non-empty columns of W, ascending (0-based)
  int npass = 0;
  std::vector<int> pass_nc;        // columns of pass p (vec, the last pass may have fewer)
  std::vector<int64_t> pass_ptr;   // pass p owns pos / ent [pass_ptr[p], pass_ptr[p + 1])
  std::vector<int64_t> pos;        // order[row - 1] * vec + q: pivot position of the entry, vector q of its pass
  std::vector<int> ent;            // 0-based CSC position of the entry (its value: wval[ent])
  std::vector<int64_t> plan_ptr;   // pass p visits plan [plan_ptr[p], plan_ptr[p + 1]), ascending
  std::vector<int> plan;
};

// wptr / wrow: k columns, CSC, 1-based (validated by the caller: build_updown_plan).  order: user variable -> pivot
// position.  first[v]: the first pivot position of column v, -1 for an empty column.  paths(first positions, count,
// out): the block columns a sweep that starts at these positions visits, ascending (updown_paths).
template <class Paths>
void stage_updown(int k, const int* wptr, const int* wrow, const int* order, const int* first, int vec, Paths&& paths,
                  UpdownStage& st) {
  st = UpdownStage();
  for (int v = 0; v < k; ++v)
    if (first[v] >= 0) st.cols.push_back(v);
  const int nc_all = (int)st.cols.size();
  st.npass = (nc_all + vec - 1) / vec;
  st.pass_ptr.assign(1, 0);
  st.plan_ptr.assign(1, 0);
  std::vector<int> pf, plan;
  for (int p = 0; p < st.npass; ++p) {
    const int c0 = p * vec, nc = std::min(vec, nc_all - c0);
    st.pass_nc.push_back(nc);
    pf.clear();
    for (int q = 0; q < nc; ++q) {
      const int v = st.cols[(size_t)(c0 + q)];
      for (int e = wptr[v] - 1; e < wptr[v + 1] - 1; ++e) {
        st.pos.push_back((int64_t)order[(size_t)wrow[e] - 1] * vec + q);
        st.ent.push_back(e);
      }
      pf.push_back(first[v]);
    }
    st.pass_ptr.push_back((int64_t)st.pos.size());
    paths(pf.data(), nc, plan);
    st.plan.insert(st.plan.end(), plan.begin(), plan.end());
    st.plan_ptr.push_back((int64_t)st.plan.size());
  }
}

}  // namespace spx
