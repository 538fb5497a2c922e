// Host-only test of stage_updown (spllt_amd/csrc/updown_stage.hpp): pass counts, position lists and per-pass plans
// against a brute-force restatement, on a small tree of block columns.  Built with the address and
// undefined-behaviour sanitizers by tests/test_updown_batch_cpu.py and run as a program of its own.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "updown_stage.hpp"

namespace {

constexpr int N = 40, VEC = 8;
// the stand-in symbolic: block column of a pivot position = position / 4, parent of block column b = PARENT[b]
// (10 = none); a sweep from position j visits bcol(j) and its ancestors
const int PARENT[10] = {2, 2, 6, 5, 5, 6, 9, 8, 9, 10};

void paths(const int* first, int count, std::vector<int>& out) {
  std::set<int> s;
  for (int v = 0; v < count; ++v)
    for (int b = first[v] / 4; b < 10; b = PARENT[b]) s.insert(b);
  out.assign(s.begin(), s.end());
}

int fails = 0;
#define CHECK(c)                                                    \
  do {                                                              \
    if (!(c)) {                                                     \
      std::printf("FAILED line %d: %s\n", __LINE__, #c);            \
      ++fails;                                                      \
    }                                                               \
  } while (0)

// k columns; column v is empty when empty[v], else rows {r, r + 1 (when it exists)} with r = (7 v + 3) mod N, the
// last column on the last pivot alone when last_pivot
void run(int k, const std::vector<char>& empty, bool last_pivot) {
  std::vector<int> order((size_t)N);
  for (int i = 0; i < N; ++i) order[(size_t)i] = (i * 17 + 5) % N;   // a permutation (17 and 40 are coprime)
  int last_var = 0;
  for (int i = 0; i < N; ++i)
    if (order[(size_t)i] == N - 1) last_var = i;
  std::vector<int> wptr(1, 1), wrow, first;
  for (int v = 0; v < k; ++v) {
    if (!empty[(size_t)v]) {
      if (last_pivot && v == k - 1) {
        wrow.push_back(last_var + 1);
      } else {
        const int r = (7 * v + 3) % N;
        wrow.push_back(r + 1);
        if (r + 1 < N) wrow.push_back(r + 2);
      }
    }
    wptr.push_back((int)wrow.size() + 1);
    int j = -1;
    for (int e = wptr[(size_t)v] - 1; e < wptr[(size_t)v + 1] - 1; ++e) {
      const int p = order[(size_t)wrow[(size_t)e] - 1];
      if (j < 0 || p < j) j = p;
    }
    first.push_back(j);
  }
  wrow.push_back(0);   // (never read)
  spx::UpdownStage st;
  spx::stage_updown(k, wptr.data(), wrow.data(), order.data(), first.data(), VEC, paths, st);

  // the restatement: walk the columns, open a new pass at every 8th non-empty one
  int nonempty = 0;
  std::vector<std::vector<int>> pass_cols;
  for (int v = 0; v < k; ++v) {
    if (wptr[(size_t)v + 1] == wptr[(size_t)v]) continue;
    if (nonempty % VEC == 0) pass_cols.emplace_back();
    pass_cols.back().push_back(v);
    ++nonempty;
  }
  CHECK(st.npass == (int)pass_cols.size());
  CHECK(st.npass == (nonempty + VEC - 1) / VEC);
  CHECK((int)st.cols.size() == nonempty);
  CHECK((int)st.pass_ptr.size() == st.npass + 1 && (int)st.plan_ptr.size() == st.npass + 1);
  CHECK((int)st.pass_nc.size() == st.npass);
  CHECK(st.pos.size() == st.ent.size());
  if (fails) return;
  int64_t at = 0, pat = 0;
  std::set<int> seen;
  for (int p = 0; p < st.npass; ++p) {
    CHECK(st.pass_ptr[(size_t)p] == at && st.plan_ptr[(size_t)p] == pat);
    CHECK(st.pass_nc[(size_t)p] == (int)pass_cols[(size_t)p].size());
    std::set<int> want_plan;
    for (size_t q = 0; q < pass_cols[(size_t)p].size(); ++q) {
      const int v = pass_cols[(size_t)p][q];
      for (int e = wptr[(size_t)v] - 1; e < wptr[(size_t)v + 1] - 1; ++e, ++at) {
        CHECK(at < (int64_t)st.pos.size());
        if (at >= (int64_t)st.pos.size()) return;
        const int pv = order[(size_t)wrow[(size_t)e] - 1];
        CHECK(st.pos[(size_t)at] == (int64_t)pv * VEC + (int64_t)q);
        CHECK(st.ent[(size_t)at] == e);
        CHECK(seen.insert(e).second);
      }
      for (int b = first[(size_t)v] / 4; b < 10; b = PARENT[b]) want_plan.insert(b);
    }
    const std::vector<int> want(want_plan.begin(), want_plan.end());
    const std::vector<int> got(st.plan.begin() + st.plan_ptr[(size_t)p], st.plan.begin() + st.plan_ptr[(size_t)p + 1]);
    CHECK(got == want);
    pat += (int64_t)want.size();
  }
  CHECK(at == (int64_t)st.pos.size() && at == (int64_t)wptr[(size_t)k] - 1);
  CHECK(pat == (int64_t)st.plan.size());
  if (last_pivot && k > 0 && !empty[(size_t)k - 1]) {
    CHECK(st.pos.back() / VEC == N - 1);
    CHECK(st.plan.back() == 9);
  }
}

}  // namespace

int main() {
  for (int k : {0, 1, 8, 9, 17}) {
    run(k, std::vector<char>((size_t)k, 0), false);
    run(k, std::vector<char>((size_t)k, 0), true);
    std::vector<char> holes((size_t)k, 0);
    for (int v = 0; v < k; ++v) holes[(size_t)v] = v % 3 == 1;   // empty columns in between
    run(k, holes, false);
    run(k, holes, true);
    run(k, std::vector<char>((size_t)k, 1), false);             // every column empty: no pass
  }
  if (fails) {
    std::printf("updown_stage_test: %d checks failed\n", fails);
    return 1;
  }
  std::printf("updown_stage_test: ok\n");
  return 0;
}
