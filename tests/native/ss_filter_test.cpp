// Host-only test of build_solve_slots / filter_solve_program (spllt_amd/csrc/ss_filter.hpp): the slots and the
// filtered launches of two substitution programs of the same small tree -- panel width 256 and panel width = chain
// block = 64, the single handle's and the batch's -- against a brute-force restatement.  Built with the address and
// undefined-behaviour sanitizers by tests/test_solve_sparse_batch_cpu.py and run as a program of its own.
#include <cstdint>
#include <cstdio>
#include <set>
#include <vector>

#include "ss_filter.hpp"

namespace {

using namespace spx;

int fails = 0;
#define CHECK(c)                                                    \
  do {                                                              \
    if (!(c)) {                                                     \
      std::printf("FAILED line %d: %s\n", __LINE__, #c);            \
      ++fails;                                                      \
    }                                                               \
  } while (0)

// the stand-in tree: node s on level LEVEL[s] with NBC[s] block columns of width 16; block column c of a node has
// BELOW[s] + 16 (NBC[s] - 1 - c) rows below its square (0, 1, 2 or 3 strips of 64 rows)
constexpr int NN = 7;
const int LEVEL[NN] = {0, 0, 1, 0, 0, 1, 2};
const int NBC[NN] = {1, 2, 1, 1, 3, 2, 2};
const int BELOW[NN] = {40, 100, 130, 0, 64, 65, 0};

// the rule of build_solve_program: per level and block-column step one diagonal launch and one strip launch, the
// backward sweep their mirror; pw / cb only go into the units
void build(int pw, int cb, SolveProgram& P, std::vector<int>& bcol0) {
  P = SolveProgram();
  bcol0.assign(NN + 1, 0);
  for (int s = 0; s < NN; ++s) bcol0[(size_t)s + 1] = bcol0[(size_t)s] + NBC[s];
  int64_t off = 0, doff = 0;
  int gcol = 0;
  for (int s = 0; s < NN; ++s)
    for (int c = 0; c < NBC[s]; ++c) {
      SolveUnit u{};
      u.w = 16;
      u.nrow = 16 + BELOW[s] + 16 * (NBC[s] - 1 - c);
      u.off = off;
      u.dinv_off = doff;
      u.idx_off = gcol;
      u.pw = pw;
      u.cb = cb;
      u.gcol0 = gcol;
      off += (int64_t)u.nrow * u.w;
      doff += (int64_t)cb * cb;
      gcol += 16;
      P.units.push_back(u);
    }
  struct Step { int level; int64_t d0, dn, t0, tn; };
  std::vector<Step> steps;
  for (int lev = 0; lev <= 2; ++lev)
    for (int c = 0; c < 3; ++c) {
      Step st{lev, (int64_t)P.diag_list.size(), 0, (int64_t)P.tiles.size(), 0};
      for (int s = 0; s < NN; ++s) {
        if (LEVEL[s] != lev || c >= NBC[s]) continue;
        const int b = bcol0[(size_t)s] + c;
        P.diag_list.push_back(b);
        const int below = P.units[(size_t)b].nrow - P.units[(size_t)b].w;
        for (int t = 0; t * kSolveStripRows < below; ++t) P.tiles.push_back(UpdTile{b, (short)t, 0});
      }
      st.dn = (int64_t)P.diag_list.size() - st.d0;
      st.tn = (int64_t)P.tiles.size() - st.t0;
      if (st.dn > 0) steps.push_back(st);
    }
  for (const Step& st : steps) {
    P.fwd.push_back(SolveLaunch{SV_DIAG_FWD, st.level, st.d0, st.dn});
    if (st.tn > 0) P.fwd.push_back(SolveLaunch{SV_STRIP_FWD, st.level, st.t0, st.tn});
  }
  for (size_t i = steps.size(); i-- > 0;) {
    const Step& st = steps[i];
    if (st.tn > 0) P.bwd.push_back(SolveLaunch{SV_STRIP_BWD, st.level, st.t0, st.tn});
    P.bwd.push_back(SolveLaunch{SV_DIAG_BWD, st.level, st.d0, st.dn});
  }
  P.fwd_nsub = P.fwd.size();
}

struct Filtered {
  std::vector<SolveLaunch> launches;
  std::vector<int> list;
  std::vector<UpdTile> tiles;
  int64_t info[6] = {0, 0, 0, 0, 0, 0};
};

// the restatement: walk the launches of the sweep, keep the entries whose block column is in the set
void brute(const SolveProgram& P, bool bwd, const std::set<int>& set, Filtered& F) {
  for (const SolveLaunch& l : bwd ? P.bwd : P.fwd) {
    const bool diag = l.kind == SV_DIAG_FWD || l.kind == SV_DIAG_BWD;
    SolveLaunch out{l.kind, l.level, (int64_t)(diag ? F.list.size() : F.tiles.size()), 0};
    for (int64_t q = l.first; q < l.first + l.count; ++q) {
      const int b = diag ? P.diag_list[(size_t)q] : P.tiles[(size_t)q].unit;
      if (!set.count(b)) continue;
      if (diag) F.list.push_back(b); else F.tiles.push_back(P.tiles[(size_t)q]);
      ++out.count;
    }
    if (out.count > 0) F.launches.push_back(out);
  }
}

bool same(const Filtered& a, const Filtered& b) {
  if (a.launches.size() != b.launches.size() || a.list != b.list || a.tiles.size() != b.tiles.size()) return false;
  for (size_t i = 0; i < a.launches.size(); ++i)
    if (a.launches[i].kind != b.launches[i].kind || a.launches[i].level != b.launches[i].level ||
        a.launches[i].first != b.launches[i].first || a.launches[i].count != b.launches[i].count)
      return false;
  for (size_t i = 0; i < a.tiles.size(); ++i)
    if (a.tiles[i].unit != b.tiles[i].unit || a.tiles[i].ti != b.tiles[i].ti || a.tiles[i].tj != b.tiles[i].tj) return false;
  return true;
}

void run(const std::vector<int>& set) {
  SolveProgram wide, batch;
  std::vector<int> bcol0;
  build(256, 256, wide, bcol0);
  build(64, 64, batch, bcol0);
  const SolveSlots sw = build_solve_slots(wide), sb = build_solve_slots(batch);
  CHECK(sw.ok && sb.ok);
  CHECK(sw.entries == sb.entries && sw.bwd_wgs == sb.bwd_wgs);
  CHECK(sw.slot.size() == wide.units.size() && sb.slot.size() == batch.units.size());
  int64_t entries = 0, wgs = 0;
  for (const SolveUnit& u : wide.units) entries += (int64_t)u.nrow * u.w;
  for (const SolveLaunch& l : wide.bwd) wgs += l.count;
  CHECK(sw.entries == entries && sw.bwd_wgs == wgs);
  const std::set<int> want(set.begin(), set.end());
  for (int bwd = 0; bwd < 2; ++bwd) {
    Filtered fw, fb, ref;
    filter_solve_program(wide, sw.slot, bwd != 0, set, fw.launches, fw.list, fw.tiles, fw.info);
    filter_solve_program(batch, sb.slot, bwd != 0, set, fb.launches, fb.list, fb.tiles, fb.info);
    brute(batch, bwd != 0, want, ref);
    CHECK(same(fw, fb));          // the same block columns, launches and tiles from both programs
    CHECK(same(fb, ref));         // ... and they are the program's, in program order
    // every block column of the set once, its tiles one run (strip 0, 1, ...) equal to the program's run
    CHECK(std::set<int>(fb.list.begin(), fb.list.end()) == want && fb.list.size() == want.size());
    int64_t tiles = 0, ent = 0;
    for (int b : set) {
      const SolveBcolSlot& sl = sb.slot[(size_t)b];
      tiles += sl.tn;
      ent += (int64_t)batch.units[(size_t)b].nrow * batch.units[(size_t)b].w;
      const int below = batch.units[(size_t)b].nrow - batch.units[(size_t)b].w;
      CHECK(sl.tn == (below + kSolveStripRows - 1) / kSolveStripRows);
      for (int64_t q = 0; q < sl.tn; ++q)
        CHECK(batch.tiles[(size_t)(sl.t0 + q)].unit == b && batch.tiles[(size_t)(sl.t0 + q)].ti == q);
    }
    CHECK((int64_t)fb.tiles.size() == tiles);
    CHECK(fb.info[bwd ? 1 : 0] == (int64_t)set.size() && fb.info[bwd ? 0 : 1] == 0);
    CHECK(fb.info[bwd ? 3 : 2] == ent);
    CHECK(fb.info[5] == tiles + (int64_t)set.size());
    for (size_t i = 0; i < fb.tiles.size();) {   // a run per block column
      const int b = fb.tiles[i].unit;
      size_t j = i;
      for (; j < fb.tiles.size() && fb.tiles[j].unit == b; ++j) CHECK(fb.tiles[j].ti == (short)(j - i));
      CHECK((int64_t)(j - i) == sb.slot[(size_t)b].tn);
      i = j;
    }
  }
}

}  // namespace

int main() {
  const int nbc = 12;
  run({});
  run({0});
  run({nbc - 1});
  run({4});                      // no rows below its square: no strip launch holds it
  run({1, 2, 3, 10, 11});        // a path: a node of two block columns, its parent, the root
  run({0, 5, 6, 7, 8, 9});       // two branches
  std::vector<int> all;
  for (int b = 0; b < nbc; ++b) all.push_back(b);
  run(all);
  {
    // a program of another shape is found out: a block column in two diagonal launches; strips in two runs
    SolveProgram P;
    std::vector<int> bcol0;
    build(64, 64, P, bcol0);
    SolveProgram Q = P;
    Q.diag_list.push_back(0);
    Q.fwd.push_back(SolveLaunch{SV_DIAG_FWD, 3, (int64_t)Q.diag_list.size() - 1, 1});
    CHECK(!build_solve_slots(Q).ok);
    Q = P;
    Q.tiles.push_back(UpdTile{1, 0, 0});
    Q.fwd.push_back(SolveLaunch{SV_STRIP_FWD, 3, (int64_t)Q.tiles.size() - 1, 1});
    CHECK(!build_solve_slots(Q).ok);
    CHECK(build_solve_slots(P).ok);
  }
  if (fails) {
    std::printf("ss_filter_test: %d checks failed\n", fails);
    return 1;
  }
  std::printf("ss_filter_test: ok\n");
  return 0;
}
