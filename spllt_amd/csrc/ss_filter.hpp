// Filtering a substitution program to a set of block columns, host only and without a device
// (tests/native/ss_filter_test.cpp): where every block column sits in the launches of a SolveProgram, and the
// launches of one sweep that are left when only the block columns of a set are visited, with their entries
// compacted.  The single handle filters its own program (sprog_), the batch its own (bt_.sprog, pw = cb = 64): the
// launches of a program do not depend on the panel width, so both are filtered by this one implementation
// (DESIGN.md sections 16 and 29).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "schedule.hpp"

namespace spx {

// where block column b sits in the program: its launches of fwd / bwd (-1: no strips), its entry of diag_list
// and its tiles -- what filtering the program to a set of block columns walks
struct SolveBcolSlot {
  int fdiag = -1, fstrip = -1, bdiag = -1, bstrip = -1;
  int64_t dpos = 0, t0 = 0, tn = 0;
};

struct SolveSlots {
  std::vector<SolveBcolSlot> slot;   // per block column
  bool ok = true;                    // the program has the shape the slots assume (checked while they are built)
  int64_t entries = 0;               // doubles of L in all block columns
  int64_t bwd_wgs = 0;               // workgroups of the whole backward sweep
};

inline SolveSlots build_solve_slots(const SolveProgram& P) {
  SolveSlots S;
  S.slot.assign(P.units.size(), SolveBcolSlot{});
  for (const SolveUnit& u : P.units) S.entries += (int64_t)u.nrow * u.w;
  for (const SolveLaunch& l : P.bwd) S.bwd_wgs += l.count;
  for (int sweep = 0; sweep < 2; ++sweep) {
    const std::vector<SolveLaunch>& ls = sweep ? P.bwd : P.fwd;
    for (size_t i = 0; i < ls.size(); ++i) {
      const bool diag = ls[i].kind == SV_DIAG_FWD || ls[i].kind == SV_DIAG_BWD;
      for (int64_t q = ls[i].first; q < ls[i].first + ls[i].count; ++q) {
        SolveBcolSlot& sl = S.slot[(size_t)(diag ? P.diag_list[(size_t)q] : P.tiles[(size_t)q].unit)];
        // what the filter relies on: per sweep a block column sits in ONE diagonal launch, and its strips are one
        // run of consecutive tiles (strip 0, 1, ...) of ONE strip launch, the same run in both sweeps
        if (diag) {
          int& at = sweep ? sl.bdiag : sl.fdiag;
          if (at >= 0 || (sweep && sl.dpos != q)) S.ok = false;
          at = (int)i;
          sl.dpos = q;
        } else {
          int& at = sweep ? sl.bstrip : sl.fstrip;
          if (at >= 0 && at != (int)i) S.ok = false;
          at = (int)i;
          const int64_t ti = P.tiles[(size_t)q].ti;
          if (!sweep) {   // (the backward launches index the same tiles)
            if (sl.tn == 0) sl.t0 = q;
            if (q != sl.t0 + sl.tn || ti != sl.tn) S.ok = false;
            ++sl.tn;
          } else if (q < sl.t0 || q >= sl.t0 + sl.tn || ti != q - sl.t0) {
            S.ok = false;
          }
        }
      }
    }
  }
  return S;
}

// the launches of one sweep that hold a block column of `set` (ascending), appended to `out` with their entries
// compacted into list / tiles in program order; a launch left empty is dropped.  info (the fields of
// spllt_hip_solve_sparse_info): block columns [0] / [1] and entries of L [2] / [3] of the forward / backward
// sweep, workgroups [5].  Work: the set and its tiles, sorted.
inline void filter_solve_program(const SolveProgram& P, const std::vector<SolveBcolSlot>& slot, bool bwd,
                                 const std::vector<int>& set, std::vector<SolveLaunch>& out, std::vector<int>& list,
                                 std::vector<UpdTile>& tiles, int64_t info[6]) {
  struct Item { int launch; int64_t key; int b; };
  std::vector<Item> items;
  items.reserve(2 * set.size());
  for (int b : set) {
    const SolveBcolSlot& sl = slot[(size_t)b];
    const int ld = bwd ? sl.bdiag : sl.fdiag, ls = bwd ? sl.bstrip : sl.fstrip;
    if (ld >= 0) items.push_back({ld, sl.dpos, b});
    if (ls >= 0) items.push_back({ls, sl.t0, b});
  }
  std::sort(items.begin(), items.end(),
            [](const Item& a, const Item& b) { return a.launch != b.launch ? a.launch < b.launch : a.key < b.key; });
  const std::vector<SolveLaunch>& prog = bwd ? P.bwd : P.fwd;
  for (size_t i = 0; i < items.size();) {
    const SolveLaunch& src = prog[(size_t)items[i].launch];
    const bool diag = src.kind == SV_DIAG_FWD || src.kind == SV_DIAG_BWD;
    SolveLaunch l{src.kind, src.level, (int64_t)(diag ? list.size() : tiles.size()), 0};
    size_t j = i;
    for (; j < items.size() && items[j].launch == items[i].launch; ++j) {
      const SolveBcolSlot& sl = slot[(size_t)items[j].b];
      if (diag) {
        list.push_back(items[j].b);
        ++l.count;
        info[bwd ? 1 : 0] += 1;
        info[bwd ? 3 : 2] += (int64_t)P.units[(size_t)items[j].b].nrow * P.units[(size_t)items[j].b].w;
      } else {
        tiles.insert(tiles.end(), P.tiles.begin() + sl.t0, P.tiles.begin() + sl.t0 + sl.tn);
        l.count += sl.tn;
      }
    }
    out.push_back(l);
    info[5] += l.count;
    i = j;
  }
}

}  // namespace spx
