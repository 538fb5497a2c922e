// The call sequence of the sparse right-hand-side family, once: solve_sparse / solve_sparse_batch and gram_sparse /
// gram_sparse_batch.  Host only: the driver cuts the columns into groups, orders the steps of a call and keeps the
// counters; a backend knows which substitution program, workspace and kernels a step runs on (engine_solve.cpp:
// Engine::SsHandleBackend, Engine::SsBatchBackend; tests/native/ss_driver_test.cpp: a scripted one that records the
// sequence).
//
// What a backend has.  Data: n, members (single handle: 1), cap (widest group: 16 or 32), W0 (the workspace of the
// first group), st (an SsState), and a type Group with c0, nv, rb, chunks, info[6] and bytes.  Steps:
//
//   void  plan_rows(k)                          gram: the rows any column of the call touches, once
//   Group plan(c0, nv, rb, job, gram)           plan, filter and stage one group (host only)
//   int   take(tab_bytes, out_elems, gram_elems)   all device memory of the call; 0 or the code of the call
//   int   upload(g)                             the tables of g (the stream is idle)
//   int   enqueue(g, job, W)                    zero, scatter and the filtered sweeps on W; launches made
//   int   gather(g, c)                          the wanted entries of W0 to the caller or the output buffer; launches
//   int   pair(gI, gJ, WI, WJ, nchunk, part, diag, Gij, Gji, ld)   product and reduce of one pair; launches made
//   int   launch_check() / sync()
//   int   copy_out(g, c) / copy_gram(G, gout, ldg, k)   to a host caller
//   void  progress(info)                        after every group and after the pairs: what a failed call leaves
//   int   overflow()                            the code of a launch that does not fit a grid, its message set
//   int   finish(info)                          the counters of the call; its code
//
// A step that launches returns a negative count when a launch would overflow a grid (the batch only).  Then nothing
// further is enqueued and nothing is copied to the host; the launch check and the sync still happen, and the call
// returns overflow().  Counter 4 (launches) is what the steps report; 0-3 and 5 are summed from the groups.
#pragma once
#include <algorithm>
#include <chrono>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "engine_detail.hpp"

namespace spx {

// the storage and the readers' values of one owner of the family (the handle, the batch): the staged tables of one
// group, the gathered entries / G / partial products, gram's workspaces of the groups after the first
struct SsState {
  char* tab = nullptr;
  double* out = nullptr;
  double* gramW = nullptr;
  size_t tab_cap = 0, out_cap = 0, gram_cap = 0;   // bytes, doubles, doubles
  int64_t info[8] = {0, 0, 0, 0, 0, 0, 0, 0};      // (6 and 7: the batch's members served and flagged)
  int64_t host_us = 0;                              // planning, before the first device call
};

struct SsSolveCall {
  int k, job;
  bool all, dev;     // every entry wanted / x is on the device
  double* x;
  int64_t ldx, nout;
};

constexpr size_t kSsPartial = 1024;   // doubles of partial products per chunk of rows (and member): a 32 x 32 block

using SsClock = std::chrono::steady_clock;

// the groups of k columns, planned by plan(c0, nv, rb); returns the bytes of the largest group's tables and
// records the host time since t0
template <class Backend, class Plan>
size_t ss_plan_groups(Backend& be, int k, SsClock::time_point t0, std::vector<typename Backend::Group>& groups,
                      Plan&& plan) {
  size_t tab_bytes = 0;
  for_each_block(k, be.cap, [&](int c0, int nv, int rb) {
    groups.push_back(plan(c0, nv, rb));
    tab_bytes = std::max(tab_bytes, groups.back().bytes);
    return 0;
  });
  be.st.host_us = std::chrono::duration_cast<std::chrono::microseconds>(SsClock::now() - t0).count();
  return tab_bytes;
}

// One group on workspace W: upload, enqueue, (c: gather), launch check, (c, host caller: copy-out), sync -- the
// next group reuses the tables -- and the counters.  c: the solve the group belongs to, null for gram's sweeps.
template <class Backend>
int ss_run_group(Backend& be, const typename Backend::Group& g, int job, double* W, const SsSolveCall* c,
                 int64_t info[6]) {
  int rc = be.upload(g);
  if (rc) return rc;
  int made = be.enqueue(g, job, W);
  if (c && made >= 0) {
    const int out = be.gather(g, *c);
    made = out < 0 ? -1 : made + out;
  }
  if ((rc = be.launch_check())) return rc;
  if (c && made >= 0 && !c->dev && (rc = be.copy_out(g, *c))) return rc;
  if ((rc = be.sync())) return rc;
  if (made < 0) return be.overflow();
  for (int i = 0; i < 6; ++i) info[i] += i == 4 ? made : g.info[i];
  be.progress(info);
  return 0;
}

// X = the wanted entries of A^-1 B (job 0), L^-1 B (1) or L^-T B (2), group by group on the first workspace
template <class Backend>
int ss_solve_sequence(Backend& be, const SsSolveCall& c) {
  std::vector<typename Backend::Group> groups;
  const size_t tab_bytes = ss_plan_groups(be, c.k, SsClock::now(), groups,
                                          [&](int c0, int nv, int rb) { return be.plan(c0, nv, rb, c.job, false); });
  int rc = be.take(tab_bytes, c.dev ? 0 : (size_t)be.members * 32 * (size_t)c.nout, 0);
  if (rc) return rc;
  int64_t info[6] = {0, 0, 0, 0, 0, 0};
  for (const auto& g : groups)
    if ((rc = ss_run_group(be, g, c.job, be.W0, &c, info))) return rc;
  return be.finish(info);
}

// G = B^T A^-1 B: the forward sweeps of every group into a workspace of its own, then the products of the pairs of
// groups over the rows any column touches.  G: gout on the device, else the output buffer (packed, ld = k).
template <class Backend>
int ss_gram_sequence(Backend& be, int k, bool dev, double* gout, int64_t ldg) {
  std::vector<typename Backend::Group> groups;
  const auto t0 = SsClock::now();
  be.plan_rows(k);
  const size_t tab_bytes =
      ss_plan_groups(be, k, t0, groups, [&](int c0, int nv, int rb) { return be.plan(c0, nv, rb, 1, true); });
  const size_t ng = groups.size(), nchunk = groups[0].chunks.size() / 2;
  const size_t wstride = (size_t)be.members * 32 * (size_t)be.n;
  const size_t g_elems = dev ? 0 : (size_t)be.members * (size_t)k * (size_t)k;
  int rc = be.take(tab_bytes, g_elems + (size_t)be.members * nchunk * kSsPartial, wstride * (ng - 1));
  if (rc) return rc;
  auto workspace = [&](size_t gi) { return gi == 0 ? be.W0 : be.st.gramW + (gi - 1) * wstride; };
  int64_t info[6] = {0, 0, 0, 0, 0, 0};
  for (size_t gi = 0; gi < ng; ++gi)
    if ((rc = ss_run_group(be, groups[gi], 1, workspace(gi), nullptr, info))) return rc;
  // (the chunk list of the last group, the same in every group, is still in the tables)
  double* G = dev ? gout : be.st.out;
  const int64_t ld = dev ? ldg : (int64_t)k;
  double* part = be.st.out + g_elems;
  bool fits = true;
  for (size_t I = 0; I < ng && fits; ++I)
    for (size_t J = 0; J <= I && fits; ++J) {
      const auto &gi = groups[I], &gj = groups[J];
      const int made = be.pair(gi, gj, workspace(I), workspace(J), (int)nchunk, part, I == J,
                               G + (int64_t)gj.c0 * ld + gi.c0, G + (int64_t)gi.c0 * ld + gj.c0, ld);
      if (made < 0) fits = false;
      else info[4] += made;
    }
  be.progress(info);
  if ((rc = be.launch_check())) return rc;
  if (fits && !dev && (rc = be.copy_gram(G, gout, ldg, k))) return rc;
  if ((rc = be.sync())) return rc;
  return fits ? be.finish(info) : be.overflow();
}

}  // namespace spx
