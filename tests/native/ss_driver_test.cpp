// Stand-alone check of ss_solve_sequence and ss_gram_sequence (ss_driver.hpp): a scripted backend records every
// step with its arguments and can refuse the take, fail the k-th upload / launch check / copy-out / sync or report
// "overflows a grid" from the k-th enqueue, gather or pair.  The expected traces below are written out from the
// sequence of the sparse right-hand-side family (DESIGN.md sections 16 and 29), not produced by the driver.  Host
// only; built and run by tests/test_ss_driver_cpu.py.
#include <cstdio>
#include <string>
#include <vector>

#include "ss_driver.hpp"

using namespace spx;

static int g_failed = 0;
#define CHECK(cond)                                                         \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);         \
      ++g_failed;                                                           \
    }                                                                       \
  } while (0)

using Trace = std::vector<std::string>;

// what the scripted steps report: 3 launches per enqueue, 1 per gather, 2 per pair; every group counts
// {1, 2, 3, 4, (99: never to be summed), 5} and stages 100 + nv bytes over kChunks chunks of rows
constexpr int kEnqueue = 3, kGather = 1, kPair = 2, kChunks = 2, kOverflow = -99;
constexpr size_t kOut = 1 << 15, kGram = 1 << 12, kW = 1 << 10;

struct Scripted {
  struct Group {
    int c0, nv, rb;
    std::vector<int> chunks;
    int64_t info[6];
    size_t bytes;
  };
  int n, members, cap;
  std::vector<double> w0 = std::vector<double>(kW), outbuf = std::vector<double>(kOut), gw = std::vector<double>(kGram),
                      caller = std::vector<double>(kOut);
  double* W0 = w0.data();
  SsState st;
  int take_rc = 0;
  int upload_fail_at = 0, check_fail_at = 0, copy_fail_at = 0, sync_fail_at = 0;   // the call (from 1) that fails with -30
  int enqueue_over_at = 0, gather_over_at = 0, pair_over_at = 0;                     // ... that overflows a grid
  Trace trace;
  int uploads = 0, checks = 0, copies = 0, syncs = 0, enqueues = 0, gathers = 0, pairs = 0, progressed = 0;
  int64_t left[6] = {-1, -1, -1, -1, -1, -1}, final_info[6] = {-1, -1, -1, -1, -1, -1};

  Scripted(int n, int members, int cap) : n(n), members(members), cap(cap) {}

  static std::string num(int64_t v) { return std::to_string(v); }
  std::string where(const double* p) const {
    if (p == W0) return "W0";
    if (p >= gw.data() && p < gw.data() + kGram) return "gramW+" + num(p - gw.data());
    if (p >= outbuf.data() && p < outbuf.data() + kOut) return "out+" + num(p - outbuf.data());
    if (p >= caller.data() && p < caller.data() + kOut) return "caller+" + num(p - caller.data());
    return "?";
  }
  void plan_rows(int k) { trace.push_back("plan_rows " + num(k)); }
  Group plan(int c0, int nv, int rb, int job, bool gram) {
    trace.push_back("plan " + num(c0) + " " + num(nv) + " " + num(rb) + " job" + num(job) + (gram ? " gram" : " solve"));
    return Group{c0, nv, rb, std::vector<int>(2 * kChunks, 0), {1, 2, 3, 4, 99, 5}, (size_t)(100 + nv)};
  }
  int take(size_t tab_bytes, size_t out_elems, size_t gram_elems) {
    trace.push_back("take " + num((int64_t)tab_bytes) + " " + num((int64_t)out_elems) + " " + num((int64_t)gram_elems));
    if (take_rc) return take_rc;
    st.out = outbuf.data();
    st.gramW = gw.data();
    return 0;
  }
  int upload(const Group& g) {
    trace.push_back("upload " + num(g.c0));
    return ++uploads == upload_fail_at ? -30 : 0;
  }
  int enqueue(const Group& g, int job, double* W) {
    trace.push_back("enqueue " + num(g.c0) + " job" + num(job) + " " + where(W));
    return ++enqueues == enqueue_over_at ? -1 : kEnqueue;
  }
  int gather(const Group& g, const SsSolveCall& c) {
    trace.push_back("gather " + num(g.c0) + (c.all ? " all" : " selected") + " nout" + num(c.nout));
    return ++gathers == gather_over_at ? -1 : kGather;
  }
  int pair(const Group& gi, const Group& gj, double* WI, double* WJ, int nchunk, double* part, bool diag, double* Gij,
           double* Gji, int64_t ld) {
    trace.push_back("pair " + num(gi.c0) + " " + num(gj.c0) + " " + where(WI) + " " + where(WJ) + " chunks" + num(nchunk) +
                    " part " + where(part) + (diag ? " diag " : " off ") + where(Gij) + " " + where(Gji) + " ld" + num(ld));
    return ++pairs == pair_over_at ? -1 : kPair;
  }
  int launch_check() {
    trace.push_back("check");
    return ++checks == check_fail_at ? -30 : 0;
  }
  int sync() {
    trace.push_back("sync");
    return ++syncs == sync_fail_at ? -30 : 0;
  }
  int copy_out(const Group& g, const SsSolveCall& c) {
    trace.push_back("copy_out " + num(g.c0) + " " + where(c.x) + " ldx" + num(c.ldx));
    return ++copies == copy_fail_at ? -30 : 0;
  }
  int copy_gram(double* G, double* gout, int64_t ldg, int k) {
    trace.push_back("copy_gram " + where(G) + " " + where(gout) + " ldg" + num(ldg) + " k" + num(k));
    return ++copies == copy_fail_at ? -30 : 0;
  }
  void progress(const int64_t info[6]) {
    ++progressed;
    for (int i = 0; i < 6; ++i) left[i] = info[i];
  }
  int overflow() {
    trace.push_back("overflow");
    return kOverflow;
  }
  int finish(const int64_t info[6]) {
    trace.push_back("finish");
    for (int i = 0; i < 6; ++i) final_info[i] = info[i];
    return 7;   // (the code of the call is the backend's)
  }
};

static bool same(const Trace& got, const Trace& want, const char* name) {
  bool ok = got.size() == want.size();
  for (size_t i = 0; ok && i < got.size(); ++i) ok = got[i] == want[i];
  if (!ok) {
    std::printf("trace '%s' differs:\n", name);
    for (size_t i = 0; i < std::max(got.size(), want.size()); ++i)
      std::printf("  %-3zu got  %s\n      want %s\n", i, i < got.size() ? got[i].c_str() : "-", i < want.size() ? want[i].c_str() : "-");
  }
  return ok;
}

static bool info_is(const int64_t got[6], std::vector<int64_t> want) {
  for (int i = 0; i < 6; ++i)
    if (got[i] != want[(size_t)i]) return false;
  return true;
}

static SsSolveCall solve_call(Scripted& be, int k, int job, bool all, bool dev) {
  const int64_t nout = all ? be.n : 3;
  return SsSolveCall{k, job, all, dev, be.caller.data(), dev ? 50 : 40, nout};
}

// ---- group cutting ----------------------------------------------------------------------------------------
struct Cut { int k, cap; Trace plans; };

static void test_group_cutting() {
  const std::vector<Cut> cuts = {
      {1, 32, {"plan 0 1 16 job0 solve"}},
      {16, 32, {"plan 0 16 16 job0 solve"}},
      {17, 32, {"plan 0 17 32 job0 solve"}},
      {32, 32, {"plan 0 32 32 job0 solve"}},
      {33, 32, {"plan 0 32 32 job0 solve", "plan 32 1 16 job0 solve"}},
      {48, 32, {"plan 0 32 32 job0 solve", "plan 32 16 16 job0 solve"}},
      {65, 32, {"plan 0 32 32 job0 solve", "plan 32 32 32 job0 solve", "plan 64 1 16 job0 solve"}},
      {33, 16, {"plan 0 16 16 job0 solve", "plan 16 16 16 job0 solve", "plan 32 1 16 job0 solve"}},
  };
  for (const Cut& c : cuts) {
    Scripted be(10, 1, c.cap);
    CHECK(ss_solve_sequence(be, solve_call(be, c.k, 0, true, true)) == 7);
    Trace plans;
    for (const std::string& s : be.trace)
      if (s.rfind("plan ", 0) == 0) plans.push_back(s);
    CHECK(same(plans, c.plans, ("cut k=" + std::to_string(c.k) + " cap=" + std::to_string(c.cap)).c_str()));
    CHECK(be.syncs == (int)c.plans.size() && be.uploads == be.syncs && be.progressed == be.syncs);
  }
  // the per-group step order, one group: a device caller (k = 1) and a host caller (k = 16)
  Scripted dev(10, 1, 32);
  CHECK(ss_solve_sequence(dev, solve_call(dev, 1, 0, true, true)) == 7);
  CHECK(same(dev.trace, {"plan 0 1 16 job0 solve", "take 101 0 0", "upload 0", "enqueue 0 job0 W0", "gather 0 all nout10",
                         "check", "sync", "finish"}, "k=1 device"));
  CHECK(info_is(dev.final_info, {1, 2, 3, 4, kEnqueue + kGather, 5}));
  Scripted host(10, 1, 32);
  CHECK(ss_solve_sequence(host, solve_call(host, 16, 0, true, false)) == 7);
  CHECK(same(host.trace, {"plan 0 16 16 job0 solve", "take 116 320 0", "upload 0", "enqueue 0 job0 W0",
                          "gather 0 all nout10", "check", "copy_out 0 caller+0 ldx40", "sync", "finish"}, "k=16 host"));
  CHECK(host.st.host_us >= 0);
}

// ---- solve ----------------------------------------------------------------------------------------------------
static void test_solve() {
  // two groups, a host caller, 2 members: every job, all entries and three selected rows
  for (int job = 0; job < 3; ++job)
    for (int all = 0; all < 2; ++all) {
      Scripted be(10, 2, 32);
      CHECK(ss_solve_sequence(be, solve_call(be, 33, job, all != 0, false)) == 7);
      const std::string j = "job" + std::to_string(job), g = all ? " all nout10" : " selected nout3";
      CHECK(same(be.trace,
                 {"plan 0 32 32 " + j + " solve", "plan 32 1 16 " + j + " solve",
                  all ? "take 132 640 0" : "take 132 192 0",   // (members * 32 * wanted entries)
                  "upload 0", "enqueue 0 " + j + " W0", "gather 0" + g, "check", "copy_out 0 caller+0 ldx40", "sync",
                  "upload 32", "enqueue 32 " + j + " W0", "gather 32" + g, "check", "copy_out 32 caller+0 ldx40", "sync",
                  "finish"},
                 ("solve host " + j + g).c_str()));
      CHECK(info_is(be.final_info, {2, 4, 6, 8, 2 * (kEnqueue + kGather), 10}));
      CHECK(info_is(be.left, {2, 4, 6, 8, 2 * (kEnqueue + kGather), 10}) && be.progressed == 2);
    }
  // a device caller: nothing taken for the outputs, nothing copied
  Scripted be(10, 2, 32);
  CHECK(ss_solve_sequence(be, solve_call(be, 33, 1, false, true)) == 7);
  CHECK(same(be.trace, {"plan 0 32 32 job1 solve", "plan 32 1 16 job1 solve", "take 132 0 0",
                        "upload 0", "enqueue 0 job1 W0", "gather 0 selected nout3", "check", "sync",
                        "upload 32", "enqueue 32 job1 W0", "gather 32 selected nout3", "check", "sync", "finish"},
             "solve device"));
}

// ---- gram -----------------------------------------------------------------------------------------------------
// n = 10, 2 members: a workspace of the groups after the first is 2 * 32 * 10 = 640 doubles
static void test_gram() {
  {   // one group, a host caller: G packed in the output buffer, the partial products behind it
    Scripted be(10, 2, 32);
    CHECK(ss_gram_sequence(be, 20, false, be.caller.data(), 25) == 7);
    CHECK(same(be.trace, {"plan_rows 20", "plan 0 20 32 job1 gram", "take 120 4896 0",   // 2 * 400 + 2 * 2 * 1024
                          "upload 0", "enqueue 0 job1 W0", "check", "sync",
                          "pair 0 0 W0 W0 chunks2 part out+800 diag out+0 out+0 ld20",
                          "check", "copy_gram out+0 caller+0 ldg25 k20", "sync", "finish"}, "gram 1 group"));
    CHECK(info_is(be.final_info, {1, 2, 3, 4, kEnqueue + kPair, 5}));
  }
  {   // two groups, a device caller with ldg > k: G is the caller's
    Scripted be(10, 2, 32);
    CHECK(ss_gram_sequence(be, 40, true, be.caller.data(), 50) == 7);
    CHECK(same(be.trace, {"plan_rows 40", "plan 0 32 32 job1 gram", "plan 32 8 16 job1 gram", "take 132 4096 640",
                          "upload 0", "enqueue 0 job1 W0", "check", "sync",
                          "upload 32", "enqueue 32 job1 gramW+0", "check", "sync",
                          "pair 0 0 W0 W0 chunks2 part out+0 diag caller+0 caller+0 ld50",
                          "pair 32 0 gramW+0 W0 chunks2 part out+0 off caller+32 caller+1600 ld50",
                          "pair 32 32 gramW+0 gramW+0 chunks2 part out+0 diag caller+1632 caller+1632 ld50",
                          "check", "sync", "finish"}, "gram 2 groups device"));
    CHECK(info_is(be.final_info, {2, 4, 6, 8, 2 * kEnqueue + 3 * kPair, 10}));
  }
  for (int dev = 0; dev < 2; ++dev) {   // three groups: packed (ld = k = 70) and in the caller's array (ldg = 80)
    Scripted be(10, 2, 32);
    CHECK(ss_gram_sequence(be, 70, dev != 0, be.caller.data(), 80) == 7);
    const std::string G = dev ? "caller+" : "out+", ld = dev ? " ld80" : " ld70";
    const std::string part = dev ? " chunks2 part out+0" : " chunks2 part out+9800";   // 2 * 70 * 70
    auto at = [&](int packed, int callers) { return G + std::to_string(dev ? callers : packed); };
    Trace want = {"plan_rows 70", "plan 0 32 32 job1 gram", "plan 32 32 32 job1 gram", "plan 64 6 16 job1 gram",
                  dev ? "take 132 4096 1280" : "take 132 13896 1280",
                  "upload 0", "enqueue 0 job1 W0", "check", "sync",
                  "upload 32", "enqueue 32 job1 gramW+0", "check", "sync",
                  "upload 64", "enqueue 64 job1 gramW+640", "check", "sync",
                  "pair 0 0 W0 W0" + part + " diag " + at(0, 0) + " " + at(0, 0) + ld,
                  "pair 32 0 gramW+0 W0" + part + " off " + at(32, 32) + " " + at(2240, 2560) + ld,
                  "pair 32 32 gramW+0 gramW+0" + part + " diag " + at(2272, 2592) + " " + at(2272, 2592) + ld,
                  "pair 64 0 gramW+640 W0" + part + " off " + at(64, 64) + " " + at(4480, 5120) + ld,
                  "pair 64 32 gramW+640 gramW+0" + part + " off " + at(2304, 2624) + " " + at(4512, 5152) + ld,
                  "pair 64 64 gramW+640 gramW+640" + part + " diag " + at(4544, 5184) + " " + at(4544, 5184) + ld,
                  "check"};
    if (!dev) want.push_back("copy_gram out+0 caller+0 ldg80 k70");
    want.push_back("sync");
    want.push_back("finish");
    CHECK(same(be.trace, want, dev ? "gram 3 groups device" : "gram 3 groups host"));
    CHECK(info_is(be.final_info, {3, 6, 9, 12, 3 * kEnqueue + 6 * kPair, 15}));
    CHECK(be.progressed == 4);   // (every group, and the pairs)
  }
}

// ---- failures ---------------------------------------------------------------------------------------------------
static void test_failures() {
  const Trace plans3 = {"plan 0 32 32 job0 solve", "plan 32 32 32 job0 solve", "plan 64 6 16 job0 solve"};
  const Trace group1 = {"upload 0", "enqueue 0 job0 W0", "gather 0 all nout10", "check", "copy_out 0 caller+0 ldx40", "sync"};
  auto cat = [](std::initializer_list<Trace> parts) {
    Trace t;
    for (const Trace& p : parts) t.insert(t.end(), p.begin(), p.end());
    return t;
  };
  {   // the take refuses: nothing is uploaded or enqueued
    Scripted be(10, 1, 32);
    be.take_rc = -1;
    CHECK(ss_solve_sequence(be, solve_call(be, 70, 0, true, false)) == -1);
    CHECK(same(be.trace, cat({plans3, {"take 132 320 0"}}), "take refuses"));
    CHECK(be.progressed == 0);
    Scripted gr(10, 1, 32);
    gr.take_rc = -1;
    CHECK(ss_gram_sequence(gr, 40, false, gr.caller.data(), 40) == -1);
    CHECK(same(gr.trace, {"plan_rows 40", "plan 0 32 32 job1 gram", "plan 32 8 16 job1 gram", "take 132 3648 320"},
               "gram take refuses"));
  }
  {   // the upload of group 2 of 3 fails: nothing is enqueued after it
    Scripted be(10, 1, 32);
    be.upload_fail_at = 2;
    CHECK(ss_solve_sequence(be, solve_call(be, 70, 0, true, false)) == -30);
    CHECK(same(be.trace, cat({plans3, {"take 132 320 0"}, group1, {"upload 32"}}), "upload fails"));
    CHECK(be.progressed == 1 && info_is(be.left, {1, 2, 3, 4, kEnqueue + kGather, 5}));   // (the completed group)
  }
  {   // the enqueue of group 2 overflows: no gather, no copy-out; the launch check and the sync still happen
    Scripted be(10, 1, 32);
    be.enqueue_over_at = 2;
    CHECK(ss_solve_sequence(be, solve_call(be, 70, 0, true, false)) == kOverflow);
    CHECK(same(be.trace, cat({plans3, {"take 132 320 0"}, group1, {"upload 32", "enqueue 32 job0 W0", "check", "sync", "overflow"}}),
               "enqueue overflows"));
    CHECK(be.progressed == 1);
  }
  {   // ... and the gather of group 2: no copy-out
    Scripted be(10, 1, 32);
    be.gather_over_at = 2;
    CHECK(ss_solve_sequence(be, solve_call(be, 70, 0, true, false)) == kOverflow);
    CHECK(same(be.trace, cat({plans3, {"take 132 320 0"}, group1,
                              {"upload 32", "enqueue 32 job0 W0", "gather 32 all nout10", "check", "sync", "overflow"}}),
               "gather overflows"));
  }
  {   // gram: the sweeps of group 2 overflow -- no pair is enqueued
    Scripted be(10, 1, 32);
    be.enqueue_over_at = 2;
    CHECK(ss_gram_sequence(be, 40, false, be.caller.data(), 40) == kOverflow);
    CHECK(same(be.trace, {"plan_rows 40", "plan 0 32 32 job1 gram", "plan 32 8 16 job1 gram", "take 132 3648 320",
                          "upload 0", "enqueue 0 job1 W0", "check", "sync",
                          "upload 32", "enqueue 32 job1 gramW+0", "check", "sync", "overflow"}, "gram sweep overflows"));
  }
  {   // gram: the second pair overflows -- no pair after it, no D2H; the sync happens
    Scripted be(10, 1, 32);
    be.pair_over_at = 2;
    CHECK(ss_gram_sequence(be, 40, false, be.caller.data(), 40) == kOverflow);
    CHECK(same(be.trace, {"plan_rows 40", "plan 0 32 32 job1 gram", "plan 32 8 16 job1 gram", "take 132 3648 320",
                          "upload 0", "enqueue 0 job1 W0", "check", "sync",
                          "upload 32", "enqueue 32 job1 gramW+0", "check", "sync",
                          "pair 0 0 W0 W0 chunks2 part out+1600 diag out+0 out+0 ld40",
                          "pair 32 0 gramW+0 W0 chunks2 part out+1600 off out+32 out+1280 ld40",
                          "check", "sync", "overflow"}, "pair overflows"));
  }
  {   // a failing copy-out, launch check or sync ends the sequence with its code
    Scripted be(10, 1, 32);
    be.copy_fail_at = 1;
    CHECK(ss_solve_sequence(be, solve_call(be, 70, 0, true, false)) == -30);
    CHECK(same(be.trace, cat({plans3, {"take 132 320 0", "upload 0", "enqueue 0 job0 W0", "gather 0 all nout10", "check",
                                       "copy_out 0 caller+0 ldx40"}}), "copy-out fails"));
    Scripted sy(10, 1, 32);
    sy.sync_fail_at = 2;
    CHECK(ss_solve_sequence(sy, solve_call(sy, 70, 0, true, false)) == -30);
    CHECK(same(sy.trace, cat({plans3, {"take 132 320 0"}, group1,
                              {"upload 32", "enqueue 32 job0 W0", "gather 32 all nout10", "check", "copy_out 32 caller+0 ldx40", "sync"}}),
               "sync fails"));
    CHECK(sy.progressed == 1);
    Scripted ck(10, 1, 32);
    ck.check_fail_at = 1;
    CHECK(ss_solve_sequence(ck, solve_call(ck, 70, 0, true, false)) == -30);
    CHECK(same(ck.trace, cat({plans3, {"take 132 320 0", "upload 0", "enqueue 0 job0 W0", "gather 0 all nout10", "check"}}),
               "launch check fails"));
    Scripted gc(10, 1, 32);   // gram, one group: the D2H of G is the first copy, the sync after it the second
    gc.copy_fail_at = 1;
    CHECK(ss_gram_sequence(gc, 20, false, gc.caller.data(), 20) == -30);
    CHECK(gc.trace.back() == "copy_gram out+0 caller+0 ldg20 k20");
    Scripted gs(10, 1, 32);
    gs.sync_fail_at = 2;
    CHECK(ss_gram_sequence(gs, 20, false, gs.caller.data(), 20) == -30);
    CHECK(gs.trace.back() == "sync" && gs.final_info[0] == -1);
  }
}

int main() {
  test_group_cutting();
  test_solve();
  test_gram();
  test_failures();
  if (g_failed) {
    std::printf("ss_driver_test: %d check(s) failed\n", g_failed);
    return 1;
  }
  std::printf("ss_driver_test: ok\n");
  return 0;
}
