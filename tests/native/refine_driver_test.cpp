// Stand-alone check of refine_iterate (refine_driver.hpp): a scripted backend records every operation with its
// arguments, serves the read-backs from a list of state vectors and can fail the k-th apply_factor / read-back or
// report "does not fit" from the k-th launch on.  The expected traces below are written out from the sequence of
// the refined solves, not produced by the driver.  Host only; built and run by
// tests/test_refine_driver_cpu.py.
#include <algorithm>
#include <cstdio>
#include <initializer_list>
#include <string>
#include <vector>

#include "refine_driver.hpp"

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
using States = std::vector<std::vector<int>>;   // one state per pair and read-back

constexpr int kVslots = 7, kSslots = 11;

struct Scripted {
  int np, out_stride;
  States states;
  int fail_factor_at = 0, fail_factor_with = 0;     // the apply_factor (from 1) that fails; 0: none
  int fail_readback_at = 0, fail_readback_with = 0;
  int unfit_at = 0;                                 // the launch (from 1) that does not fit; 0: none
  Trace trace;
  int launches = 0, factors = 0, readbacks = 0;
  bool fit = true;

  static const char* vec(RfVec v) {
    static const char* names[] = {"-", "B", "X", "R", "P", "Q", "XB"};
    return names[v + 1];
  }
  static const char* selector(RfSel s) {
    static const char* names[] = {"all", "st", "decl", "improve"};
    return names[s];
  }
  static const char* stage(int s) {
    static const char* names[] = {"AMAX", "BNORM", "TRUE", "ALPHA", "REC", "BETA", "FINAL"};
    return names[s];
  }
  void launch(const std::string& what) {
    trace.push_back(what);
    if (++launches == unfit_at) fit = false;
  }
  static std::string num(int k) { return std::to_string(k); }

  int pairs() const { return np; }
  int stride() const { return out_stride; }
  int vslots() const { return kVslots; }
  int sslots() const { return kSslots; }
  bool fits() const { return fit; }
  int permute_in() {
    launch("permute_in");
    return 0;
  }
  void dot(RfVec a, RfVec b, RfSel s, int want, bool residual_like) {
    launch(std::string("dot ") + vec(a) + " " + vec(b) + " " + selector(s) + " " + num(want) + (residual_like ? " reslike" : " plain"));
  }
  void finalize(int st, int nslots, int flag) { launch(std::string("finalize ") + stage(st) + " " + num(nslots) + " " + num(flag)); }
  void copy(RfVec dst, RfVec src, RfSel s, int want, bool zero_others) {
    launch(std::string("copy ") + vec(dst) + " " + vec(src) + " " + selector(s) + " " + num(want) + (zero_others ? " zero" : " keep"));
  }
  int apply_factor(RfVec v) {
    trace.push_back(std::string("apply_factor ") + vec(v));
    return ++factors == fail_factor_at ? fail_factor_with : 0;
  }
  void spmv(RfVec x, RfVec b, RfVec y, RfSel s, int want, bool partials) {
    launch(std::string("spmv ") + vec(x) + " " + vec(b) + " " + vec(y) + " " + selector(s) + " " + num(want) + (partials ? " part" : " nopart"));
  }
  void axpy(bool alpha, RfVec x, RfVec p, RfVec r, RfVec q, RfSel s, int want, bool partials) {
    launch(std::string("axpy ") + (alpha ? "alpha " : "one ") + vec(x) + " " + vec(p) + " " + vec(r) + " " + vec(q) + " " + selector(s) +
           " " + num(want) + (partials ? " part" : " nopart"));
  }
  void pupdate(RfVec p, RfVec z, RfSel s, int want) {
    launch(std::string("pupdate ") + vec(p) + " " + vec(z) + " " + selector(s) + " " + num(want));
  }
  int readback(std::vector<double>& out) {
    trace.push_back("readback");
    if (++readbacks == fail_readback_at) return fail_readback_with;
    CHECK((size_t)readbacks <= states.size());
    CHECK(out.size() == 2 * (size_t)out_stride);
    if ((size_t)readbacks > states.size() || out.size() != 2 * (size_t)out_stride) return -1000;
    for (int g = 0; g < np; ++g) {
      out[(size_t)g] = 100.0 * readbacks + g;   // (the "error" of pair g at this read-back)
      out[(size_t)out_stride + g] = states[(size_t)readbacks - 1][(size_t)g];
    }
    return 0;
  }
  int permute_out(RfVec src) {
    launch(std::string("permute_out ") + vec(src));
    return 0;
  }
  int finish() {
    trace.push_back("finish");
    return fit ? 0 : -99;
  }
};

// ---- the sequence, written out ------------------------------------------------------------------------------
static const Trace kPrologue = {"permute_in",
                                "dot B B all 0 reslike",
                                "finalize BNORM 7 0",
                                "copy X B all 0 keep",
                                "apply_factor X",
                                "spmv X B R st 0 part",
                                "finalize TRUE 11 0",
                                "copy XB X improve 1 keep",
                                "readback"};
static const Trace kIrStep = {"copy P R st 0 zero",
                              "apply_factor P",
                              "axpy one X P - - st 0 nopart",
                              "spmv X B R st 0 part",
                              "finalize TRUE 11 0",
                              "copy XB X improve 1 keep",
                              "readback"};
static const Trace kPcgStep = {"copy Q R st 0 zero",
                               "apply_factor Q",
                               "dot R Q st 0 plain",
                               "finalize BETA 7 0",
                               "pupdate P Q st 0",
                               "spmv P - Q st 0 part",
                               "finalize ALPHA 11 0",
                               "axpy alpha X P R Q st 0 part",
                               "finalize REC 7 0",
                               "spmv X B R decl 1 part",
                               "finalize TRUE 11 1",
                               "copy XB X improve 1 keep",
                               "readback"};
static const Trace kEpilogue = {"finalize FINAL 0 0", "spmv X B R decl 1 part", "finalize TRUE 11 1", "copy XB X improve 1 keep",
                                "readback"};
static const Trace kEnd = {"permute_out XB", "finish"};

static Trace cat(std::initializer_list<Trace> parts) {
  Trace t;
  for (const Trace& p : parts) t.insert(t.end(), p.begin(), p.end());
  return t;
}

static void expect_trace(const char* name, const Trace& got, const Trace& want) {
  bool same = got.size() == want.size();
  for (size_t i = 0; same && i < got.size(); ++i) same = got[i] == want[i];
  if (same) return;
  ++g_failed;
  std::printf("FAILED %s: the trace differs\n", name);
  for (size_t i = 0; i < std::max(got.size(), want.size()); ++i)
    std::printf("  %2zu  %-34s | %s\n", i, i < got.size() ? got[i].c_str() : "", i < want.size() ? want[i].c_str() : "");
}

struct Result {
  int rc;
  std::vector<int> its;
  std::vector<double> out;
  Trace trace;
};
static Result run(Scripted be, int method, int max_iter) {
  Result r;
  r.rc = refine_iterate(be, method, max_iter, r.its, r.out);
  r.trace = be.trace;
  return r;
}
// np = 1 reads back like the single handle (stride RF_G), np = 4 = 2 members x 2 vectors like a pass (stride np)
static Scripted backend(int np, States states) { return Scripted{np, np == 1 ? RF_G : np, std::move(states)}; }
static States rows(int np, std::vector<int> first_pair, std::vector<int> other_pairs) {
  States s;
  for (size_t k = 0; k < first_pair.size(); ++k) {
    std::vector<int> row((size_t)np, other_pairs[k]);
    row[0] = first_pair[k];
    s.push_back(row);
  }
  return s;
}

static void test_converged_at_once(int np) {
  for (int method = 0; method < 2; ++method) {
    const Result r = run(backend(np, {std::vector<int>((size_t)np, 1)}), method, 10);
    CHECK(r.rc == 0);
    expect_trace("converged at once", r.trace, cat({kPrologue, kEnd}));
    CHECK(r.its == std::vector<int>((size_t)np, 0));
    CHECK(r.out[0] == 100.0 && r.out[(size_t)(np == 1 ? RF_G : np)] == 1.0);
  }
}

static void test_ir(int np) {
  if (np == 1) {
    // one pair: converged after step 1; or after step 2 in state 2
    Result r = run(backend(1, {{0}, {1}}), 0, 10);
    CHECK(r.rc == 0);
    expect_trace("ir, one pair, one step", r.trace, cat({kPrologue, kIrStep, kEnd}));
    CHECK(r.its == std::vector<int>{1});
    r = run(backend(1, {{0}, {0}, {2}}), 0, 10);
    CHECK(r.rc == 0);
    expect_trace("ir, one pair, two steps", r.trace, cat({kPrologue, kIrStep, kIrStep, kEnd}));
    CHECK(r.its == std::vector<int>{2});
    CHECK(r.out[(size_t)RF_G] == 2.0);
    return;
  }
  // pair 0 converges after step 1, the others after step 2, pair 2 in state 2
  States s = rows(np, {0, 1, 1}, {0, 0, 1});
  s[2][2] = 2;
  const Result r = run(backend(np, s), 0, 10);
  CHECK(r.rc == 0);
  expect_trace("ir, two steps", r.trace, cat({kPrologue, kIrStep, kIrStep, kEnd}));
  CHECK((r.its == std::vector<int>{1, 2, 2, 2}));
  CHECK(r.out[0] == 300.0 && r.out[(size_t)np + 2] == 2.0 && r.out[(size_t)np + 3] == 1.0);
}

static void test_pcg_runs_out(int np) {
  const States s(4, std::vector<int>((size_t)np, 0));   // prologue, two steps, epilogue: never converging
  const Result r = run(backend(np, s), 1, 2);
  CHECK(r.rc == 0);
  expect_trace("pcg, out of iterations", r.trace, cat({kPrologue, kPcgStep, kPcgStep, kEpilogue, kEnd}));
  CHECK(r.its == std::vector<int>((size_t)np, 2));
  CHECK(r.out[0] == 400.0);   // (of the read-back of the epilogue)
}

static void test_pcg_frozen_pairs(int np) {
  // a pair that converged at step 1 keeps its count; the epilogue runs for the one that is left
  if (np == 1) return;
  const Result r = run(backend(np, rows(np, {0, 0, 0, 0}, {0, 1, 1, 1})), 1, 2);
  CHECK(r.rc == 0);
  expect_trace("pcg, one pair left", r.trace, cat({kPrologue, kPcgStep, kPcgStep, kEpilogue, kEnd}));
  CHECK((r.its == std::vector<int>{2, 1, 1, 1}));
}

static void test_no_iterations(int np) {
  const States s(2, std::vector<int>((size_t)np, 0));
  Result r = run(backend(np, s), 1, 0);
  CHECK(r.rc == 0);
  expect_trace("pcg, max_iter 0", r.trace, cat({kPrologue, kEpilogue, kEnd}));
  CHECK(r.its == std::vector<int>((size_t)np, 0));
  r = run(backend(np, s), 0, 0);
  CHECK(r.rc == 0);
  expect_trace("ir, max_iter 0", r.trace, cat({kPrologue, kEnd}));
  CHECK(r.its == std::vector<int>((size_t)np, 0));
}

static void test_failing_calls(int np) {
  const States s(3, std::vector<int>((size_t)np, 0));
  // the second apply_factor is the one of step 1
  Scripted be = backend(np, s);
  be.fail_factor_at = 2;
  be.fail_factor_with = -3;
  Result r = run(be, 0, 5);
  CHECK(r.rc == -3);
  expect_trace("ir, apply_factor fails", r.trace, cat({kPrologue, {"copy P R st 0 zero", "apply_factor P"}}));
  r = run(be, 1, 5);
  CHECK(r.rc == -3);
  expect_trace("pcg, apply_factor fails", r.trace, cat({kPrologue, {"copy Q R st 0 zero", "apply_factor Q"}}));
  // the first one: nothing after it
  be.fail_factor_at = 1;
  r = run(be, 1, 5);
  CHECK(r.rc == -3);
  expect_trace("apply_factor of the first iterate fails", r.trace,
               {"permute_in", "dot B B all 0 reslike", "finalize BNORM 7 0", "copy X B all 0 keep", "apply_factor X"});
  // a read-back that fails ends the driver as well (the second: that of step 1)
  be = backend(np, s);
  be.fail_readback_at = 2;
  be.fail_readback_with = -30;
  r = run(be, 0, 5);
  CHECK(r.rc == -30);
  expect_trace("ir, read-back fails", r.trace, cat({kPrologue, kIrStep}));
}

static void test_does_not_fit(int np) {
  const States s(3, std::vector<int>((size_t)np, 0));
  // launches of the prologue: permute_in, dot, finalize, copy, spmv, finalize, copy = 7.  The first product of step 1
  // is launch 10 under refinement (copy, axpy, spmv) and 12 under PCG (copy, dot, finalize, pupdate, spmv): the
  // step is finished, no further step and no epilogue follow, the pass reports -99 once the stream is idle
  Scripted be = backend(np, s);
  be.unfit_at = 10;
  Result r = run(be, 0, 5);
  CHECK(r.rc == -99);
  expect_trace("ir, does not fit", r.trace, cat({kPrologue, kIrStep, kEnd}));
  be.unfit_at = 12;
  r = run(be, 1, 5);
  CHECK(r.rc == -99);
  expect_trace("pcg, does not fit", r.trace, cat({kPrologue, kPcgStep, kEnd}));
  // in front of the first iterate: no sweep on vectors that were not written
  be.unfit_at = 1;
  r = run(be, 1, 5);
  CHECK(r.rc == -99);
  expect_trace("does not fit from the first launch", r.trace,
               {"permute_in", "dot B B all 0 reslike", "finalize BNORM 7 0", "copy X B all 0 keep", "finish"});
}

int main() {
  for (int np : {1, 4}) {
    test_converged_at_once(np);
    test_ir(np);
    test_pcg_runs_out(np);
    test_pcg_frozen_pairs(np);
    test_no_iterations(np);
    test_failing_calls(np);
    test_does_not_fit(np);
  }
  if (g_failed) {
    std::printf("refine_driver_test: %d check(s) failed\n", g_failed);
    return 1;
  }
  std::printf("refine_driver_test: ok\n");
  return 0;
}
