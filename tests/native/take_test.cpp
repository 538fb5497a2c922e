// Stand-alone check of the feature-memory helpers of engine_detail.hpp (Take, give_back, grow, Shared, the
// allocation hooks) against a counting allocator on malloc / free that fails at a chosen call.  Host only: the two
// HIP entry points the header uses are defined here.  Built and run by tests/test_take_cpu.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "engine_detail.hpp"

static int g_cleared = 0;   // calls of hipGetLastError
extern "C" hipError_t hipGetLastError(void) { ++g_cleared; return hipSuccess; }
extern "C" hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind) {
  std::memcpy(dst, src, bytes);
  return hipSuccess;
}

using namespace spx;

static int g_failed = 0;
#define CHECK(cond)                                                         \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);         \
      ++g_failed;                                                           \
    }                                                                       \
  } while (0)

struct Heap {
  int calls = 0, fail_at = 0;       // fail_at: the call (from 1) that returns "out of memory"; 0: none
  hipError_t fail_with = hipErrorOutOfMemory;
  std::vector<void*> live, released;   // in the order of the calls
};
struct FakeAlloc {
  Heap* h;
  hipError_t operator()(void** p, size_t bytes) const {
    if (++h->calls == h->fail_at) return h->fail_with;
    *p = std::malloc(bytes);
    h->live.push_back(*p);
    return hipSuccess;
  }
};
struct FakeRelease {
  Heap* h;
  void operator()(void* p) const {
    bool found = false;
    for (size_t i = 0; i < h->live.size(); ++i)
      if (h->live[i] == p) { h->live.erase(h->live.begin() + (long)i); found = true; break; }
    CHECK(found);   // released once, and only what was taken
    if (found) std::free(p);
    h->released.push_back(p);
  }
};
using TestTake = Take<FakeAlloc, FakeRelease>;

static void test_commit() {
  Heap h;
  double* a = nullptr;
  int* b = nullptr;
  {
    TestTake t(FakeAlloc{&h}, FakeRelease{&h});
    t(&a, 64);
    t.block(&b, 32);
    t.check(hipSuccess);
    CHECK(t.ok() && t.error() == hipSuccess && t.bytes() == 96);
    t.commit();
  }
  CHECK(a && b && h.live.size() == 2 && h.released.empty());
  give_back(FakeRelease{&h}, a, b);
  CHECK(!a && !b && h.live.empty());
}

// the roll-back: what the transaction took goes back last first, its pointers are null, the others untouched
static void test_rollback(int fail_at) {
  Heap h;
  h.fail_at = fail_at;
  double* held = (double*)std::malloc(8);   // held before the call: not the transaction's
  double* const held0 = held;
  double *a = nullptr, *b = nullptr, *c = nullptr;
  void *pa = nullptr, *pb = nullptr;
  const int cleared = g_cleared;
  {
    TestTake t(FakeAlloc{&h}, FakeRelease{&h});
    t(&a, 16);
    pa = a;
    t(&b, 16);
    pb = b;
    t(&c, 16);
    CHECK(!t.ok() && t.error() == hipErrorOutOfMemory);
    CHECK(t.bytes() == 48);                     // every request, made or skipped
    CHECK(h.calls == fail_at);                  // nothing is asked for after the failure
    t.check(hipErrorInvalidValue);
    CHECK(t.error() == hipErrorOutOfMemory);    // the first error stays
    t.commit();                                 // (of a failed transaction: nothing)
  }
  CHECK(!a && !b && !c && held == held0);
  CHECK(h.live.empty() && (int)h.released.size() == fail_at - 1);
  if (fail_at == 3) CHECK(h.released[0] == pb && h.released[1] == pa);
  CHECK(g_cleared == cleared + 1);              // the sticky error is cleared once
  std::free(held);
}

// any other error joins the outcome; leaving without commit rolls a transaction without error back too
static void test_check_and_abandon() {
  Heap h;
  double *a = nullptr, *b = nullptr;
  {
    TestTake t(FakeAlloc{&h}, FakeRelease{&h});
    t(&a, 8);
    t.check(hipErrorInvalidValue);
    t(&b, 8);
    CHECK(!t.ok() && t.error() == hipErrorInvalidValue && h.calls == 1);
  }
  CHECK(!a && !b && h.live.empty());
  {
    TestTake t(FakeAlloc{&h}, FakeRelease{&h});
    t(&a, 8);
    CHECK(t.ok());
  }
  CHECK(!a && h.live.empty());
}

static void test_tables() {
  const std::vector<int> x{1, 2, 3};
  const std::vector<double> y{4.0, 5.0};
  for (int fail_at = 0; fail_at <= 2; ++fail_at) {
    Heap h;
    h.fail_at = fail_at;
    char* blob = nullptr;
    int* dx = nullptr;
    double *dy = nullptr, *w = nullptr;
    {
      TableStager tab;
      tab.add(&dx, x);
      tab.add(&dy, y);
      TestTake t(FakeAlloc{&h}, FakeRelease{&h});
      t.tables(tab, &blob);
      t(&w, 8);
      if (fail_at == 0) {
        CHECK(t.ok() && dx && dy && dx[2] == 3 && dy[1] == 5.0 && (char*)dx == blob && (char*)dy == blob + 256);
        t.commit();
      } else {
        CHECK(!t.ok());
      }
    }
    if (fail_at == 0) {
      CHECK(blob && w && h.live.size() == 2);
      give_back(FakeRelease{&h}, blob, w);
    } else {
      CHECK(!blob && !dx && !dy && !w);   // the typed pointers into the blob are rolled back too
    }
    CHECK(h.live.empty());
  }
}

// the width fallback as the engine writes it: one Take per width, "out of memory" alone tries the next width
static hipError_t take_widths(Heap& h, double** w, double** s, int* rb) {
  for (*rb = 32;; *rb /= 2) {
    TestTake t(FakeAlloc{&h}, FakeRelease{&h});
    t.block(w, 8 * (size_t)*rb);
    t.block(s, 4 * (size_t)*rb);
    t.commit();
    if (t.ok() || *rb == 16 || alloc_code(t.error()) != -1) return t.error();
  }
}

static void test_width_retry() {
  double *w = nullptr, *s = nullptr;
  int rb = 0;
  {
    Heap h;
    h.fail_at = 2;   // the scratch at 32
    CHECK(take_widths(h, &w, &s, &rb) == hipSuccess && rb == 16 && w && s && h.calls == 4 && h.live.size() == 2);
    give_back(FakeRelease{&h}, w, s);
  }
  {
    Heap h;
    h.fail_at = 1;
    h.fail_with = hipErrorInvalidValue;   // not "out of memory": no second width
    CHECK(take_widths(h, &w, &s, &rb) == hipErrorInvalidValue && rb == 32 && !w && !s && h.calls == 1);
  }
  {
    Heap h;   // the hook of the blocked paths: the first block() of either width fails, the allocator is not asked
    fmult_alloc_fail_left().store(2);
    CHECK(take_widths(h, &w, &s, &rb) == hipErrorOutOfMemory && rb == 16 && !w && !s && h.calls == 0 && h.live.empty());
    CHECK(fmult_alloc_fail_left().load() == 0);
  }
}

static void test_hooks() {
  Heap h;
  double *a = nullptr, *b = nullptr;
  alloc_fail_countdown().store(2);
  {
    TestTake t(FakeAlloc{&h}, FakeRelease{&h});
    t(&a, 8);
    CHECK(t.ok() && alloc_fail_countdown().load() == 1);
    t(&b, 8);
    CHECK(!t.ok() && t.error() == hipErrorOutOfMemory && h.calls == 1);
  }
  CHECK(alloc_fail_countdown().load() == 0 && h.live.empty());   // fired once, disarmed
  {
    TestTake t(FakeAlloc{&h}, FakeRelease{&h});
    t(&a, 8);
    t.commit();
  }
  CHECK(a);
  give_back(FakeRelease{&h}, a);
  // grow counts too
  size_t have = 0;
  alloc_fail_countdown().store(1);
  CHECK(grow(FakeAlloc{&h}, FakeRelease{&h}, &a, &have, 4) == hipErrorOutOfMemory && !a && have == 0);
  CHECK(alloc_fail_countdown().load() == 0);
}

static void test_grow() {
  Heap h;
  double* p = nullptr;
  size_t have = 0;
  CHECK(grow(FakeAlloc{&h}, FakeRelease{&h}, &p, &have, 4) == hipSuccess && p && have == 4 && h.calls == 1);
  double* const first = p;
  p[3] = 1.0;
  CHECK(grow(FakeAlloc{&h}, FakeRelease{&h}, &p, &have, 3) == hipSuccess && p == first && h.calls == 1);   // kept
  CHECK(grow(FakeAlloc{&h}, FakeRelease{&h}, &p, &have, 9) == hipSuccess && have == 9 && h.calls == 2);
  CHECK(h.released.size() == 1 && h.released[0] == first && h.live.size() == 1);
  p[8] = 1.0;
  h.fail_at = 3;
  CHECK(grow(FakeAlloc{&h}, FakeRelease{&h}, &p, &have, 20) == hipErrorOutOfMemory && !p && have == 0 && h.live.empty());
  CHECK(grow(FakeAlloc{&h}, FakeRelease{&h}, &p, &have, 0) == hipSuccess && p && have == 0);   // (no empty allocation)
  give_back(FakeRelease{&h}, p);
  CHECK(h.live.empty());
}

static void test_give_back() {
  Heap h;
  double* a = nullptr;
  int* b = nullptr;
  char* c = nullptr;
  CHECK(FakeAlloc{&h}((void**)&a, 8) == hipSuccess);
  CHECK(FakeAlloc{&h}((void**)&c, 8) == hipSuccess);
  give_back(FakeRelease{&h}, a, b, c);   // (b is null: skipped)
  CHECK(!a && !b && !c && h.released.size() == 2 && h.live.empty());
  give_back(FakeRelease{&h}, a, b, c);   // twice is harmless
  CHECK(h.released.size() == 2);
}

static void test_shared() {
  Shared s;
  int returned = 0;
  auto last = [&] { ++returned; };
  s.hold();
  s.hold();
  s.hold();
  s.drop(last);
  s.drop(last);
  CHECK(s.users == 1 && returned == 0);
  s.drop(last);
  CHECK(s.users == 0 && returned == 1);
  s.drop(last);   // nobody holds it: nothing
  CHECK(s.users == 0 && returned == 1);
}

int main() {
  test_commit();
  for (int k = 1; k <= 3; ++k) test_rollback(k);
  test_check_and_abandon();
  test_tables();
  test_width_retry();
  test_hooks();
  test_grow();
  test_give_back();
  test_shared();
  std::printf(g_failed ? "take_test: %d check(s) failed\n" : "take_test: ok\n", g_failed);
  return g_failed ? 1 : 0;
}
