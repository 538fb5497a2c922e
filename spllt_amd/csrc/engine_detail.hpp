// What the translation units of the Engine share (engine.cpp, engine_solve.cpp): the error-check macros of
// its member functions, the one-allocation table upload, the error code of a failed allocation, the two rules
// by which a call's vectors are cut into launch sets, RCCL.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

namespace spx {

constexpr int kErrHip = -30, kErrNotPosDef = -20;

#define HIPCHK(call, what)                                   \
  do {                                                       \
    hipError_t e__ = (call);                                 \
    if (e__ != hipSuccess) return fail(kErrHip, what, e__);  \
  } while (0)

// what a feature returns when taking its device memory failed: -1 (no memory) or -30 (the runtime)
inline int alloc_code(hipError_t e) { return e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation ? -1 : kErrHip; }

// The vectors of a call for the blocked kernels (blocks of rb = 16 or 32; cap: the widest block the feature's
// storage holds): blocks of 32 while more than 16 are left, the tail as ONE zero-padded block of 16 or 32.
// f(done, nv, rb) per block of nv <= rb vectors; the walk stops at the first non-zero return of f and returns it.
template <class F>
int for_each_block(int total, int cap, F&& f) {
  for (int done = 0; done < total;) {
    const int left = total - done;
    const int rb = (left > 16 && cap == 32) ? 32 : 16, nv = std::min(left, rb);
    if (int rc = f(done, nv, rb)) return rc;
    done += nv;
  }
  return 0;
}

// The same for the kernels that take 4, 2 or 1 vectors per sweep: f(done, cur).
template <class F>
int for_each_group4(int total, F&& f) {
  for (int done = 0; done < total;) {
    const int left = total - done;
    const int cur = left >= 4 ? 4 : (left >= 2 ? 2 : 1);
    if (int rc = f(done, cur)) return rc;
    done += cur;
  }
  return 0;
}

// The products of one block of the factor products on two workspaces, the packed vectors in w0: job 0 is L^T X into
// w1 and L of that back into w0, job 1 is L X and job 2 L^T X into w1.  product(transpose, from, to); returns the
// workspace that holds the result.
template <class P>
double* factor_mult_sequence(int job, double* w0, double* w1, P&& product) {
  if (job != 1) product(true, w0, w1);
  if (job == 0) product(false, w1, w0);
  if (job == 1) product(false, w0, w1);
  return job == 0 ? w0 : w1;
}

// Tables of an engine go to the device as ONE allocation and ONE copy: the parts are laid out in
// a host staging buffer (256-byte aligned), the typed device pointers are set after the upload.
// (Two dozen allocations, synchronous copies and frees per engine were two dozen chances per
// engine to sit in the runtime.)
struct TableStager {
  struct Slot { void** dptr; size_t off; };
  std::vector<char> host;
  std::vector<Slot> slots;
  template <class Tp>
  void add(Tp** dptr, const Tp* src, size_t count) {
    const size_t off = (host.size() + 255) / 256 * 256;
    const size_t bytes = std::max<size_t>(count * sizeof(Tp), 8);
    host.resize(off + bytes, 0);
    if (count) std::memcpy(host.data() + off, src, count * sizeof(Tp));
    slots.push_back({(void**)dptr, off});
  }
  template <class Tp>
  void add(Tp** dptr, const std::vector<Tp>& v) { add(dptr, v.data(), v.size()); }
  template <class Alloc>
  hipError_t commit(char** blob, Alloc&& alloc) {
    hipError_t e = alloc((void**)blob, std::max<size_t>(host.size(), 8));
    if (e != hipSuccess) return e;
    if (!host.empty()) e = hipMemcpy(*blob, host.data(), host.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) return e;
    for (const Slot& sl : slots) *sl.dptr = *blob + sl.off;
    return hipSuccess;
  }
};

// ---- the device memory of the optional features -------------------------------------------------------------
// Every feature takes its buffers on first use, all or nothing, through ONE allocation path (feature_alloc) and
// the three helpers below; what several features use is counted (Shared).  None of this owns memory beyond a
// call: the engine's ledger does, and a Take lives on the stack of the prepare_* / reserve_* that made it.
//
// The two debug hooks of that path (spllt_hip_debug): simulated return codes, nothing is asked of the device.
inline std::atomic<int>& fmult_alloc_fail_left() { static std::atomic<int> v{0}; return v; }   // "fmult_alloc_fail=n"
inline std::atomic<int>& alloc_fail_countdown() { static std::atomic<int> v{0}; return v; }    // "alloc_fail_at=k"

// block: an allocation the hook "fmult_alloc_fail" may refuse (the width-dependent buffers of the blocked paths,
// the buffers of the constraints); every call counts for "alloc_fail_at", which disarms itself when it fires
template <class Alloc>
hipError_t feature_alloc(Alloc& alloc, void** p, size_t bytes, bool block) {
  if (block && fmult_alloc_fail_left().load() > 0) {
    fmult_alloc_fail_left().fetch_sub(1);
    return hipErrorOutOfMemory;
  }
  if (alloc_fail_countdown().load() > 0 && alloc_fail_countdown().fetch_sub(1) == 1) return hipErrorOutOfMemory;
  return alloc(p, bytes);
}

// releases every non-null argument and nulls it, whatever its pointee type
template <class Release, class... Tp>
void give_back(Release&& release, Tp*&... p) {
  auto one = [&](auto*& q) {
    if (q) release((void*)q);
    q = nullptr;
  };
  (one(p), ...);
}

// One all-or-nothing take.  Every request after the first failure is a no-op; leaving the scope without commit()
// releases what THIS transaction took, last first, nulls the pointers it set (and no other) and clears the
// sticky HIP error.  alloc(void**, size_t) -> hipError_t, release(void*).
template <class Alloc, class Release>
class Take {
 public:
  Take(Alloc alloc, Release release) : alloc_(std::move(alloc)), release_(std::move(release)) {}
  Take(const Take&) = delete;
  Take& operator=(const Take&) = delete;
  ~Take() {
    if (committed_) return;
    for (size_t i = set_.size(); i-- > 0;) {
      if (set_[i].owns) release_(*set_[i].p);
      *set_[i].p = nullptr;
    }
    if (e_ != hipSuccess) (void)hipGetLastError();
  }
  template <class Tp> void operator()(Tp** p, size_t bytes) { take((void**)p, bytes, false); }
  template <class Tp> void block(Tp** p, size_t bytes) { take((void**)p, bytes, true); }   // through "fmult_alloc_fail"
  // the one allocation and the one copy of a TableStager; the typed pointers of its slots are rolled back too
  void tables(TableStager& tab, char** blob) {
    bytes_ += std::max<size_t>(tab.host.size(), 8);
    if (e_ != hipSuccess) return;
    e_ = tab.commit(blob, [this](void** q, size_t b) {
      const hipError_t e = feature_alloc(alloc_, q, b, false);
      if (e == hipSuccess) set_.push_back({q, true});
      return e;
    });
    if (e_ == hipSuccess)
      for (const TableStager::Slot& sl : tab.slots) set_.push_back({sl.dptr, false});
  }
  void check(hipError_t e) { if (e_ == hipSuccess) e_ = e; }   // any other step joins the same outcome
  bool ok() const { return e_ == hipSuccess; }
  hipError_t error() const { return e_; }
  size_t bytes() const { return bytes_; }   // of every request, made or skipped
  void commit() { committed_ = e_ == hipSuccess; }

 private:
  struct Entry { void** p; bool owns; };
  void take(void** p, size_t bytes, bool block) {
    bytes_ += bytes;
    if (e_ != hipSuccess) return;
    e_ = feature_alloc(alloc_, p, bytes, block);
    if (e_ == hipSuccess) set_.push_back({p, true});
  }
  Alloc alloc_;
  Release release_;
  std::vector<Entry> set_;
  hipError_t e_ = hipSuccess;
  size_t bytes_ = 0;
  bool committed_ = false;
};

// A buffer that grows with the calls: kept while it holds `need` elements, else released and taken again.  A
// failure leaves *p null and *have 0; the caller writes its own message.
template <class Alloc, class Release, class Tp>
hipError_t grow(Alloc&& alloc, Release&& release, Tp** p, size_t* have, size_t need) {
  if (*p && *have >= need) return hipSuccess;
  give_back(release, *p);
  *have = 0;
  const hipError_t e = feature_alloc(alloc, (void**)p, sizeof(Tp) * std::max<size_t>(need, 1), false);
  if (e == hipSuccess) {
    *have = need;
  } else {
    (void)hipGetLastError();
    *p = nullptr;
  }
  return e;
}

// What more than one feature uses: every user holds it once (on its own not-ready -> ready edge) and drops it
// once; the drop of the last user runs `last`, which returns the memory.
struct Shared {
  int users = 0;
  void hold() { ++users; }
  template <class F>
  void drop(F&& last) {
    if (users > 0 && --users == 0) last();
  }
};

// RCCL, resolved at run time from the librccl the process already has (engine.cpp)
typedef int (*nccl_allreduce_t)(const void*, void*, size_t, int, int, void*, hipStream_t);
typedef int (*nccl_reducescatter_t)(const void*, void*, size_t, int, int, void*, hipStream_t);
typedef int (*nccl_broadcast_t)(const void*, void*, size_t, int, int, void*, hipStream_t);
typedef int (*nccl_group_t)();
typedef int (*nccl_query_t)(void*, int*);
typedef const char* (*nccl_errstr_t)(int);
struct Rccl {
  void* handle = nullptr;
  nccl_allreduce_t all_reduce = nullptr;
  nccl_reducescatter_t reduce_scatter = nullptr;
  nccl_broadcast_t broadcast = nullptr;
  nccl_group_t group_start = nullptr, group_end = nullptr;
  nccl_query_t comm_count = nullptr, comm_user_rank = nullptr;
  nccl_errstr_t err_string = nullptr;
  bool ok() const { return all_reduce && reduce_scatter && broadcast && group_start && group_end && comm_count && comm_user_rank; }
};
constexpr int kNcclDouble = 8, kNcclSum = 0;      // ncclFloat64, ncclSum (rccl.h)
Rccl& rccl();

#define NCCLCHK(call, what)                                                                      \
  do {                                                                                           \
    int r__ = (call);                                                                            \
    if (r__ != 0) {                                                                              \
      status_ = kErrHip;                                                                         \
      err_ = std::string(what) + ": RCCL error " + std::to_string(r__) +                         \
             (rccl().err_string ? std::string(" (") + rccl().err_string(r__) + ")" : std::string()); \
      std::fprintf(stderr, "spllt-hip: %s\n", err_.c_str());                                     \
      return kErrHip;                                                                            \
    }                                                                                            \
  } while (0)

}  // namespace spx
