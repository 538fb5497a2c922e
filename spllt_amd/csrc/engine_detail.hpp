// What the translation units of the Engine share (engine.cpp, engine_solve.cpp): the error-check macros of
// its member functions, the one-allocation table upload, the error code of a failed allocation, the two rules
// by which a call's vectors are cut into launch sets, RCCL.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
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
