// Engine implementation (HIP runtime API; compiled by hipcc as host code).
#include "engine.hpp"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <mutex>
#include <thread>
#include <dlfcn.h>

#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "engine_detail.hpp"
#include "kernels.hpp"
#include "updown_stage.hpp"

namespace spx {

namespace {
double now_ms() {
  using namespace std::chrono;
  return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}
}  // namespace

int Engine::fail(int code, const char* what, hipError_t e) {
  status_ = code;
  err_ = std::string(what) + ": " + hipGetErrorString(e);
  std::fprintf(stderr, "spllt-hip: %s\n", err_.c_str());
  return code;
}

// pinned words for the "not positive definite" flag, pooled per process
static std::vector<int*> g_pinned_words;
static std::mutex g_pinned_mu;
static hipError_t borrow_pinned_word(int** p) {
  std::lock_guard<std::mutex> lk(g_pinned_mu);
  if (!g_pinned_words.empty()) {
    *p = g_pinned_words.back();
    g_pinned_words.pop_back();
    return hipSuccess;
  }
  return hipHostMalloc((void**)p, sizeof(int), hipHostMallocDefault);
}
static void return_pinned_word(int* p) {
  std::lock_guard<std::mutex> lk(g_pinned_mu);
  if (p) g_pinned_words.push_back(p);
}

// ---------------------------------------------------------------------------
// Process-wide resource pools.  An engine takes its runtime objects from here and hands them
// back; nothing is created or destroyed per engine that can be reused:
//   * streams and events (below): creating and destroying a CU-masked stream is creating and
//     destroying a hardware queue (the driver unmaps and remaps every queue of the process for
//     it) -- the one thing the engines of round 2 did per factorization that nothing else in
//     the process does, see DESIGN.md "Hangs";
//   * device buffers: hipFree synchronises the WHOLE device -- every other live engine's
//     streams, and the caller's -- so the buffers of a closed engine are kept (up to a cap) for
//     the next one;
//   * pinned staging buffers for the host-to-device copy of val.
// pools_teardown() (atexit, registered on first use, i.e. after the HIP runtime has registered
// its own handlers and therefore run BEFORE them) drains and destroys all of it, so that the
// runtime does not unload with live CU-masked queues (the exit crash of the profiled runs).
// ---------------------------------------------------------------------------
namespace {
std::mutex g_pool_mu;
struct DevBuf { void* p; size_t bytes; int device; };
std::vector<DevBuf> g_dev_cache;
size_t g_dev_cached_bytes = 0;
struct PinBuf { void* p; size_t bytes; };
std::vector<PinBuf> g_pin_cache;
bool g_teardown_registered = false;
void pools_teardown();
// Process-wide: a wait ran into its deadline or a submission never returned.  From then on the
// HIP runtime may be stuck inside a call that holds its own locks (or ours): nothing at exit may
// touch it again -- pools_teardown() returns at once, so that the process that DETECTED the hang
// can still exit (its exit code tells the caller), instead of trading "the call never returns"
// for "the process never exits".
std::atomic<bool> g_runtime_wedged{false};
void register_teardown() {
  if (!g_teardown_registered) {
    g_teardown_registered = true;
    std::atexit(pools_teardown);
  }
}
size_t dev_cache_cap() {
  static const size_t cap = [] {
    const char* e = std::getenv("SPLLT_HIP_CACHE_MB");
    return (size_t)(e && *e ? std::atoll(e) : 2048) << 20;
  }();
  return cap;
}
}  // namespace

// a device buffer of at least `bytes`: from the cache (smallest fit that wastes at most half), else
// hipMalloc; *cap receives the buffer's real capacity (what dev_release must be told, so that the
// cache's byte count -- and with it the SPLLT_HIP_CACHE_MB cap -- stays exact)
static hipError_t dev_alloc(void** p, size_t bytes, int device, size_t* cap) {
  bytes = std::max<size_t>(bytes, 256);
  *cap = bytes;
  {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    register_teardown();
    int best = -1;
    for (size_t i = 0; i < g_dev_cache.size(); ++i) {
      const DevBuf& b = g_dev_cache[i];
      if (b.device != device || b.bytes < bytes || b.bytes > 2 * bytes + (1 << 20)) continue;
      if (best < 0 || b.bytes < g_dev_cache[(size_t)best].bytes) best = (int)i;
    }
    if (best >= 0) {
      *p = g_dev_cache[(size_t)best].p;
      *cap = g_dev_cache[(size_t)best].bytes;
      g_dev_cached_bytes -= g_dev_cache[(size_t)best].bytes;
      g_dev_cache.erase(g_dev_cache.begin() + best);
      return hipSuccess;
    }
  }
  return hipMalloc(p, bytes);
}
// back into the cache (the caller has drained every stream that used it); beyond the cap, or
// when the size is not known to the cache, it is freed for real
static void dev_release(void* p, size_t bytes, int device) {
  if (!p) return;
  bytes = std::max<size_t>(bytes, 256);
  {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    if (g_dev_cached_bytes + bytes <= dev_cache_cap()) {
      g_dev_cache.push_back({p, bytes, device});
      g_dev_cached_bytes += bytes;
      return;
    }
  }
  (void)hipFree(p);
}
static hipError_t pin_alloc(void** p, size_t bytes) {
  {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    register_teardown();
    for (size_t i = 0; i < g_pin_cache.size(); ++i)
      if (g_pin_cache[i].bytes == bytes) {
        *p = g_pin_cache[i].p;
        g_pin_cache.erase(g_pin_cache.begin() + (long)i);
        return hipSuccess;
      }
  }
  return hipHostMalloc(p, bytes, hipHostMallocDefault);
}
static void pin_release(void* p, size_t bytes) {
  if (!p) return;
  std::lock_guard<std::mutex> lk(g_pool_mu);
  g_pin_cache.push_back({p, bytes});
}

double hip_deadline_s() {
  static const double limit_s = [] {
    const char* e = std::getenv("SPLLT_HIP_TIMEOUT_S");
    return (e && *e) ? std::atof(e) : 180.0;
  }();
  return limit_s;
}

// hipEventSynchronize with the deadline of sync_stream
int Engine::wait_event(hipEvent_t ev, const char* what) {
  const double limit_s = hip_deadline_s();
  if (limit_s <= 0) {
    hipError_t e = hipEventSynchronize(ev);
    return e == hipSuccess ? 0 : fail(kErrHip, what, e);
  }
  const double t0 = now_ms();
  for (;;) {
    hipError_t q = hipEventQuery(ev);
    if (q == hipSuccess) return 0;
    if (q != hipErrorNotReady) return fail(kErrHip, what, q);
    const double dt = now_ms() - t0;
    if (dt > limit_s * 1e3) break;
    if (dt > 5.0) std::this_thread::sleep_for(std::chrono::microseconds(50));
    else std::this_thread::yield();
  }
  status_ = kErrHip;
  err_ = std::string(what) + ": the copy engine did not finish within " + std::to_string((int)limit_s) + " s";
  poisoned_ = true;
  mark_runtime_wedged();
  std::fprintf(stderr, "spllt-hip: %s\n", err_.c_str());
  return kErrHip;
}

// val (pageable user memory) -> d_val_ through two pinned 16 MiB buffers: the host copies chunk
// k + 1 while the DMA of chunk k flies; every wait has the deadline.
int Engine::stage_val(const double* val_host, int64_t nnz) {
  const size_t bytes = sizeof(double) * (size_t)nnz;
  // (two sizes of staging buffers: pinning 2 x 16 MiB costs ~2 ms the first time, which a small
  // problem need not pay)
  const size_t chunk = bytes <= kH2dSmall ? kH2dSmall : kH2dChunk;
  if (h2d_chunk_ != chunk) {
    for (int i = 0; i < 2; ++i) {
      if (h2d_busy_[i]) { int rc = wait_event(h2d_ev_[i], "val H2D staging"); if (rc) return rc; h2d_busy_[i] = false; }
      if (h2d_buf_[i]) pin_release(h2d_buf_[i], h2d_chunk_);
      h2d_buf_[i] = nullptr;
    }
    h2d_chunk_ = chunk;
  }
  for (int i = 0; i < 2; ++i) {
    if (!h2d_buf_[i]) HIPCHK(pin_alloc(&h2d_buf_[i], chunk), "hipHostMalloc(staging)");
    if (!h2d_ev_[i]) HIPCHK(hipEventCreateWithFlags(&h2d_ev_[i], hipEventDisableTiming), "hipEventCreate");
  }
  const char* src = reinterpret_cast<const char*>(val_host);
  char* dst = reinterpret_cast<char*>(d_val_);
  int k = 0;
  for (size_t off = 0; off < bytes; off += chunk, ++k) {
    const int i = k & 1;
    const size_t len = std::min(chunk, bytes - off);
    if (h2d_busy_[i]) {               // the buffer's previous DMA (this call's or the last one's)
      int rc = wait_event(h2d_ev_[i], "val H2D staging");
      if (rc) return rc;
    }
    std::memcpy(h2d_buf_[i], src + off, len);
    HIPCHK(hipMemcpyAsync(dst + off, h2d_buf_[i], len, hipMemcpyHostToDevice, stream_), "val H2D");
    HIPCHK(hipEventRecord(h2d_ev_[i], stream_), "event");
    h2d_busy_[i] = true;
  }
  return 0;
}

int Engine::sync_stream(hipStream_t st, const char* what) {
  const double limit_s = hip_deadline_s();
  if (limit_s <= 0) {
    hipError_t e = hipStreamSynchronize(st);
    return e == hipSuccess ? 0 : fail(kErrHip, what, e);
  }
  const double t0 = now_ms();
  for (;;) {
    hipError_t q = hipStreamQuery(st);
    if (q == hipSuccess) return 0;
    if (q != hipErrorNotReady) return fail(kErrHip, what, q);
    const double dt = now_ms() - t0;
    if (dt > limit_s * 1e3) break;
    if (dt > 20.0) std::this_thread::sleep_for(std::chrono::microseconds(50));
    else std::this_thread::yield();
  }
  // the device does not finish: say where the program stands
  std::string rep = std::string(what) + ": the stream did not drain within " + std::to_string((int)limit_s) + " s;";
  int shown = 0;
  for (size_t i = 0; i < prog_.launches.size() && shown < 4; ++i) {
    const Launch& l = prog_.launches[i];
    if (l.record < 0 || hipEventQuery(dag_events_[(size_t)l.record]) == hipSuccess) continue;
    rep += " launch " + std::to_string(i) + " (kind " + std::to_string(l.kind) + ", level " + std::to_string(l.level) +
           ", count " + std::to_string((long long)l.count) + ", tile " + std::to_string(l.tile) + ", stream " +
           std::to_string(l.stream) + ") has not finished;";
    ++shown;
  }
  for (int i = 0; i < ST_COUNT; ++i)
    if (streams_[i]) rep += " stream " + std::to_string(i) + (hipStreamQuery(streams_[i]) == hipSuccess ? " idle;" : " busy;");
  status_ = kErrHip;
  err_ = rep;
  // The device may still be working on (or stuck in) what this engine enqueued: nothing of it is
  // touched again -- no further synchronisation (it would block for good), and its streams,
  // events, pinned words and device buffers are neither reused nor freed (see ~Engine).
  poisoned_ = true;
  mark_runtime_wedged();
  std::fprintf(stderr, "spllt-hip: %s\n", err_.c_str());
  return kErrHip;
}

hipError_t Engine::dalloc(void** p, size_t bytes) {
  size_t cap = 0;
  hipError_t e = dev_alloc(p, bytes, device_, &cap);
  if (e == hipSuccess) owned_.push_back({*p, cap});
  return e;
}

template <class Tp>
hipError_t Engine::dev_upload(Tp** dptr, const std::vector<Tp>& v) {
  size_t bytes = sizeof(Tp) * (v.empty() ? 1 : v.size());
  hipError_t e = dalloc((void**)dptr, bytes);
  if (e != hipSuccess) return e;
  if (!v.empty()) e = hipMemcpy(*dptr, v.data(), sizeof(Tp) * v.size(), hipMemcpyHostToDevice);
  return e;
}

// the "user variable -> pivot position" table of every device-side permutation: uploaded on first use, kept
// until the engine dies (n = 0: one entry)
hipError_t Engine::ensure_order() {
  if (d_order_) return hipSuccess;
  std::vector<int> order(S_->order.begin(), S_->order.end());
  if (order.empty()) order.push_back(0);
  hipError_t e = dev_upload(&d_order_, order);
  if (e != hipSuccess) give_back(d_order_);
  return e;
}

// nv vectors of len doubles (-1: n) between the caller's host array, vector q at host + q * ldx, and a packed
// device block, on stream_: one copy when ldx == len, else one per vector
int Engine::copy_vectors(bool to_device, double* dev, double* host, int64_t ldx, int64_t nv, const char* what,
                         int64_t len) {
  if (len < 0) len = S_->n;
  const hipMemcpyKind kind = to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost;
  const int64_t ncopy = ldx == len ? 1 : nv;
  const size_t bytes = sizeof(double) * (size_t)len * (size_t)(ldx == len ? nv : 1);
  for (int64_t q = 0; q < ncopy; ++q) {
    double *d = dev + q * len, *h = host + q * ldx;
    HIPCHK(hipMemcpyAsync(to_device ? d : h, to_device ? h : d, bytes, kind, stream_), what);
  }
  return 0;
}

// EngineOptions -> ScheduleOptions, in ONE place (the engine and the host-only program of
// spllt_hip_program_get / the CPU tests must build the same program); resolves the "-1 = decide by
// the problem" options of opt in place.
int resolve_graph_mode(const Symbolic& S, const EngineOptions& opt) {
  int mode = opt.graph;
  if (const char* e = std::getenv("SPLLT_HIP_GRAPH")) mode = std::atoi(e);
  if (mode < 0) {
    // by problem size (profiles/r04/graph_replay_by_size.txt): a small factorization is a few dozen
    // launches whose submission takes the host as long as the device needs for them -- the replay of
    // ONE chain of kernel nodes over the single-stream program wins 45-50 % at the small end (0.22 vs
    // 0.48 ms at the smoke size, 0.36 vs 0.69 ms on BASELINE config 1), 15 % at 19-33 GFLOP (2.80 /
    // 4.02 ms against 3.28 / 4.66 eager and 3.04 / 4.38 as the DAG replay), and is level with eager
    // launches at 313 GFLOP (hipGraphLaunch submits nothing before all nodes are enqueued)
    const double fl = (double)S.flops;
    mode = fl <= 40e9 ? 1 : 0;
  }
  if (opt.nranks > 1 || opt.poison_lds) mode = 0;      // (single-GPU programs without the debug poison only)
  return mode;
}

ScheduleOptions schedule_options(const Symbolic& S, EngineOptions& opt) {
  ScheduleOptions so;
  so.pw = opt.pw;
  so.tile = opt.tile;
  so.cb = opt.cb;
  so.lookahead = opt.lookahead;
  // a factorization that is replayed as ONE chain of kernel nodes runs in program order anyway: it gets
  // the single-stream program -- no zones, no early slices, no markers: 27 instead of 36 kernels on
  // BASELINE config 1 (profiles/r04/graph_replay_by_size.txt)
  {
    const char* e = std::getenv("SPLLT_CHAIN_GRAPH_SERIAL");      // (0: the multi-stream program, replayed in program order)
    if (!(e && std::atoi(e) == 0) && resolve_graph_mode(S, opt) == 1) so.lookahead = false;
  }
  so.slice_between = opt.slice_between;
  so.deterministic = opt.deterministic;
  so.fused_panel = opt.fused_panel;
  if (opt.subtrees >= 0) so.subtrees = opt.subtrees != 0;
  const bool lb = latency_bound(S, std::min(opt.pw, kPanelMax));
  // CU reservation (bulk / far streams masked off the last CUs): OFF by default since round 4.  It
  // bought 24.9 -> 24.4 ms in round 2 and buys 23.35 -> 23.2 ms now (0.6 %, profiles/r04/ab_cu_reserve.txt),
  // and CU-masked streams are the one object of this library whose destruction can hang
  // (profiles/r03/hang_evidence.txt) and whose survival makes rocprofv3 crash at exit.  Opt in
  // with SPLLT_HIP_RESERVE_CUS=32.
  if (opt.reserve_cus < 0) opt.reserve_cus = 0;
  if (opt.zones < 0) opt.zones = lb ? 1 : 0;
  so.zones = opt.zones != 0;
  // throughput-bound problems use the (LDS-DMA) 128-tile from 1024 tiles on: +0.3-0.9 % on the
  // large configurations; the latency-bound bench workload prefers 4096 (24.5 vs 25.0 ms)
  so.tile128_min = lb ? 4096 : 1024;
  return so;
}

void partition_options(const Symbolic& S, const EngineOptions& opt, std::vector<int>& owner,
                       std::vector<int>& top_owner, ScheduleOptions& so) {
  owner.clear();
  top_owner.clear();
  if (opt.nranks <= 1) return;
  assign_owners(S, opt.nranks, owner);
  so.node_owner = owner.data();
  so.rank = opt.rank;
  so.nranks = opt.nranks;
  int dist = opt.dist_top;
  if (const char* e = std::getenv("SPLLT_DIST_TOP"))
    if (*e) dist = std::atoi(e);
  if (dist < 0) dist = distribute_top_tree(S, owner, opt.nranks) ? 1 : 0;
  if (dist) {
    assign_top_owners(S, owner, opt.nranks, top_owner);
    so.top_owner = top_owner.data();
  }
}

Engine::Engine(std::shared_ptr<const Symbolic> S, const EngineOptions& opt)
    : S_(std::move(S)), opt_(opt) {
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev == 0) {
    // The product has no CPU path: fail loudly.
    status_ = kErrHip;
    err_ = "no HIP device available (the factorize path runs only on gfx950)";
    std::fprintf(stderr, "spllt-hip: %s\n", err_.c_str());
    return;
  }
  hipGetDevice(&device_);
  ScheduleOptions so = schedule_options(*S_, opt_);
  if (opt_.nranks > 1) {
    partition_options(*S_, opt_, owner_, top_owner_, so);
    for (int b = 0; b < S_->nbcol(); ++b)
      if (owner_[S_->bcols[b].node] < 0) top_bcols_.push_back(b);
    // only the block columns this rank touches (its own branches + the top tree) are cleared
    // per factorization: the others are never read or written here
    for (int b = 0; b < S_->nbcol(); ++b) {
      const int own = owner_[S_->bcols[b].node];
      if (own != opt_.rank && own >= 0) continue;
      const int64_t off = S_->bcols[b].off, cnt = (int64_t)S_->bcols[b].nrow * S_->bcols[b].width;
      if (!zero_ranges_.empty() && zero_ranges_.back().first + zero_ranges_.back().second == off)
        zero_ranges_.back().second += cnt;
      else
        zero_ranges_.push_back({off, cnt});
    }
  }
  build_program(*S_, so, prog_);
  arena_elems_ = S_->arena;
  if (opt_.nranks > 1) localize_program();
  if (status_ == 0) upload();
}

// Breadcrumbs (SPLLT_HIP_CRUMBS=<file>): the last step the library reached, rewritten at every
// step.  After a call that never returned (a wedged runtime call cannot be interrupted or traced
// from the caller) the file names the step.
static std::atomic<const char*> g_last_crumb{"(nothing yet)"};
const char* last_crumb() { return g_last_crumb.load(); }
static void crumb(const char* what) {
  g_last_crumb.store(what);
  static const char* path = std::getenv("SPLLT_HIP_CRUMBS");
  if (!path || !*path) return;
  if (FILE* f = std::fopen(path, "w")) {
    std::fprintf(f, "%s\n", what);
    std::fclose(f);
  }
}

// The HIP streams of the engines are pooled per process: an engine borrows a set (chain, bulk,
// far) and hands it back drained; streams are created once per (device, CU reservation) and set
// in use at the same time, never destroyed.  Hundreds of engines per process (the test suite, a
// solver that re-analyses) then do not create and destroy hundreds of priority / CU-masked
// streams -- the rare hangs seen on the GPU box sat in runtime calls, not in kernels.
namespace {
struct StreamSet {
  int device, reserve, far_on_bulk;
  hipStream_t chain, bulk, far;
  bool in_use;
  hipStream_t side = nullptr;     // the chain's companion (same priority, no mask): ScheduleOptions::split_next
};
std::mutex g_stream_mu;
std::vector<StreamSet> g_stream_pool;
}  // namespace

static hipError_t borrow_streams(int device, int reserve, int ncu, bool far_on_bulk, hipStream_t* chain,
                                 hipStream_t* bulk, hipStream_t* far, hipStream_t* side) {
  std::lock_guard<std::mutex> lk(g_stream_mu);
  for (StreamSet& ss : g_stream_pool)
    if (!ss.in_use && ss.device == device && ss.reserve == reserve && ss.far_on_bulk == (int)far_on_bulk) {
      ss.in_use = true;
      *chain = ss.chain; *bulk = ss.bulk; *far = ss.far; *side = ss.side;
      return hipSuccess;
    }
  int prio_lo = 0, prio_hi = 0;
  hipError_t e = hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
  if (e != hipSuccess) return e;
  auto masked_stream = [&](hipStream_t* st) -> hipError_t {
    if (reserve <= 0) return hipStreamCreateWithPriority(st, hipStreamNonBlocking, prio_lo);
    std::vector<uint32_t> mask((ncu + 31) / 32, 0u);
    for (int cu = 0; cu < ncu - reserve; ++cu) mask[cu / 32] |= 1u << (cu % 32);
    return hipExtStreamCreateWithCUMask(st, (uint32_t)mask.size(), mask.data());
  };
  StreamSet ss{device, reserve, (int)far_on_bulk, nullptr, nullptr, nullptr, true};
  // (the chain stream confined to the reserved CUs -- the mirror image of the bulk mask -- was
  // measured: 32.7 ms with 32 CUs, 26.6 with 64, 28.1 with 96 against 23.7: its launches at the
  // lower levels have thousands of workgroups)
  if ((e = hipStreamCreateWithPriority(&ss.chain, hipStreamNonBlocking, prio_hi)) != hipSuccess) return e;
  if ((e = masked_stream(&ss.bulk)) != hipSuccess) return e;
  if (far_on_bulk) ss.far = ss.bulk;
  else if ((e = masked_stream(&ss.far)) != hipSuccess) return e;
  if ((e = hipStreamCreateWithPriority(&ss.side, hipStreamNonBlocking, prio_hi)) != hipSuccess) return e;
  g_stream_pool.push_back(ss);
  *chain = ss.chain; *bulk = ss.bulk; *far = ss.far; *side = ss.side;
  return hipSuccess;
}

// ... and so are the dependency events of the programs (a few hundred per engine, no timing).
// An event taken from the pool may carry the record of an earlier engine: waiting for it is a
// no-op, exactly like waiting for an event that was never recorded.
static std::vector<std::vector<hipEvent_t>> g_event_pool;   // per device

static hipError_t borrow_events(std::vector<hipEvent_t>& out, size_t n, int device) {
  std::lock_guard<std::mutex> lk(g_stream_mu);
  if ((int)g_event_pool.size() <= device) g_event_pool.resize((size_t)device + 1);
  std::vector<hipEvent_t>& pool = g_event_pool[(size_t)device];
  out.assign(n, nullptr);
  for (size_t i = 0; i < n; ++i) {
    if (!pool.empty()) {
      out[i] = pool.back();
      pool.pop_back();
    } else {
      hipError_t e = hipEventCreateWithFlags(&out[i], hipEventDisableTiming);
      if (e != hipSuccess) return e;
    }
  }
  return hipSuccess;
}

static void return_events(std::vector<hipEvent_t>& ev, int device) {
  std::lock_guard<std::mutex> lk(g_stream_mu);
  if ((int)g_event_pool.size() <= device) g_event_pool.resize((size_t)device + 1);
  for (hipEvent_t e : ev)
    if (e) g_event_pool[(size_t)device].push_back(e);
  ev.clear();
}

static void return_streams(hipStream_t chain) {
  std::lock_guard<std::mutex> lk(g_stream_mu);
  for (StreamSet& ss : g_stream_pool)
    if (ss.chain == chain) ss.in_use = false;
}

namespace {
// atexit: the pools go before the HIP runtime does (see the comment at the pools).  Streams that
// are still in use (a leaked, poisoned engine) or not idle are left alone.
void pools_teardown() {
  // SPLLT_TEARDOWN: 0 nothing, 1 (default) everything but the streams, 2 the streams too.
  // hipStreamDestroy of a CU-masked stream is the one call of this library that has been caught
  // not returning (profiles/r03/hang_evidence.txt): it is not made unless asked for -- the
  // profiling scripts ask, because rocprofv3's own teardown crashes on live CU-masked queues,
  // and they run under a timeout.
  static const int mode = [] { const char* e = std::getenv("SPLLT_TEARDOWN"); return e ? std::atoi(e) : 1; }();
  if (mode == 0) return;
  if (g_runtime_wedged.load()) {
    crumb("teardown: skipped, the runtime is wedged");
    return;
  }
  crumb("teardown: streams (lock)");
  // (a helper thread stuck inside borrow_streams / hipExtStreamCreateWithCUMask holds this mutex for good)
  std::unique_lock<std::mutex> lk(g_stream_mu, std::try_to_lock);
  if (!lk.owns_lock()) {
    crumb("teardown: skipped, the stream pool is locked");
    return;
  }
  for (StreamSet& ss : g_stream_pool) {
    if (mode < 2) break;
    if (ss.in_use) continue;
    crumb("teardown: streams (query)");
    if (hipStreamQuery(ss.chain) != hipSuccess || hipStreamQuery(ss.bulk) != hipSuccess ||
        hipStreamQuery(ss.far) != hipSuccess || (ss.side && hipStreamQuery(ss.side) != hipSuccess)) continue;
    crumb("teardown: streams (destroy chain)");
    (void)hipStreamDestroy(ss.chain);
    crumb("teardown: streams (destroy bulk)");
    (void)hipStreamDestroy(ss.bulk);
    crumb("teardown: streams (destroy far)");
    if (ss.far != ss.bulk) (void)hipStreamDestroy(ss.far);
    if (ss.side) (void)hipStreamDestroy(ss.side);      // (plain priority stream: no CU mask)
    ss.chain = ss.bulk = ss.far = ss.side = nullptr;
    ss.in_use = true;        // (never handed out again)
  }
  crumb("teardown: events");
  for (auto& pool : g_event_pool) {
    for (hipEvent_t e : pool) (void)hipEventDestroy(e);
    pool.clear();
  }
  crumb("teardown: pinned memory");
  {
    std::lock_guard<std::mutex> lk2(g_pinned_mu);
    for (int* q : g_pinned_words) (void)hipHostFree(q);
    g_pinned_words.clear();
  }
  std::lock_guard<std::mutex> lk3(g_pool_mu);
  for (const PinBuf& b : g_pin_cache) (void)hipHostFree(b.p);
  g_pin_cache.clear();
  crumb("teardown: device buffers");
  for (const DevBuf& b : g_dev_cache) (void)hipFree(b.p);
  g_dev_cache.clear();
  g_dev_cached_bytes = 0;
  crumb("teardown: done");
}
}  // namespace

// the val -> L map bucketed by chunks of kInitChunk doubles of the arena (k_init_arena, k_batch_init): a
// counting sort, two passes over the map; at least one chunk
static void bucket_value_map(const Symbolic& S, std::vector<int64_t>& cptr, std::vector<unsigned short>& loc,
                             std::vector<int>& src) {
  const int64_t nch = std::max<int64_t>(1, (S.arena + kInitChunk - 1) / kInitChunk);
  cptr.assign((size_t)nch + 1, 0);
  for (int64_t d : S.map_dst) cptr[(size_t)(d / kInitChunk) + 1]++;
  for (int64_t c = 0; c < nch; ++c) cptr[(size_t)c + 1] += cptr[(size_t)c];
  std::vector<int64_t> fill(cptr.begin(), cptr.end() - 1);
  loc.resize(S.map_dst.size());
  src.resize(S.map_dst.size());
  for (size_t i = 0; i < S.map_dst.size(); ++i) {
    const int64_t d = S.map_dst[i];
    const int64_t at = fill[(size_t)(d / kInitChunk)]++;
    loc[(size_t)at] = (unsigned short)(d % kInitChunk);
    src[(size_t)at] = (int)S.map_src[i];
  }
}

int Engine::upload() {
  const Symbolic& S = *S_;
  crumb("engine: upload begins");
  // The chain and side streams carry the latency-critical kernels: highest priority, all
  // CUs.  The bulk and far streams carry the updates that run BESIDE a chain: lowest
  // priority and masked off the last `reserve_cus` CUs, so that a chain kernel (one
  // workgroup, up to 145 KB of LDS) and the side launches always find a free CU instead of
  // waiting for a bulk workgroup to retire (measured, scripts/cumask_probe.hip: 14 us
  // launch-to-completion beside a masked bulk kernel, 30 us beside an unmasked one; masking
  // the FIRST bits instead gives erratic 13-450 us).  The wide stream (launches that have
  // the chip to themselves) is not masked.
  graph_mode_ = resolve_graph_mode(S, opt_);
  if (const char* e = std::getenv("SPLLT_CHAIN_PRIO")) chain_prio_ = std::atoi(e);
  if (const char* e = std::getenv("SPLLT_BULK_PAD128")) bulk_pad128_ = std::atoi(e);
  if (const char* e = std::getenv("SPLLT_BULK_PAD64")) bulk_pad64_ = std::atoi(e);
  int reserve = opt_.reserve_cus;
  if (const char* e = std::getenv("SPLLT_HIP_RESERVE_CUS")) reserve = std::atoi(e);
  // a factorization that is replayed as a graph has no streams of its own to mask (the kernel nodes
  // of a graph go where the runtime puts them): the small, latency-bound problems -- the ones that
  // used to get CU-masked streams -- no longer create any
  if (graph_mode_ > 0 && opt_.nranks <= 1 && !opt_.poison_lds && !std::getenv("SPLLT_HIP_RESERVE_CUS")) reserve = 0;
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device_), "device props");
  const int ncu = prop.multiProcessorCount;
  if (reserve < 0 || reserve * 2 > ncu || !opt_.lookahead) reserve = 0;
  // At most four hardware queues carry the five streams of the program: the runtime
  // multiplexes streams onto a handful of hardware queues, and streams that share one
  // serialise (five queues of our own: no overlap at all, 33.0 ms = the serialized 33.2 ms).
  // The wide stream only runs when the chains of a level are done -> chain queue.
  crumb("engine: borrowing streams");
  HIPCHK(borrow_streams(device_, reserve, ncu, std::getenv("SPLLT_FAR_ON_BULK") != nullptr, &streams_[ST_CHAIN],
                        &streams_[ST_BULK], &streams_[ST_FAR], &streams_[ST_SIDE]), "stream creation");
  streams_[ST_WIDE] = streams_[ST_CHAIN];
  if (!streams_[ST_SIDE]) streams_[ST_SIDE] = streams_[ST_CHAIN];
  stream_ = streams_[ST_CHAIN];
  crumb("engine: creating events");
  HIPCHK(borrow_events(dag_events_, (size_t)prog_.nevents, device_), "hipEventCreate");
  crumb("engine: allocating and uploading");
  HIPCHK(hipEventCreate(&ev0_), "hipEventCreate");
  HIPCHK(hipEventCreate(&ev1_), "hipEventCreate");
  HIPCHK(hipEventCreate(&ev_h2d_), "hipEventCreate");
  HIPCHK(hipEventCreateWithFlags(&ev_init_, hipEventDisableTiming), "hipEventCreate");
  // (+ 32 doubles: the update kernel loads whole 16-column chunks, the last one of a ragged K
  // window reaches past the block column's end)
  HIPCHK(dalloc((void**)&d_L_, sizeof(double) * (size_t)(std::max<int64_t>(1, arena_elems_) + 32)), "hipMalloc(L arena)");
  HIPCHK(dalloc((void**)&d_val_, sizeof(double) * (size_t)std::max<int64_t>(1, S.nnzA)), "hipMalloc(val)");
  HIPCHK(dalloc((void**)&d_dinv_, sizeof(double) * (size_t)(std::max<int64_t>(1, prog_.dinv_size) + 32)), "hipMalloc(dinv)");
  // the POTRF kernels store the lower triangle of an inverted panel only; what lies above the
  // diagonal of a slot is zero from here on (nothing else writes there)
  HIPCHK(hipMemset(d_dinv_, 0, sizeof(double) * (size_t)(std::max<int64_t>(1, prog_.dinv_size) + 32)), "hipMemset(dinv)");
  if (prog_.gen_size > 0) {
    // the generated elements of the subtree tasks: zero here, and zero again after every factorization
    // (the root of a subtree clears what it adds to its ancestors)
    HIPCHK(dalloc((void**)&d_gen_, sizeof(double) * (size_t)prog_.gen_size), "hipMalloc(generated elements)");
    HIPCHK(hipMemset(d_gen_, 0, sizeof(double) * (size_t)prog_.gen_size), "hipMemset(generated elements)");
  }
  if (opt_.nranks > 1) {
    // this rank scatters A only into its own subtrees; the top tree's values
    // are contributed by rank 0 alone so that the cross-rank sum holds them once
    std::vector<int64_t> md, ms;
    map_keep_.assign(S.map_dst.size(), 0);
    for (int b = 0; b < S.nbcol(); ++b) {
      const int own = owner_[S.bcols[b].node];
      const bool keep = (own == opt_.rank) || (own < 0 && opt_.rank == 0);
      if (!keep) continue;
      const int64_t delta = loc_off_[(size_t)b] - S.bcols[b].off;   // (kept block columns are held here)
      for (int64_t i = S.lmap_ptr[b]; i < S.lmap_ptr[b + 1]; ++i) {
        map_keep_[i] = 1;
        md.push_back(S.map_dst[i] + delta);
        ms.push_back(S.map_src[i]);
      }
    }
    nmap_ = (int64_t)md.size();
    HIPCHK(dev_upload(&d_map_dst_, md), "upload map_dst");
    HIPCHK(dev_upload(&d_map_src_, ms), "upload map_src");
  } else {
    nmap_ = S.nnzA;
    HIPCHK(dev_upload(&d_map_dst_, S.map_dst), "upload map_dst");
    HIPCHK(dev_upload(&d_map_src_, S.map_src), "upload map_src");
    // the same map bucketed by 32 KB chunks of the arena, for the one-pass initialisation
    // (k_init_arena): a counting sort, two passes over the map
    static const bool one_pass = [] { const char* e = std::getenv("SPLLT_INIT_ONE_PASS"); return !(e && std::atoi(e) == 0); }();
    if (one_pass && S.arena > 0 && S.nnzA <= INT_MAX) {
      std::vector<int64_t> cptr;
      std::vector<unsigned short> loc;
      std::vector<int> src;
      bucket_value_map(S, cptr, loc, src);
      HIPCHK(dev_upload(&d_init_cptr_, cptr), "upload init map");
      HIPCHK(dev_upload(&d_init_loc_, loc), "upload init map");
      HIPCHK(dev_upload(&d_init_src_, src), "upload init map");
    }
  }
  std::vector<int64_t> off(S.nbcol());
  std::vector<int> w(S.nbcol());
  for (int b = 0; b < S.nbcol(); ++b) {
    off[b] = loc_off_.empty() ? S.bcols[b].off : loc_off_[(size_t)b];   // (-1: never dereferenced here)
    w[b] = S.bcols[b].width;
  }
  TableStager tab;
  tab.add(&d_bc_off_, off);
  tab.add(&d_bc_w_, w);
  std::vector<UpdUnit> units;    // (outlives the staging copy below)
  if (prog_.scratch_size > 0) {
    HIPCHK(dalloc((void**)&d_scratch_, sizeof(double) * (size_t)prog_.scratch_size), "hipMalloc(scratch)");
    // MODE_BUFFER units address the scratch relative to the arena pointer like every other unit
    units = prog_.units;
    const int64_t shift = d_scratch_ - d_L_;
    for (UpdUnit& u : units)
      if (u.mode == MODE_BUFFER) u.d_off += shift;
    tab.add(&d_units_, units);
  } else {
    tab.add(&d_units_, prog_.units);
  }
  tab.add(&d_gtiles_, prog_.gather_tiles);
  tab.add(&d_gitems_, prog_.gather_items);
  tab.add(&d_tiles_, prog_.tiles);
  tab.add(&d_chain_, prog_.chain_units);
  tab.add(&d_panel_, prog_.panel_units);
  tab.add(&d_sub_tasks_, prog_.sub_tasks);
  tab.add(&d_sub_nodes_, prog_.sub_nodes);
  const std::vector<int> zeros(2 * std::max<size_t>(1, prog_.panel_units.size()), 0);
  tab.add(&d_panel_cnt_, zeros);
  tab.add(&d_relpos_, prog_.relpos);
  tab.add(&d_rlist_, S.rlist);
  const int big_flag = INT_MAX;
  tab.add(&d_flag_, &big_flag, 1);
  HIPCHK(tab.commit(&d_tables_, [this](void** q, size_t b) { return dalloc(q, b); }), "upload tables");
  HIPCHK(borrow_pinned_word(&h_flag_), "hipHostMalloc(flag)");
  crumb("engine: ready");
  return 0;
}

// Arena offset of the global layout -> this rank's packed arena.  Offsets in the tables are
// always the base of a block column.
int64_t Engine::to_local(int64_t g) const {
  const auto& bc = S_->bcols;
  size_t lo = 0, hi = bc.size();
  while (hi - lo > 1) {
    const size_t mid = (lo + hi) / 2;
    if (bc[mid].off <= g) lo = mid; else hi = mid;
  }
  if (bc[lo].off != g || loc_off_[lo] < 0) {
    // (const: called from a const context too; the flag is picked up by localize_program)
    std::fprintf(stderr, "spllt-hip: internal error: arena offset %lld is not a block column held by rank %d\n",
                 (long long)g, opt_.rank);
    localize_failed_ = true;
    return 0;
  }
  return loc_off_[lo];
}

void Engine::localize_program() {
  const Symbolic& S = *S_;
  loc_off_.assign((size_t)S.nbcol(), -1);
  int64_t o = 0;
  for (int b = 0; b < S.nbcol(); ++b) {
    const int own = owner_[S.bcols[b].node];
    if (own != opt_.rank && own >= 0) continue;
    loc_off_[(size_t)b] = o;
    o += (int64_t)S.bcols[b].nrow * S.bcols[b].width;
  }
  arena_elems_ = o;
  zero_ranges_.assign(1, {0, o});      // everything held here is cleared per factorization
  for (UpdUnit& u : prog_.units) {
    u.a_off = to_local(u.a_off);
    if (u.mode != MODE_BUFFER) u.d_off = to_local(u.d_off);   // (BUFFER: an offset into the scratch)
  }
  for (ChainUnit& u : prog_.chain_units) u.off = to_local(u.off);
  for (PanelUnit& u : prog_.panel_units) u.off = to_local(u.off);
  for (GatherTile& t : prog_.gather_tiles) t.d_off = to_local(t.d_off);
  for (ExchangeItem& it : prog_.xitems)
    if (it.space == 0) it.off = to_local(it.off);
  if (localize_failed_) {
    // a table entry points at a block column this rank does not hold: running the program would
    // silently read and write this rank's first block column instead
    status_ = -30;
    err_ = "internal error: the rank's program refers to a block column it does not hold";
  }
}

Engine::~Engine() {
  if (graph_exec_ && !poisoned_) hipGraphExecDestroy(graph_exec_);
  if (graph_ && !poisoned_) hipGraphDestroy(graph_);
  if (poisoned_) {
    // A wait of this engine ran into its deadline (or its submission never returned): the device
    // may still execute, or be stuck in, what it enqueued.  Nothing is synchronised (that would
    // block for good), nothing goes back into the pools (the next engine would run behind, or
    // beside, the stale program), nothing the queued work may touch is freed: it is leaked.
    crumb("engine: poisoned, resources leaked");
    return;
  }
  crumb("engine: destructor, draining streams");
  for (hipStream_t st : streams_)
    if (st && sync_stream(st, "engine teardown") != 0) {
      crumb("engine: teardown ran into the deadline, resources leaked");
      return;                               // (poisoned by sync_stream)
    }
  crumb("engine: destructor, releasing");
  return_events(dag_events_, device_);       // (the streams are drained: nothing refers to them any more)
  for (const auto& b : owned_) dev_release(b.first, b.second, device_);   // kept for the next engine, not hipFree'd:
  owned_.clear();                                                          // hipFree synchronises the whole device
  if (h2d_buf_[0]) pin_release(h2d_buf_[0], h2d_chunk_);
  if (h2d_buf_[1]) pin_release(h2d_buf_[1], h2d_chunk_);
  for (hipEvent_t e : h2d_ev_)
    if (e) hipEventDestroy(e);
  return_pinned_word(h_flag_);
  if (ev0_) hipEventDestroy(ev0_);
  if (ev1_) hipEventDestroy(ev1_);
  if (ev_h2d_) hipEventDestroy(ev_h2d_);
  if (ev_init_) hipEventDestroy(ev_init_);
  if (streams_[ST_CHAIN]) return_streams(streams_[ST_CHAIN]);   // drained above; back into the pool
  crumb("engine: destroyed");
}

// the kernel of one launch of the program, onto a stream or into a graph (LaunchSink)
void Engine::emit_kernel(const Launch& l, const LaunchSink& sink, bool multi) {
  if (l.kind == L_CHAIN) {
    launch_chain_panel(sink, d_chain_ + l.first, l.count, d_L_, d_dinv_, d_flag_, prog_.chain_units[(size_t)l.first]);
  } else if (l.kind == L_CHAIN4) {
    launch_chain_block(sink, d_chain_ + l.first, l.count, d_L_, d_dinv_, d_flag_, prog_.pw,
                       prog_.chain_units[(size_t)l.first]);
  } else if (l.kind == L_TRSM4) {
    launch_trsm_rows(sink, d_tiles_ + l.first, l.count, d_units_, d_L_, d_dinv_, prog_.pw,
                     (multi && l.stream == ST_CHAIN) ? chain_prio_ : 0);
  } else if (l.kind == L_SUBTREE) {
    launch_subtree(sink, d_sub_tasks_ + l.first, l.count, d_sub_nodes_, d_units_, d_relpos_, d_rlist_, d_L_, d_dinv_,
                   d_gen_, d_flag_);
  } else if (l.kind == L_PANEL) {
    launch_panel(sink, d_tiles_ + l.first, l.count, d_panel_, d_L_, d_dinv_, d_panel_cnt_, d_flag_);
  } else if (l.kind == L_GATHER) {
    launch_gather(sink, d_gtiles_ + l.first, l.count, d_gitems_, d_L_, d_scratch_, d_relpos_, d_rlist_);
  } else {
    // multi-stream program: chain / side launches run at raised wave priority
    const int prio = (multi && (l.stream == ST_CHAIN || l.stream == ST_SIDE)) ? chain_prio_ : 0;
    int pad = 0;
    if (multi && l.overlap) pad = l.tile == 128 ? bulk_pad128_ : bulk_pad64_;
    launch_update(sink, l.tile, d_tiles_ + l.first, l.count, d_units_, d_bc_off_, d_bc_w_, d_L_,
                  d_relpos_, d_rlist_, d_dinv_, prio, pad, true, l.lat != 0);
  }
}

int Engine::enqueue_launch(const Launch& l, bool serial) {
  hipStream_t st = serial ? stream_ : streams_[l.stream];
  if (!serial)
    for (int w : l.wait)
      if (w >= 0) HIPCHK(hipStreamWaitEvent(st, dag_events_[w], 0), "stream wait");
  if (l.count > 0 && l.kind != L_EXCHANGE) {
    if (opt_.poison_lds) launch_poison_lds(st);
    emit_kernel(l, LaunchSink(st), !serial && opt_.lookahead);
  }
  if (!serial && l.record >= 0) HIPCHK(hipEventRecord(dag_events_[l.record], st), "event record");
  return 0;
}

// The whole factorization of one pattern as ONE HIP graph (analyse once,
// factorize many -- reference spllt_kernels_mod.F90:2301-2364 re-initialises the same structure
// for new values).  Built explicitly from the program (no stream capture: capturing the
// multi-stream program crashed inside the runtime on ROCm 7.2): clear the arena, the "last
// reader" counters and the flag, scatter the values, then one kernel node per launch, the flag's
// way back to the host last.  Every address is fixed for the life of the engine; only the
// content of d_val_ changes between replays.
//   mode 1: a chain in program order (= the single-stream program: every node behind the one in
//           front; 1.5 us per boundary instead of the eager path's 2.7 us, or 6.4 us where an
//           event record sits between two launches -- scripts/gap_probe.hip)
//   mode 2: the DAG of the multi-stream program: a node follows its predecessor on the same
//           program stream and the launches that record the events it waits for
int Engine::build_graph(int mode) {
  if (graph_exec_) return 0;
  if (!prog_.exchanges.empty() || opt_.poison_lds) return -98;   // single-GPU programs only
  const Symbolic& S = *S_;
  HIPCHK(hipGraphCreate(&graph_, 0), "hipGraphCreate");
  std::vector<hipGraphNode_t> head;      // the prefix every launch follows
  auto memset_node = [&](void* dst, int value, size_t words, const std::vector<hipGraphNode_t>& deps,
                         hipGraphNode_t* out) -> hipError_t {
    hipMemsetParams mp{};
    mp.dst = dst;
    mp.elementSize = 4;
    mp.value = (unsigned)value;
    mp.width = words;
    mp.height = 1;
    mp.pitch = words * 4;
    return hipGraphAddMemsetNode(out, graph_, deps.data(), deps.size(), &mp);
  };
  hipGraphNode_t n_cnt = nullptr, n_flag = nullptr;
  std::vector<hipGraphNode_t> pre;
  const bool one_pass_init = d_init_cptr_ != nullptr;     // k_init_arena clears as it copies
  if (!one_pass_init) {
    // (in pieces of 4 GiB: 32-bit element counts somewhere below would not be a surprise)
    const size_t words = (size_t)S.arena * 2, piece = (size_t)1 << 30;
    for (size_t o = 0; o < words; o += piece) {
      hipGraphNode_t n = nullptr;
      HIPCHK(memset_node((int*)d_L_ + o, 0, std::min(piece, words - o), {}, &n), "graph memset arena");
      pre.push_back(n);
    }
  }
  if (!prog_.panel_units.empty()) {
    HIPCHK(memset_node(d_panel_cnt_, 0, 2 * prog_.panel_units.size(), {}, &n_cnt), "graph memset counters");
    pre.push_back(n_cnt);
  }
  HIPCHK(memset_node(d_flag_, INT_MAX, 1, {}, &n_flag), "graph memset flag");
  pre.push_back(n_flag);
  hipGraphNode_t n_scatter = nullptr;
  {
    LaunchSink sink;
    sink.graph = graph_;
    sink.deps = pre.data();
    sink.ndeps = pre.size();
    if (one_pass_init)
      launch_init_arena(sink, d_L_, S.arena, d_val_, d_init_cptr_, d_init_loc_, d_init_src_);
    else
      launch_scatter_val(sink, d_L_, d_val_, d_map_dst_, d_map_src_, nmap_);
    HIPCHK(sink.err, "graph scatter node");
    n_scatter = sink.node;
    if (!n_scatter) {     // (no entries: an empty node keeps the prefix in one piece)
      HIPCHK(hipGraphAddEmptyNode(&n_scatter, graph_, pre.data(), pre.size()), "graph empty node");
    }
  }
  const size_t nl = prog_.launches.size();
  std::vector<hipGraphNode_t> recorder((size_t)std::max(1, prog_.nevents), nullptr);   // event id -> node
  hipGraphNode_t last_on[ST_COUNT] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  hipGraphNode_t last = n_scatter;
  for (size_t i = 0; i < nl; ++i) {
    const Launch& l = prog_.launches[i];
    std::vector<hipGraphNode_t> deps;
    auto add_dep = [&](hipGraphNode_t n) {
      if (!n) return;
      for (hipGraphNode_t d : deps)
        if (d == n) return;
      deps.push_back(n);
    };
    if (mode == 1) {
      add_dep(last);
    } else {
      // (the wide and side streams are the chain stream, as in the eager engine)
      const int sid = (l.stream == ST_WIDE || l.stream == ST_SIDE) ? ST_CHAIN : l.stream;
      add_dep(last_on[sid] ? last_on[sid] : n_scatter);
      for (int w : l.wait)
        if (w >= 0) add_dep(recorder[(size_t)w]);
    }
    hipGraphNode_t node = nullptr;
    if (l.count > 0) {
      LaunchSink sink;
      sink.graph = graph_;
      sink.deps = deps.data();
      sink.ndeps = deps.size();
      emit_kernel(l, sink, mode == 2 && opt_.lookahead);
      HIPCHK(sink.err, "graph kernel node");
      node = sink.node;
    } else {
      HIPCHK(hipGraphAddEmptyNode(&node, graph_, deps.data(), deps.size()), "graph marker node");
    }
    last = node;
    const int sid = (l.stream == ST_WIDE || l.stream == ST_SIDE) ? ST_CHAIN : l.stream;
    last_on[sid] = node;
    if (l.record >= 0) recorder[(size_t)l.record] = node;
  }
  {
    std::vector<hipGraphNode_t> deps;
    if (mode == 1) {
      deps.push_back(last);
    } else {
      auto add = [&](hipGraphNode_t n) {
        if (n && std::find(deps.begin(), deps.end(), n) == deps.end()) deps.push_back(n);
      };
      for (hipGraphNode_t n : last_on) add(n);
      if (prog_.final_event >= 0) add(recorder[(size_t)prog_.final_event]);
      if (deps.empty()) deps.push_back(n_scatter);
    }
    hipGraphNode_t n_out = nullptr;
    HIPCHK(hipGraphAddMemcpyNode1D(&n_out, graph_, deps.data(), deps.size(), h_flag_, d_flag_, sizeof(int),
                                   hipMemcpyDeviceToHost), "graph flag read");
  }
  HIPCHK(hipGraphInstantiate(&graph_exec_, graph_, nullptr, nullptr, 0), "hipGraphInstantiate");
  return 0;
}

int Engine::enqueue_range(size_t first, size_t last) {
  for (size_t i = first; i < last; ++i) {
    int rc = enqueue_launch(prog_.launches[i], false);
    if (rc) return rc;
  }
  return 0;
}

int Engine::finish_enqueue() {
  if (prog_.final_event >= 0)
    HIPCHK(hipStreamWaitEvent(stream_, dag_events_[prog_.final_event], 0), "final wait");
  HIPCHK(hipGetLastError(), "kernel launch");
  HIPCHK(hipMemcpyAsync(h_flag_, d_flag_, sizeof(int), hipMemcpyDeviceToHost, stream_), "flag read");
  return 0;
}

int Engine::enqueue_program() {
  const Symbolic& S = *S_;
  if (replays_graph()) {
    int rc = build_graph(graph_mode_);
    if (rc) return rc;
    stats_.launches = (int)prog_.launches.size() + 1;
    HIPCHK(hipGraphLaunch(graph_exec_, stream_), "hipGraphLaunch");
    awaiting_exchange_ = false;
    return 0;
  }
  const bool one_pass_init = opt_.nranks <= 1 && d_init_cptr_ != nullptr;
  if (opt_.nranks > 1) {
    for (const auto& r : zero_ranges_)
      HIPCHK(hipMemsetAsync(d_L_ + r.first, 0, sizeof(double) * (size_t)r.second, stream_), "memset arena");
  } else if (!one_pass_init) {
    HIPCHK(hipMemsetAsync(d_L_, 0, sizeof(double) * (size_t)S.arena, stream_), "memset arena");
  }
  // the "last reader" counters of the fused panel launches return to zero by themselves; a
  // factorization that was cut short (a failed launch, the watchdog) may have left some behind
  if (!prog_.panel_units.empty())
    HIPCHK(hipMemsetAsync(d_panel_cnt_, 0, sizeof(int) * 2 * prog_.panel_units.size(), stream_), "memset counters");
  const int big = INT_MAX;
  *h_flag_ = big;
  HIPCHK(hipMemcpyAsync(d_flag_, h_flag_, sizeof(int), hipMemcpyHostToDevice, stream_), "flag init");
  if (one_pass_init)
    launch_init_arena(stream_, d_L_, S.arena, val_src_ ? val_src_ : d_val_, d_init_cptr_, d_init_loc_, d_init_src_);
  else
    launch_scatter_val(stream_, d_L_, val_src_ ? val_src_ : d_val_, d_map_dst_, d_map_src_, nmap_);
  if (!prog_.exchanges.empty() || !prog_.sub_tasks.empty()) {
    // (the subtree tasks are the first launch of the side stream and wait for nothing else.)
    // A partitioned program may have an exchange as its FIRST launch on a stream other than this one
    // (a rank that owns no subtree: its phase 1 is empty, and the per-level reduce-scatters of a
    // distributed top tree run on the side stream): nothing would order its pack behind the clearing
    // of the arena and the scatter of the values above.  Every other stream starts behind them.
    HIPCHK(hipEventRecord(ev_init_, stream_), "event");
    for (int i = 0; i < ST_COUNT; ++i)
      if (streams_[i] && streams_[i] != stream_) HIPCHK(hipStreamWaitEvent(streams_[i], ev_init_, 0), "init wait");
  }
  stats_.launches = (int)prog_.launches.size() + 1;
  if (!prog_.exchanges.empty() && !xbuf_) return fail(-10, "exchange buffer not set", hipSuccess);
  return run_from(0);
}

// Launches [first, ...) until the next exchange point (packed, awaiting_exchange_) or the end.
int Engine::run_from(size_t first) {
  for (size_t i = first; i < prog_.launches.size(); ++i) {
    const Launch& l = prog_.launches[i];
    if (l.kind == L_EXCHANGE) {
      int rc = pre_exchange(l);
      if (rc) return rc;
      cur_x_ = i;
      awaiting_exchange_ = true;
      return 0;
    }
    int rc = enqueue_launch(l, false);
    if (rc) return rc;
  }
  awaiting_exchange_ = false;
  return finish_enqueue();
}

// The part of an exchange in front of the collective: its dependencies, then what this rank
// contributes goes into the exchange buffer (all on the chain stream, where the caller then
// enqueues the collective).
// the stream an exchange runs on: pack, collective and unpack (the chain stream, or -- the per-level
// reduce-scatters of a distributed top tree in the multi-stream program -- the side stream, so that
// the chunks of the upper levels travel while the lowest top level is already being factorized)
hipStream_t Engine::exchange_stream(const Launch& X) const {
  return (X.stream >= 0 && X.stream < ST_COUNT && streams_[X.stream]) ? streams_[X.stream] : stream_;
}

int Engine::pre_exchange(const Launch& X) {
  const Exchange& E = prog_.exchanges[(size_t)X.first];
  hipStream_t xs = exchange_stream(X);
  for (int w : X.wait)
    if (w >= 0) HIPCHK(hipStreamWaitEvent(xs, dag_events_[w], 0), "exchange wait");
  for (int i = E.first_item; i < E.first_item + E.nitems; ++i) {
    const ExchangeItem& it = prog_.xitems[(size_t)i];
    if (E.kind == X_BCAST && it.root != opt_.rank) continue;   // the owner sends
    HIPCHK(hipMemcpyAsync(xbuf_ + it.xoff, (it.space ? d_dinv_ : d_L_) + it.off, sizeof(double) * (size_t)it.count,
                          hipMemcpyDeviceToDevice, xs), "pack exchange");
  }
  if (E.kind == X_REDUCE_ALL || E.kind == X_FLAG) launch_flag_pack(xs, d_flag_, xbuf_ + (E.elems - 1));
  HIPCHK(hipGetLastError(), "kernel launch");
  return 0;
}

// ... and behind it: what this rank needs comes out of the buffer, the exchange's event fires.
int Engine::post_exchange(const Launch& X) {
  const Exchange& E = prog_.exchanges[(size_t)X.first];
  hipStream_t xs = exchange_stream(X);
  for (int i = E.first_item; i < E.first_item + E.nitems; ++i) {
    const ExchangeItem& it = prog_.xitems[(size_t)i];
    if (E.kind == X_BCAST && it.root == opt_.rank) continue;          // already here
    if (E.kind == X_REDUCE_OWNER && it.root != opt_.rank) continue;   // somebody else's sum
    HIPCHK(hipMemcpyAsync((it.space ? d_dinv_ : d_L_) + it.off, xbuf_ + it.xoff, sizeof(double) * (size_t)it.count,
                          hipMemcpyDeviceToDevice, xs), "unpack exchange");
  }
  if (E.kind == X_REDUCE_ALL || E.kind == X_FLAG) launch_flag_unpack(xs, xbuf_ + (E.elems - 1), d_flag_);
  if (X.record >= 0) HIPCHK(hipEventRecord(dag_events_[X.record], xs), "exchange record");
  return 0;
}

// ---------------------------------------------------------------------------
// RCCL, resolved at run time from the librccl the process already has (the caller created the
// communicator with it; a Python process has torch's copy): no link-time dependency, one copy.
// ---------------------------------------------------------------------------
Rccl& rccl() {
  static Rccl r = [] {
    Rccl q;
    const char* names[] = {"librccl.so.1", "librccl.so", "libnccl.so.2"};
    for (const char* nm : names)
      if ((q.handle = dlopen(nm, RTLD_NOW | RTLD_NOLOAD))) break;     // the copy the process already uses
    if (!q.handle)
      for (const char* nm : names)
        if ((q.handle = dlopen(nm, RTLD_NOW | RTLD_GLOBAL))) break;
    if (!q.handle) return q;
    q.all_reduce = (nccl_allreduce_t)dlsym(q.handle, "ncclAllReduce");
    q.reduce_scatter = (nccl_reducescatter_t)dlsym(q.handle, "ncclReduceScatter");
    q.broadcast = (nccl_broadcast_t)dlsym(q.handle, "ncclBroadcast");
    q.group_start = (nccl_group_t)dlsym(q.handle, "ncclGroupStart");
    q.group_end = (nccl_group_t)dlsym(q.handle, "ncclGroupEnd");
    q.comm_count = (nccl_query_t)dlsym(q.handle, "ncclCommCount");
    q.comm_user_rank = (nccl_query_t)dlsym(q.handle, "ncclCommUserRank");
    q.err_string = (nccl_errstr_t)dlsym(q.handle, "ncclGetErrorString");
    return q;
  }();
  return r;
}

int Engine::set_communicator(void* nccl_comm) {
  if (status_) return status_;
  if (!nccl_comm) { comm_ = nullptr; return 0; }
  Rccl& R = rccl();
  if (!R.ok()) return fail(-10, "spllt_hip_set_communicator: librccl is not loadable", hipSuccess);
  int cnt = 0, rk = 0;
  NCCLCHK(R.comm_count(nccl_comm, &cnt), "ncclCommCount");
  NCCLCHK(R.comm_user_rank(nccl_comm, &rk), "ncclCommUserRank");
  // SPLLT_HIP_COMM_REHEARSAL=1: a communicator smaller than the partition is accepted (one-GPU
  // rehearsal of the call sequence: the sums then miss the other ranks' parts, broadcast roots
  // are taken modulo its size)
  // -- accepted only for a ONE-rank communicator (the one-GPU test of the call sequence), announced
  // on stderr, and remembered: spllt_hip_last_error says so for as long as the handle lives.
  static const bool rehearsal_env = std::getenv("SPLLT_HIP_COMM_REHEARSAL") != nullptr;
  const bool mismatch = cnt != opt_.nranks || rk != opt_.rank;
  const bool rehearsal = rehearsal_env && cnt == 1;
  if (mismatch && rehearsal) {
    comm_rehearsal_ = true;
    std::fprintf(stderr, "spllt-hip: WARNING: SPLLT_HIP_COMM_REHEARSAL: a one-rank communicator stands in for rank %d of %d "
                         "-- the collectives run, the factor of this handle is NOT the factor of the matrix\n",
                 opt_.rank, opt_.nranks);
  }
  if (mismatch && !rehearsal) {
    err_ = "spllt_hip_set_communicator: the communicator is rank " + std::to_string(rk) + " of " + std::to_string(cnt) +
           ", the partition (spllt_hip_set_partition) is rank " + std::to_string(opt_.rank) + " of " +
           std::to_string(opt_.nranks);
    std::fprintf(stderr, "spllt-hip: %s\n", err_.c_str());
    return -10;
  }
  comm_ = nccl_comm;
  comm_rank_ = rk;
  comm_size_ = cnt;
  if (!xbuf_ && prog_.xbuf_elems > 0) {      // the exchange buffer is the library's own in this mode
    HIPCHK(dalloc((void**)&xbuf_, sizeof(double) * (size_t)prog_.xbuf_elems), "hipMalloc(exchange buffer)");
    HIPCHK(hipMemset(xbuf_, 0, sizeof(double) * (size_t)prog_.xbuf_elems), "hipMemset(exchange buffer)");
  }
  if (opt_.nranks > 1 && !d_owned_) {
    // a rank's share of a distributed vector: its own subtrees; rank 0 also the top tree
    std::vector<double> keep((size_t)S_->n, 0.0);
    for (int s = 0; s < S_->nnodes; ++s) {
      const int own = owner_[(size_t)s];
      const bool mine = own == opt_.rank || (own < 0 && opt_.rank == 0);
      if (mine)
        for (int p = S_->sptr[s]; p < S_->sptr[s + 1]; ++p) keep[(size_t)p] = 1.0;
    }
    HIPCHK(dev_upload(&d_owned_, keep), "upload owner mask");
  }
  return 0;
}

// the collective of one exchange on the exchange buffer, in place, enqueued on the engine's stream
// (between pre_exchange's pack and post_exchange's unpack)
int Engine::collective(const Exchange& E, hipStream_t xs) {
  Rccl& R = rccl();
  if (E.kind == X_REDUCE_ALL || E.kind == X_FLAG) {
    NCCLCHK(R.all_reduce(xbuf_, xbuf_, (size_t)E.elems, kNcclDouble, kNcclSum, comm_, xs), "ncclAllReduce");
  } else if (E.kind == X_REDUCE_OWNER) {
    // in place: rank r receives into its own chunk of the region (the region of this level's
    // exchange ends at E.elems: schedule.cpp)
    double* region = xbuf_ + (E.elems - (int64_t)opt_.nranks * E.chunk);
    NCCLCHK(R.reduce_scatter(region, region + (int64_t)comm_rank_ * E.chunk, (size_t)E.chunk, kNcclDouble, kNcclSum,
                             comm_, xs), "ncclReduceScatter");
  } else if (E.kind == X_BCAST) {
    // one broadcast per root (the items of a root are contiguous in the buffer), as one group
    // (a failed broadcast does not leave the group open: ncclGroupEnd is always reached -- the
    // communicator would stay in group mode and the other ranks in the collective -- and the first
    // error is reported afterwards)
    NCCLCHK(R.group_start(), "ncclGroupStart");
    int first_err = 0;
    for (int i = E.first_item; i < E.first_item + E.nitems;) {
      const ExchangeItem& a = prog_.xitems[(size_t)i];
      int64_t cnt = 0;
      int j = i;
      for (; j < E.first_item + E.nitems && prog_.xitems[(size_t)j].root == a.root &&
             prog_.xitems[(size_t)j].xoff == a.xoff + cnt; ++j)
        cnt += prog_.xitems[(size_t)j].count;
      const int r = R.broadcast(xbuf_ + a.xoff, xbuf_ + a.xoff, (size_t)cnt, kNcclDouble, a.root % comm_size_, comm_,
                                xs);
      if (r != 0 && first_err == 0) first_err = r;
      i = j;
    }
    const int rend = R.group_end();
    NCCLCHK(first_err, "ncclBroadcast");
    NCCLCHK(rend, "ncclGroupEnd");
  }
  return 0;
}

int Engine::run_exchanges() {
  if (status_) return status_;
  while (awaiting_exchange_) {
    if (!comm_) return 0;                     // the caller drives the exchanges (spllt_hip_continue)
    const Exchange& E = prog_.exchanges[(size_t)prog_.launches[cur_x_].first];
    int rc = collective(E, exchange_stream(prog_.launches[cur_x_]));
    if (rc) return rc;
    rc = continue_after_exchange();
    if (rc) return rc;
  }
  return 0;
}

int Engine::sync_phase() {
  if (status_) return status_;
  for (hipStream_t st : streams_)
    if (st) {
      int rc = sync_stream(st, "stream sync");
      if (rc) return rc;
    }
  return 0;
}

int Engine::continue_after_exchange() {
  if (status_) return status_;
  if (!awaiting_exchange_) return -10;
  HIPCHK(hipSetDevice(device_), "hipSetDevice");
  int rc = post_exchange(prog_.launches[cur_x_]);
  if (rc) return rc;
  rc = run_from(cur_x_ + 1);
  if (rc) return rc;
  if (!awaiting_exchange_) HIPCHK(hipEventRecord(ev1_, stream_), "event");
  return 0;
}

int Engine::factor_async_dev(const double* val_dev, int64_t nnz) {
  if (status_) return status_;
  if (nnz != S_->nnzA) return -10;
  z_valid_ = false;
  fadj_state_ = FADJ_UNSEEDED;
  factored_ = true;
  ud_invalid_ = false;
  double t0 = now_ms();
  HIPCHK(hipSetDevice(device_), "hipSetDevice");
  HIPCHK(hipEventRecord(ev0_, stream_), "event");
  // Eager launches read the caller's device array directly (it must stay valid and unchanged until
  // spllt_hip_wait: include/spllt_hip.h) -- the copy into the engine's own buffer was 88 MB each way
  // on the bench workload, 60 us in front of every factorization.  A graph replay has the engine's
  // buffer baked into its nodes: there the values are copied.
  val_src_ = nullptr;
  if (val_dev != d_val_) {
    if (replays_graph())
      HIPCHK(hipMemcpyAsync(d_val_, val_dev, sizeof(double) * (size_t)nnz, hipMemcpyDeviceToDevice, stream_), "val D2D");
    else
      val_src_ = val_dev;
  }
  HIPCHK(hipEventRecord(ev_h2d_, stream_), "event");
  int rc = enqueue_program();
  if (rc) return rc;
  if (comm_ && (rc = run_exchanges())) return rc;
  HIPCHK(hipEventRecord(ev1_, stream_), "event");
  pending_ = true;
  stats_.submit_ms = now_ms() - t0;
  return 0;
}

int Engine::factor_async(const double* val_host, int64_t nnz) {
  if (status_) return status_;
  if (nnz != S_->nnzA) return -10;
  z_valid_ = false;
  fadj_state_ = FADJ_UNSEEDED;
  factored_ = true;
  ud_invalid_ = false;
  double t0 = now_ms();
  HIPCHK(hipSetDevice(device_), "hipSetDevice");
  HIPCHK(hipEventRecord(ev0_, stream_), "event");
  val_src_ = nullptr;            // (the values go through the engine's own buffer)
  crumb("factor: H2D of val");
  // test hook (tests/test_gpu_parity.py::test_submission_deadline): a runtime call that sits
  if (const char* e = std::getenv("SPLLT_HIP_TEST_STALL_MS")) std::this_thread::sleep_for(std::chrono::milliseconds(std::atoi(e)));
  static const bool direct_h2d = [] { const char* e = std::getenv("SPLLT_HIP_H2D"); return e && std::string(e) == "direct"; }();
  if (direct_h2d) {
    HIPCHK(hipMemcpyAsync(d_val_, val_host, sizeof(double) * (size_t)nnz, hipMemcpyHostToDevice, stream_), "val H2D");
  } else {
    int rc = stage_val(val_host, nnz);
    if (rc) return rc;
  }
  HIPCHK(hipEventRecord(ev_h2d_, stream_), "event");
  crumb("factor: enqueueing the program");
  int rc = enqueue_program();
  if (rc) return rc;
  if (comm_ && (rc = run_exchanges())) return rc;
  crumb("factor: enqueued");
  HIPCHK(hipEventRecord(ev1_, stream_), "event");
  pending_ = true;
  stats_.submit_ms = now_ms() - t0;
  return 0;
}

int Engine::wait() {
  if (status_) return status_;
  if (!pending_) return 0;
  crumb("wait: polling the chain stream");
  if (awaiting_exchange_) return sync_phase();  // not finished: only drain phase 1
  {
    int rc = sync_stream(stream_, "stream sync");
    if (rc) return rc;
  }
  pending_ = false;
  crumb("wait: done");
  float ms = 0;
  if (hipEventElapsedTime(&ms, ev0_, ev1_) == hipSuccess) stats_.device_ms = ms;
  if (hipEventElapsedTime(&ms, ev0_, ev_h2d_) == hipSuccess) stats_.h2d_ms = ms;
  npd_col_ = -1;
  if (*h_flag_ != INT_MAX) {
    npd_col_ = *h_flag_ == INT_MAX - 1 ? -1 : *h_flag_ - 1;   // -1: reported by another rank
    return kErrNotPosDef;
  }
  return 0;
}

// device -> pageable host memory through the two pinned staging buffers of stage_val (the mirror
// image: the DMA of chunk k + 1 flies while the host copies chunk k out; every wait has the
// deadline).  A plain hipMemcpy into pageable memory moved the 1.5 GB factor of the bench workload
// at 3.2 GB/s (the runtime stages it itself, one small buffer at a time).
int Engine::staged_d2h(void* out_host, const void* src_dev, size_t bytes) {
  if (bytes == 0) return 0;
  const size_t chunk = kH2dChunk;
  if (h2d_chunk_ != chunk) {
    for (int i = 0; i < 2; ++i) {
      if (h2d_busy_[i]) { int rc = wait_event(h2d_ev_[i], "staging"); if (rc) return rc; h2d_busy_[i] = false; }
      if (h2d_buf_[i]) pin_release(h2d_buf_[i], h2d_chunk_);
      h2d_buf_[i] = nullptr;
    }
    h2d_chunk_ = chunk;
  }
  for (int i = 0; i < 2; ++i) {
    if (!h2d_buf_[i]) HIPCHK(pin_alloc(&h2d_buf_[i], chunk), "hipHostMalloc(staging)");
    if (!h2d_ev_[i]) HIPCHK(hipEventCreateWithFlags(&h2d_ev_[i], hipEventDisableTiming), "hipEventCreate");
    if (h2d_busy_[i]) { int rc = wait_event(h2d_ev_[i], "staging"); if (rc) return rc; h2d_busy_[i] = false; }
  }
  char* dst = reinterpret_cast<char*>(out_host);
  const char* src = reinterpret_cast<const char*>(src_dev);
  const size_t nchunk = (bytes + chunk - 1) / chunk;
  auto issue = [&](size_t k) -> int {
    const size_t off = k * chunk, len = std::min(chunk, bytes - off);
    HIPCHK(hipMemcpyAsync(h2d_buf_[k & 1], src + off, len, hipMemcpyDeviceToHost, stream_), "L D2H");
    HIPCHK(hipEventRecord(h2d_ev_[k & 1], stream_), "event");
    return 0;
  };
  int rc = issue(0);
  if (rc) return rc;
  for (size_t k = 0; k < nchunk; ++k) {
    if (k + 1 < nchunk && (rc = issue(k + 1))) return rc;
    if ((rc = wait_event(h2d_ev_[k & 1], "L D2H staging"))) return rc;
    const size_t off = k * chunk, len = std::min(chunk, bytes - off);
    std::memcpy(dst + off, h2d_buf_[k & 1], len);
  }
  return 0;
}

int Engine::download(double* out, int64_t count) {
  if (status_) return status_;
  if (count > S_->arena) count = S_->arena;
  HIPCHK(hipSetDevice(device_), "hipSetDevice");
  if (loc_off_.empty()) return staged_d2h(out, d_L_, sizeof(double) * (size_t)count);
  // a rank's arena is packed: back into the global layout (zero where nothing is held here)
  std::vector<double> tmp((size_t)std::max<int64_t>(1, arena_elems_));
  {
    int rc = staged_d2h(tmp.data(), d_L_, sizeof(double) * (size_t)arena_elems_);
    if (rc) return rc;
  }
  std::memset(out, 0, sizeof(double) * (size_t)count);
  for (int b = 0; b < S_->nbcol(); ++b) {
    if (loc_off_[(size_t)b] < 0) continue;
    const int64_t off = S_->bcols[b].off, cnt = (int64_t)S_->bcols[b].nrow * S_->bcols[b].width;
    if (off >= count) continue;
    std::memcpy(out + off, tmp.data() + loc_off_[(size_t)b], sizeof(double) * (size_t)std::min(cnt, count - off));
  }
  return 0;
}

// ---- selected inversion --------------------------------------------------------------------------
int Engine::prepare_selinv() {
  if (selinv_ready_) return 0;
  const Symbolic& S = *S_;
  if (build_selinv_program(S, prog_.pw, prog_.cb, siprog_)) {
    feature_err_ = "selected inversion: the row structure of a node is not contained in its ancestors'";
    return -10;
  }
  TableStager tab;
  tab.add(&d_siunits_, siprog_.units);
  tab.add(&d_sitiles_, siprog_.tiles);
  tab.add(&d_sirows_, siprog_.rows);
  tab.add(&d_sirelpos_, siprog_.relpos);
  tab.add(&d_sidiag_, siprog_.diag_pos);
  // (a failure here leaves the factor and the solve usable: the engine's status is not touched)
  auto t = take();
  t.tables(tab, &d_selinv_tables_);
  if (t.ok()) t.check(ensure_order());
  t(&d_siout_, sizeof(double) * ((size_t)S.n + 1));
  if (!t.ok()) {
    feature_err_ = std::string("selected inversion: not enough device memory for the program tables (") +
                   hipGetErrorString(t.error()) + ")";
    return alloc_code(t.error());
  }
  t.commit();
  selinv_ready_ = true;
  return 0;
}

void Engine::owned_info(int64_t out[2]) const {
  out[0] = (int64_t)owned_.size();
  out[1] = 0;
  for (const auto& b : owned_) out[1] += (int64_t)b.second;
}

void Engine::release_buffer(void* p) {
  for (size_t i = 0; i < owned_.size(); ++i)
    if (owned_[i].first == p) {
      dev_release(owned_[i].first, owned_[i].second, device_);
      owned_.erase(owned_.begin() + (long)i);
      return;
    }
}

int Engine::selected_inverse() {
  feature_err_.clear();
  if (status_) return status_;
  if (pending_) return -10;   // (the caller waits first)
  HIPCHK(hipSetDevice(device_), "hipSetDevice");
  int rc = prepare_selinv();
  if (rc) return rc;
  if (!d_Z_) {
    // the Z arena (L's size) and the scratch: a failure here leaves the factor usable
    const size_t zb = sizeof(double) * (size_t)std::max<int64_t>(1, S_->arena);
    const size_t sb = sizeof(double) * (size_t)std::max<int64_t>(1, siprog_.scratch_size);
    auto t = take();
    t(&d_Z_, zb);
    if (!d_siscratch_) t(&d_siscratch_, sb);
    if (!t.ok()) {
      feature_err_ = "selected inversion: not enough device memory for the inverse arena (" + std::to_string(zb >> 20) +
                     " MiB) and its scratch (" + std::to_string(sb >> 20) + " MiB)";
      return -1;
    }
    t.commit();
    si_users_.hold();
  }
  z_valid_ = false;
  for (const SelinvLaunch& l : siprog_.launches)
    launch_selinv(stream_, l, d_siunits_, d_sitiles_, d_sirows_, d_sirelpos_, d_L_, d_dinv_, d_Z_, d_siscratch_);
  HIPCHK(hipGetLastError(), "selinv launch");
  if ((rc = sync_stream(stream_, "selinv sync"))) return rc;
  z_valid_ = true;
  return 0;
}

int Engine::download_inverse(double* out, int64_t count) {
  feature_err_.clear();
  if (status_) return status_;
  if (!z_valid_) return -10;
  HIPCHK(hipSetDevice(device_), "hipSetDevice");
  return staged_d2h(out, d_Z_, sizeof(double) * (size_t)std::min<int64_t>(count, S_->arena));
}

int Engine::inverse_diag(double* out, int n) {
  feature_err_.clear();
  if (status_) return status_;
  if (!z_valid_ || n != S_->n) return -10;
  HIPCHK(hipSetDevice(device_), "hipSetDevice");
  launch_selinv_diag_gather(stream_, d_Z_, d_sidiag_, d_order_, n, d_siout_);
  HIPCHK(hipGetLastError(), "selinv diag launch");
  HIPCHK(hipMemcpyAsync(out, d_siout_, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, stream_), "diag D2H");
  return sync_stream(stream_, "selinv diag sync");
}

int Engine::log_det(double* out) {
  feature_err_.clear();
  if (status_) return status_;
  if (pending_) return -10;
  HIPCHK(hipSetDevice(device_), "hipSetDevice");
  int rc = prepare_selinv();
  if (rc) return rc;
  launch_log_det(stream_, d_L_, d_sidiag_, S_->n, d_siout_ + S_->n);
  HIPCHK(hipGetLastError(), "log det launch");
  HIPCHK(hipMemcpyAsync(out, d_siout_ + S_->n, sizeof(double), hipMemcpyDeviceToHost, stream_), "log det D2H");
  return sync_stream(stream_, "log det sync");
}

int Engine::release_inverse() {
  feature_err_.clear();
  if (status_) return status_;
  z_valid_ = false;
  if (d_Z_) {
    HIPCHK(hipSetDevice(device_), "hipSetDevice");
    if (int rc = sync_stream(stream_, "selinv release")) return rc;
    give_back(d_Z_, d_sipat_);
    si_users_.drop([this] { give_back(d_siscratch_); });
  }
  return 0;
}

// ---- reverse-mode derivative of the factor ---------------------------------------------------------
// the seed kernel's tables (block columns, (block column, strip) tiles, position -> variable): from the
// Symbolic structure alone, shared by the single arena and the arenas of a batch
int Engine::prepare_fadj_tables() {
  const Symbolic& S = *S_;
  if (!d_fadj_tables_) {
    std::vector<FadjCol> cols((size_t)S.nbcol());
    std::vector<UpdTile> tiles;
    for (int b = 0; b < S.nbcol(); ++b) {
      const BlockCol& bc = S.bcols[(size_t)b];
      cols[(size_t)b] = FadjCol{bc.off, S.rptr[(size_t)bc.node] + bc.r0, bc.width, bc.nrow, S.sptr[(size_t)bc.node] + bc.r0, 0};
      for (int t = 0; t * kSelinvTile < bc.nrow; ++t) tiles.push_back(UpdTile{b, (short)t, 0});
    }
    TableStager tab;
    tab.add(&d_facols_, cols);
    tab.add(&d_fatiles_, tiles);
    tab.add(&d_faporder_, S.porder);
    auto t = take();
    t.tables(tab, &d_fadj_tables_);
    if (!t.ok()) {
      feature_err_ = std::string("factor adjoint: not enough device memory for the seed tables (") + hipGetErrorString(t.error()) + ")";
      return alloc_code(t.error());
    }
    t.commit();
    fa_ntiles_ = (int64_t)tiles.size();
  }
  return 0;
}

int Engine::prepare_fadj() {
  int rc = prepare_selinv();
  if (rc) return rc;
  if ((rc = prepare_fadj_tables())) return rc;
  const Symbolic& S = *S_;
  if (!d_G_) {   // (hence unseeded)
    const size_t gb = sizeof(double) * (size_t)std::max<int64_t>(1, S.arena);
    const size_t sb = sizeof(double) * (size_t)std::max<int64_t>(1, siprog_.scratch_size);
    auto t = take();
    t(&d_G_, gb);
    if (!d_siscratch_) t(&d_siscratch_, sb);
    if (!t.ok()) {
      feature_err_ = "factor adjoint: not enough device memory for the adjoint arena (" + std::to_string(gb >> 20) +
                     " MiB) and the scratch (" + std::to_string(sb >> 20) + " MiB)";
      return -1;
    }
    t.commit();
    si_users_.hold();
  }
  return 0;
}

int Engine::fadj_seed(int nvec, const double* a, const double* b, int64_t ld, double alpha, bool accumulate,
                      int order_flags, bool dev) {
  feature_err_.clear();
  if (status_) return status_;
  if (pending_ || !a || !b || nvec < 0 || ld < S_->n || opt_.nranks > 1) return -10;
  if (accumulate && fadj_state_ != FADJ_SEEDED) {
    feature_err_ = "factor adjoint: accumulate = 1 needs a seeded adjoint arena of the current factor (this one is " +
                   std::string(fadj_state_ == FADJ_SWEPT ? "swept" : "unseeded or stale") + ")";
    return -10;
  }
  HIPCHK(hipSetDevice(device_), "hipSetDevice");
  int rc = prepare_fadj();
  if (rc) return rc;
  const int n = S_->n;
  double* stage = nullptr;
  const double *ad = a, *bd = b;
  int64_t ldd = ld;
  if (!dev && nvec > 0 && n > 0) {
    auto t = take();
    t(&stage, sizeof(double) * 2 * (size_t)nvec * (size_t)n);
    if (!t.ok()) {
      feature_err_ = std::string("factor adjoint: not enough device memory to stage the seed vectors (") + hipGetErrorString(t.error()) + ")";
      return alloc_code(t.error());
    }
    t.commit();   // (returned below, once the stream has drained)
    if ((rc = copy_vectors(true, stage, const_cast<double*>(a), ld, nvec, "seed H2D"))) return rc;
    if ((rc = copy_vectors(true, stage + (int64_t)nvec * n, const_cast<double*>(b), ld, nvec, "seed H2D"))) return rc;
    ad = stage;
    bd = stage + (int64_t)nvec * n;
    ldd = n;
  }
  if (!accumulate) fadj_state_ = FADJ_UNSEEDED;
  launch_fadj_seed(stream_, d_fatiles_, fa_ntiles_, d_facols_, d_rlist_, d_faporder_, d_G_, nvec, ad, bd, ldd, alpha,
                   accumulate, order_flags);
  HIPCHK(hipGetLastError(), "factor adjoint seed launch");
  rc = sync_stream(stream_, "factor adjoint seed sync");
  if (!rc) give_back(stage);
  if (rc) return rc;
  fadj_state_ = FADJ_SEEDED;
  return 0;
}

int Engine::fadj_upload(const double* host_arena, int64_t count) {
  feature_err_.clear();
  if (status_) return status_;
  if (pending_ || !host_arena || count < S_->arena || opt_.nranks > 1) return -10;
  HIPCHK(hipSetDevice(device_), "hipSetDevice");
  int rc = prepare_fadj();
  if (rc) return rc;
  fadj_state_ = FADJ_UNSEEDED;
  if (S_->arena > 0)
    HIPCHK(hipMemcpyAsync(d_G_, host_arena, sizeof(double) * (size_t)S_->arena, hipMemcpyHostToDevice, stream_), "adjoint H2D");
  if ((rc = sync_stream(stream_, "factor adjoint upload sync"))) return rc;
  fadj_state_ = FADJ_SEEDED;
  return 0;
}

int Engine::fadj_download(double* out, int64_t count) {
  feature_err_.clear();
  if (status_) return status_;
  if (fadj_state_ == FADJ_UNSEEDED || !out) return -10;
  HIPCHK(hipSetDevice(device_), "hipSetDevice");
  return staged_d2h(out, d_G_, sizeof(double) * (size_t)std::min<int64_t>(count, S_->arena));
}

int Engine::fadj_sweep(double* gval, bool dev) {
  feature_err_.clear();
  if (status_) return status_;
  if (pending_ || !gval || opt_.nranks > 1) return -10;
  if (fadj_state_ != FADJ_SEEDED) {
    feature_err_ = "factor adjoint: the sweep needs a freshly seeded adjoint arena of the current factor (this one is " +
                   std::string(fadj_state_ == FADJ_SWEPT ? "already swept" : "unseeded or stale") + ")";
    return -10;
  }
  HIPCHK(hipSetDevice(device_), "hipSetDevice");
  int rc = prepare_fadj();
  if (rc) return rc;
  const int64_t nnz = S_->nnzA;
  if (!dev && !d_gpat_ && nnz > 0) {
    auto t = take();
    t(&d_gpat_, sizeof(double) * (size_t)nnz);
    if (!t.ok()) {
      feature_err_ = std::string("factor adjoint: not enough device memory for the gathered gradient (") + hipGetErrorString(t.error()) + ")";
      return alloc_code(t.error());
    }
    t.commit();
  }
  fadj_state_ = FADJ_UNSEEDED;   // (a sweep that fails half way leaves nothing to read)
  for (const SelinvLaunch& l : siprog_.launches)
    launch_fadj(stream_, l, d_siunits_, d_sitiles_, d_sirows_, d_sirelpos_, d_L_, d_dinv_, d_G_, d_siscratch_);
  HIPCHK(hipGetLastError(), "factor adjoint launch");
  if (nnz > 0) {
    if ((rc = gather_inverse_on_pattern(dev ? gval : d_gpat_, d_G_))) return rc;
    if (!dev && (rc = staged_d2h(gval, d_gpat_, sizeof(double) * (size_t)nnz))) return rc;
  } else if ((rc = sync_stream(stream_, "factor adjoint sync"))) {
    return rc;
  }
  fadj_state_ = FADJ_SWEPT;
  return 0;
}

int Engine::release_factor_adjoint() {
  feature_err_.clear();
  if (status_) return status_;
  fadj_state_ = FADJ_UNSEEDED;
  if (d_G_) {
    HIPCHK(hipSetDevice(device_), "hipSetDevice");
    if (int rc = sync_stream(stream_, "factor adjoint release")) return rc;
    give_back(d_G_, d_gpat_);
    si_users_.drop([this] { give_back(d_siscratch_); });
  }
  return 0;
}

// A^-1 at the entries of the analysed pattern into nnz doubles of device memory: the gather kernel of the
// batched inversion with one member, enqueued on stream_ (what both readers below share)
int Engine::gather_inverse_on_pattern(double* out_dev, double* arena) {
  BatchSelinvView v{};   // one member, known to be valid: no flag
  v.v.nbatch = 1;
  v.Z = arena ? arena : d_Z_;
  if (launch_batch_selinv_pattern(stream_, v, d_map_dst_, d_map_src_, nmap_, out_dev, S_->nnzA) < 0) {
    feature_err_ = "inverse on pattern: the pattern has more entries than a grid holds work items";
    return -99;
  }
  HIPCHK(hipGetLastError(), "inverse on pattern launch");
  return sync_stream(stream_, "inverse on pattern sync");
}

int Engine::inverse_on_pattern(double* out) {
  feature_err_.clear();
  if (status_) return status_;
  if (!z_valid_ || !out || opt_.nranks > 1) return -10;
  const int64_t nnz = S_->nnzA;
  if (nnz == 0) return 0;
  HIPCHK(hipSetDevice(device_), "hipSetDevice");
  if (!d_sipat_) {
    auto t = take();
    t(&d_sipat_, sizeof(double) * (size_t)nnz);
    if (!t.ok()) {
      feature_err_ = std::string("inverse on pattern: not enough device memory for the gathered entries (") + hipGetErrorString(t.error()) + ")";
      return -1;
    }
    t.commit();
  }
  if (int rc = gather_inverse_on_pattern(d_sipat_)) return rc;
  return staged_d2h(out, d_sipat_, sizeof(double) * (size_t)nnz);
}

int Engine::inverse_on_pattern_dev(double* out_dev) {
  feature_err_.clear();
  if (status_) return status_;
  if (!z_valid_ || !out_dev || opt_.nranks > 1) return -10;
  if (S_->nnzA == 0) return 0;
  HIPCHK(hipSetDevice(device_), "hipSetDevice");
  return gather_inverse_on_pattern(out_dev);
}

// ---- sampled outer product on the analysed pattern ---------------------------------------------------
int Engine::pattern_outer(int nbatch, int nvec, const double* u, int64_t ldu, const double* v, int64_t ldv,
                          double alpha, double* out, int64_t ldout, bool dev) {
  feature_err_.clear();
  if (status_) return status_;
  const int n = S_->n;
  const int64_t nnz = S_->nnzA;
  if (!u || !v || !out || nbatch < 0 || nvec < 0 || ldu < n || ldv < n || ldout < nnz) return -10;
  if (opt_.nranks > 1) return -98;
  if (pending_) return -10;   // (the caller waits first)
  if (nbatch == 0 || nnz == 0) return 0;
  HIPCHK(hipSetDevice(device_), "hipSetDevice");
  if (!d_potab_) {
    std::vector<int> row, col;
    build_pattern_tables(*S_, row, col);
    TableStager tab;
    tab.add(&d_porow_, row);
    tab.add(&d_pocol_, col);
    auto t = take();
    t.tables(tab, &d_potab_);
    if (!t.ok()) {
      feature_err_ = std::string("pattern outer product: not enough device memory for the tables of the pattern (") +
                     hipGetErrorString(t.error()) + ")";
      return alloc_code(t.error());
    }
    t.commit();
  }
  const int64_t nv = (int64_t)nbatch * nvec;
  const double *du = u, *dv = v;
  double* dout = out;
  int64_t dldu = ldu, dldv = ldv, dldout = ldout;
  if (!dev) {
    // the caller's arrays packed: 2 nv vectors of n doubles, then nbatch rows of nnz doubles
    const size_t need = 2 * (size_t)nv * (size_t)n + (size_t)nbatch * (size_t)nnz;
    if (need > po_stage_elems_ || !d_postage_) {
      if (d_postage_)
        if (int rc = sync_stream(stream_, "pattern outer product staging")) return rc;
      if (const hipError_t e = grow(&d_postage_, &po_stage_elems_, need)) {
        feature_err_ = "pattern outer product: not enough device memory to stage the vectors (" +
                       std::to_string((sizeof(double) * need) >> 20) + " MiB): " + hipGetErrorString(e);
        return alloc_code(e);
      }
    }
    double* su = d_postage_;
    double* sv = su + (size_t)nv * (size_t)n;
    dout = sv + (size_t)nv * (size_t)n;
    if (nv > 0) {
      if (int rc = copy_vectors_to_device(su, u, ldu, nv, "u H2D")) return rc;
      if (int rc = copy_vectors_to_device(sv, v, ldv, nv, "v H2D")) return rc;
    }
    du = su; dv = sv;
    dldu = dldv = n;
    dldout = nnz;
  }
  if (launch_pattern_outer(stream_, d_porow_, d_pocol_, nnz, nbatch, nvec, du, dldu, dv, dldv, alpha, dout, dldout) < 0) {
    feature_err_ = "pattern outer product: the pattern has more entries than a grid holds work items";
    return -99;
  }
  HIPCHK(hipGetLastError(), "pattern outer product launch");
  if (!dev)
    if (int rc = copy_vectors(false, dout, out, ldout, nbatch, "pattern outer product D2H", nnz)) return rc;
  return sync_stream(stream_, "pattern outer product sync");
}

// ---- low-rank update / downdate ---------------------------------------------------------------------
// Per pass of up to kUpdownVec columns of W: their entries scattered into the work array, then the block
// columns of the pass's plan in ascending order, each a generate launch (one workgroup: the diagonal square,
// the coefficients, the dinv slots) and, where it has rows below the square, an apply launch.  The launches of
// a sweep depend on each other through the work array: one stream, program order.
int Engine::updown(int k, const int* wptr, const int* wrow, const double* wval, int sign, const std::vector<int>& all,
                   const std::vector<int>& first) {
  feature_err_.clear();
  if (status_) return status_;
  if (opt_.nranks > 1) return -98;   // a rank of a partition holds a part of L only
  if (k < 0 || (k > 0 && (!wptr || !wrow || !wval)) || (sign != 1 && sign != -1) || (int)first.size() != k) return -10;
  if (pending_) {
    int rc = wait();
    if (rc) return rc;
  }
  if (!factored_ || ud_invalid_) {
    feature_err_ = "update: nothing has been factorized on this handle";
    return -10;
  }
  const Symbolic& S = *S_;
  for (int64_t& v : ud_info_) v = 0;
  ud_device_ms_ = 0.0;
  if (all.empty()) return 0;         // k = 0, or every column empty
  HIPCHK(hipSetDevice(device_), "hipSetDevice");
  int rc = prepare_solve();
  if (rc) return rc;
  // the passes, the positions of their entries in the work array and their plans (updown_stage.hpp); the values
  // of the entries, in that order
  UpdownStage st;
  stage_updown(k, wptr, wrow, S.order.data(), first.data(), kUpdownVec,
               [&](const int* pf, int nc, std::vector<int>& plan) { updown_paths(S, pf, nc, plan); }, st);
  std::vector<double> val(st.ent.size());
  for (size_t i = 0; i < val.size(); ++i) val[i] = wval[st.ent[i]];
  int maxw = 1;
  for (const BlockCol& B : S.bcols) maxw = std::max(maxw, B.width);
  const size_t wb = sizeof(double) * kUpdownVec * (size_t)std::max(1, S.n);
  const size_t cb = sizeof(double) * ((size_t)maxw * kUpdownVec * 3 + 2);
  const size_t pb = sizeof(int64_t) * st.pos.size(), vb = sizeof(double) * val.size();
  int64_t* d_pos = nullptr;
  double* d_val = nullptr;
  {
    // a failure leaves the factor and every solve usable, and nothing of this call allocated
    auto t = take();
    if (!d_udW_) {
      t(&d_udW_, wb);
      t(&d_udcoef_, cb);
      if (t.ok()) t.check(hipMemsetAsync(d_udW_, 0, wb, stream_));
    }
    t(&d_pos, pb);
    t(&d_val, vb);
    if (t.ok()) t.check(hipMemcpyAsync(d_pos, st.pos.data(), pb, hipMemcpyHostToDevice, stream_));
    if (t.ok()) t.check(hipMemcpyAsync(d_val, val.data(), vb, hipMemcpyHostToDevice, stream_));
    if (!t.ok()) {
      (void)hipGetLastError();
      (void)sync_stream(stream_, "update staging");   // (before the roll-back returns what a copy may still write)
      feature_err_ = "update: not enough device memory for the work array (" + std::to_string(wb >> 10) +
                     " KiB), the coefficient scratch and the entries of W: " + hipGetErrorString(t.error());
      return alloc_code(t.error());
    }
    t.commit();
  }
  int* d_flag = reinterpret_cast<int*>(d_udcoef_ + (size_t)maxw * kUpdownVec * 3);
  int64_t launches = 0;
  for (int p = 0; p < st.npass; ++p) {
    const int nc = st.pass_nc[(size_t)p];
    const int64_t e0 = st.pass_ptr[(size_t)p];
    if (p == 0) (void)hipEventRecord(ev0_, stream_);
    launch_updown_scatter(stream_, d_pos + e0, d_val + e0, st.pass_ptr[(size_t)p + 1] - e0, d_udW_, d_flag, p == 0);
    ++launches;
    for (int64_t i = st.plan_ptr[(size_t)p]; i < st.plan_ptr[(size_t)p + 1]; ++i) {
      const SolveUnit& u = sprog_.units[(size_t)st.plan[(size_t)i]];
      launch_updown_gen(stream_, u, d_L_, d_dinv_, d_udW_, d_udcoef_, d_flag, sign, nc);
      ++launches;
      if (u.nrow > u.w) {
        launch_updown_apply(stream_, u, d_L_, d_rlist_, d_udW_, d_udcoef_, sign, nc);
        ++launches;
      }
    }
  }
  int flag = INT_MAX;
  hipError_t le = hipGetLastError();
  if (le == hipSuccess) le = hipEventRecord(ev1_, stream_);
  if (le == hipSuccess) le = hipMemcpyAsync(&flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, stream_);
  rc = sync_stream(stream_, "update sync");
  give_back(d_val, d_pos);
  z_valid_ = false;
  fadj_state_ = FADJ_UNSEEDED;
  if (le != hipSuccess || rc) {
    // the sweep did not finish: the arena is half modified and the work array may not be zero
    ud_invalid_ = true;
    give_back(d_udW_, d_udcoef_);
    return le != hipSuccess ? fail(kErrHip, "update launch", le) : rc;
  }
  float ms = 0;
  if (hipEventElapsedTime(&ms, ev0_, ev1_) == hipSuccess) ud_device_ms_ = ms;
  ud_info_[0] = (int64_t)all.size();
  for (int b : all) ud_info_[1] += (int64_t)S.bcols[(size_t)b].nrow * S.bcols[(size_t)b].width;
  ud_info_[2] = launches;
  ud_info_[3] = st.npass;
  if (flag != INT_MAX) {
    npd_col_ = flag - 1;
    ud_invalid_ = true;
    feature_err_ = "downdate: the modified matrix is not positive definite (pivot column " + std::to_string(flag) +
                   " in elimination order); the factor is invalid until the next factorization";
    return kErrNotPosDef;
  }
  return 0;
}

// ---- low-rank update / downdate of the factors of a batch ---------------------------------------------
// The launches of Engine::updown with every launch carrying all members (batch_updown.hip).  The units are the
// batch's own (bt_.sprog, pw = cb = 64): slot p of a block column at dinv_off + 4096 p with row stride = the
// panel's width, which is what k_batch_chain writes (ldw = ce - cs = pn, panels of 64) and what ud_gen_block
// advances by (pn x pn per panel, every panel but the last 64 wide).
void Engine::drop_updown_batch() {
  give_back(bud_.W, bud_.coef, bud_.flag);
  bud_.capacity = 0;
  for (int64_t& v : bud_.info) v = 0;
  bud_.device_ms = 0.0;
}

int Engine::release_updown_batch() {
  int rc;
  if (!enter_release(bud_.W || bud_.coef || bud_.flag, "batch update release", &rc)) return rc;
  drop_updown_batch();
  return 0;
}

int Engine::updown_batch(int k, const int* wptr, const int* wrow, const double* wval, int64_t ldw, bool dev, int sign,
                         const std::vector<int>& all, const std::vector<int>& first) {
  feature_err_.clear();
  if (status_) return status_;
  if (opt_.nranks > 1) return -98;
  if (k < 0 || (k > 0 && (!wptr || !wrow || !wval)) || (sign != 1 && sign != -1) || (int)first.size() != k) return -10;
  if (pending_ || bt_.nbatch <= 0) return -10;
  if (k > 0 && ldw < (int64_t)wptr[k] - 1) return -10;
  const Symbolic& S = *S_;
  const int nbatch = bt_.nbatch;
  for (int64_t& v : bud_.info) v = 0;
  bud_.device_ms = 0.0;
  if (all.empty()) return 0;         // k = 0, or every column empty
  HIPCHK(hipSetDevice(device_), "hipSetDevice");
  UpdownStage st;
  stage_updown(k, wptr, wrow, S.order.data(), first.data(), kUpdownVec,
               [&](const int* pf, int nc, std::vector<int>& plan) { updown_paths(S, pf, nc, plan); }, st);
  int maxw = 1;
  for (const BlockCol& B : S.bcols) maxw = std::max(maxw, B.width);
  const int64_t wstride = (int64_t)kUpdownVec * std::max(1, S.n), cstride = (int64_t)maxw * kUpdownVec * 3;
  const int64_t nent = (int64_t)wptr[k] - 1;   // (the members' values packed: row b of the staged copy)
  const size_t pb = sizeof(int64_t) * st.pos.size(), eb = sizeof(int) * st.ent.size();
  const size_t vb = dev ? 0 : sizeof(double) * (size_t)nbatch * (size_t)nent;
  int64_t* d_pos = nullptr;
  int* d_ent = nullptr;
  double* d_val = nullptr;
  {
    // a failure leaves the batch and the single factor usable, and nothing of this call allocated; a larger batch
    // takes the three per-member arrays again, together
    auto t = take();
    if (bud_.W && nbatch > bud_.capacity) drop_updown_batch();
    const bool fresh = !bud_.W;
    const size_t wbytes = sizeof(double) * (size_t)wstride * (size_t)nbatch;
    if (fresh) {
      t(&bud_.W, wbytes);
      t(&bud_.coef, sizeof(double) * (size_t)cstride * (size_t)nbatch);
      t(&bud_.flag, sizeof(int) * (size_t)nbatch);
      if (t.ok()) t.check(hipMemsetAsync(bud_.W, 0, wbytes, stream_));
    }
    t(&d_pos, pb);
    t(&d_ent, eb);
    if (!dev) t(&d_val, vb);
    if (t.ok()) t.check(hipMemcpyAsync(d_pos, st.pos.data(), pb, hipMemcpyHostToDevice, stream_));
    if (t.ok()) t.check(hipMemcpyAsync(d_ent, st.ent.data(), eb, hipMemcpyHostToDevice, stream_));
    if (!t.ok()) {
      (void)hipGetLastError();
      (void)sync_stream(stream_, "batch update staging");   // (before the roll-back returns what a copy may still write)
      feature_err_ = "batch update: not enough device memory for the work arrays of " + std::to_string(nbatch) +
                     " members (" + std::to_string(wbytes >> 10) + " KiB), the coefficient scratch and the entries of W: " +
                     hipGetErrorString(t.error());
      return alloc_code(t.error());
    }
    t.commit();
    if (fresh) {
      bud_.capacity = nbatch;
      bud_.wstride = wstride;
      bud_.cstride = cstride;
    }
  }
  const double* vd = wval;
  int64_t ldv = ldw;
  if (!dev) {
    if (int rc = copy_vectors_to_device(d_val, wval, ldw, nbatch, "batch update values H2D", nent)) {
      give_back(d_val, d_ent, d_pos);
      return rc;
    }
    vd = d_val;
    ldv = nent;
  }
  BupdownView s;
  s.v = batch_view();
  s.Wd = bud_.W;
  s.coef = bud_.coef;
  s.udflag = bud_.flag;
  s.wstride = bud_.wstride;
  s.cstride = bud_.cstride;
  int64_t launches = 0;
  bool fits = true;
  auto count = [&](int made) { if (made < 0) fits = false; else launches += made; };
  for (int p = 0; p < st.npass && fits; ++p) {
    const int nc = st.pass_nc[(size_t)p];
    if (p == 0) (void)hipEventRecord(ev0_, stream_);
    count(launch_bupdown_scatter(stream_, s, d_pos + st.pass_ptr[(size_t)p], d_ent + st.pass_ptr[(size_t)p],
                                 st.pass_ptr[(size_t)p + 1] - st.pass_ptr[(size_t)p], vd, ldv, p == 0));
    for (int64_t i = st.plan_ptr[(size_t)p]; i < st.plan_ptr[(size_t)p + 1] && fits; ++i) {
      const SolveUnit& u = bt_.sprog.units[(size_t)st.plan[(size_t)i]];
      count(launch_bupdown_gen(stream_, s, u, sign, nc));
      count(launch_bupdown_apply(stream_, s, u, d_rlist_, sign, nc));
    }
  }
  hipError_t le = hipGetLastError();
  if (le == hipSuccess) le = hipEventRecord(ev1_, stream_);
  bud_.hflag_pending.assign((size_t)nbatch, INT_MAX);
  if (le == hipSuccess)
    le = hipMemcpyAsync(bud_.hflag_pending.data(), bud_.flag, sizeof(int) * (size_t)nbatch, hipMemcpyDeviceToHost, stream_);
  int rc = sync_stream(stream_, "batch update sync");
  give_back(d_val, d_ent, d_pos);
  bt_.z_valid = false;
  bt_.g_state = FADJ_UNSEEDED;
  ++bt_.generation;
  if (le != hipSuccess || rc || !fits) {
    // the sweep did not finish: the arenas are half modified and the work arrays may not be zero
    bt_.nbatch = 0;
    bt_.hflag.clear();
    drop_updown_batch();
    if (le != hipSuccess) return fail(kErrHip, "batch update launch", le);
    if (rc) return rc;
    feature_err_ = "batch update: a block column has more strips for ONE member than a grid holds; the batch is left "
                   "without members";
    return -99;
  }
  float ms = 0;
  if (hipEventElapsedTime(&ms, ev0_, ev1_) == hipSuccess) bud_.device_ms = ms;
  // the words of this call into the batch's flags, on the host and on the device (the scatter of a later pass has
  // merged what failed before it; what failed in the last pass has not been merged yet)
  int64_t served = 0, failed = 0;
  for (int b = 0; b < nbatch; ++b) {
    if (bt_.hflag[(size_t)b] != INT_MAX) continue;
    ++served;
    if (bud_.hflag_pending[(size_t)b] != INT_MAX) {
      bt_.hflag[(size_t)b] = bud_.hflag_pending[(size_t)b];
      ++failed;
    }
  }
  if (failed) {
    HIPCHK(hipMemcpyAsync(bt_.flag, bt_.hflag.data(), sizeof(int) * (size_t)nbatch, hipMemcpyHostToDevice, stream_),
           "batch update flags H2D");
    if ((rc = sync_stream(stream_, "batch update flags sync"))) return rc;
  }
  bud_.info[0] = (int64_t)all.size();
  for (int b : all) bud_.info[1] += (int64_t)S.bcols[(size_t)b].nrow * S.bcols[(size_t)b].width;
  bud_.info[2] = launches;
  bud_.info[3] = st.npass;
  bud_.info[4] = served;
  bud_.info[5] = failed;
  if (failed)
    feature_err_ = "batch downdate: " + std::to_string(failed) + " of " + std::to_string(nbatch) +
                   " members are not positive definite after the modification; they are skipped until the next "
                   "factor_batch (spllt_hip_batch_status)";
  return batch_failed();
}

// ---- batched factorization ------------------------------------------------------------------------
int build_batch_program(const Symbolic& S, Program& P, std::string* why, bool deterministic) {
  ScheduleOptions so;
  so.pw = 64;
  so.tile = 64;
  so.cb = 64;
  so.chain4 = false;
  so.lookahead = false;
  so.fused_panel = false;
  so.subtrees = false;
  so.env_switches = false;      // (SPLLT_CHAIN4=1 / SPLLT_SUBTREES=1 are experiments of the single-handle engine)
  so.deterministic = deterministic;   // (batch_repro.hip: MODE_BUFFER units + one L_GATHER launch per level)
  P = Program();
  build_program(S, so, P);
  auto bad = [&](const std::string& what) {
    if (why) *why = "batched factorization: the batch program holds " + what + ", which the batch kernels do not implement";
    return -99;
  };
  const int scatter_mode = deterministic ? MODE_BUFFER : MODE_SCATTER;   // how this program subtracts between nodes
  if (P.pw != 64 || !P.exchanges.empty()) return bad("a panel width other than 64 or an exchange");
  for (size_t i = 0; i < P.launches.size(); ++i) {
    const Launch& l = P.launches[i];
    if (l.kind != L_CHAIN && l.kind != L_GEMM && !(deterministic && l.kind == L_GATHER))
      return bad("launch kind " + std::to_string(l.kind));
    if (l.count <= 0) continue;
    if (l.kind == L_GATHER) {
      // a tile is at most 64 x 64 (the LDS tile of the gather kernel) and its items lie inside the scratch
      if (l.first < 0 || l.first + l.count > (int64_t)P.gather_tiles.size()) return bad("a gather launch outside its table");
      for (int64_t q = l.first; q < l.first + l.count; ++q) {
        const GatherTile& t = P.gather_tiles[(size_t)q];
        if (t.rows < 1 || t.rows > 64 || t.cols < 1 || t.cols > 64 || t.first < 0 || t.count < 0 ||
            (size_t)t.first + (size_t)t.count > P.gather_items.size())
          return bad("a gather tile larger than 64 x 64");
        for (int e = t.first; e < t.first + t.count; ++e) {
          const GatherItem& g = P.gather_items[(size_t)e];
          if (g.i0 < 0 || g.i1 < g.i0 || g.j0 < 0 || g.j1 < g.j0 || g.j1 > g.ld || g.buf_off < 0 ||
              g.buf_off + (int64_t)g.i1 * g.ld > P.scratch_size)
            return bad("a gather item outside the scratch");
        }
      }
      continue;
    }
    if (l.kind == L_CHAIN) {
      for (int64_t q = l.first; q < l.first + l.count; ++q) {
        const ChainUnit& u = P.chain_units[(size_t)q];
        if (u.pn < 1 || u.pn > kPanelMax || u.cs != u.c0 || u.ce != u.c0 + u.pn) return bad("a chain block wider than its panel");
      }
      continue;
    }
    if (l.tile != 32 && l.tile != 64) return bad("tile edge " + std::to_string(l.tile));
    for (int64_t q = l.first; q < l.first + l.count; ++q) {
      const UpdUnit& u = P.units[(size_t)P.tiles[(size_t)q].unit];
      if (u.mode != MODE_DIRECT && u.mode != scatter_mode && u.mode != MODE_TRSM) return bad("unit mode " + std::to_string(u.mode));
      if (u.mode == MODE_BUFFER && (u.d_ld != u.N || u.d_off < 0 || u.d_off + (int64_t)u.M * u.N > P.scratch_size))
        return bad("a BUFFER unit outside the scratch");
      if (u.mode == MODE_DIRECT && u.atomic) return bad("a DIRECT unit that subtracts with atomics");
      // a TRSM tile overwrites its own operand rows: it must cover all the unit's columns, and the K
      // window must be the inverted panel's
      if (u.mode == MODE_TRSM && (u.N > l.tile || u.nseg != 1 || u.klen != u.dinv_ld)) return bad("a TRSM unit wider than its tile");
    }
  }
  return 0;
}

void batch_diag_positions(const Symbolic& S, std::vector<int64_t>& pos) {
  pos.resize((size_t)S.n);
  for (int g = 0; g < S.n; ++g) {
    const int s = S.snode_of[g], k = g - S.sptr[s];
    const BlockCol& B = S.bcols[S.node_bcol0[s] + k / S.nb];
    pos[(size_t)g] = B.off + (int64_t)(k - B.r0) * B.width + (k - B.r0);
  }
}

BatchView Engine::batch_view() const {
  BatchView v;
  v.L = bt_.L;
  v.dinv = bt_.dinv;
  v.flag = bt_.flag;
  v.lstride = bt_.lstride;
  v.dstride = bt_.dstride;
  v.nbatch = bt_.nbatch;
  v.member_fast = bt_.member_fast;
  return v;
}

// program, solve program and index tables of the batch: built and uploaded once per engine
int Engine::prepare_batch() {
  if (bt_.ready) return 0;
  const Symbolic& S = *S_;
  int rc = build_batch_program(S, bt_.prog, &feature_err_);
  if (rc) return rc;
  build_solve_program(S, 64, 64, bt_.sprog);
  // the bucketed value map: the engine's own tables where its one-pass initialisation uploaded them
  std::vector<int64_t> cptr;
  std::vector<unsigned short> loc;
  std::vector<int> src;
  bt_.own_init = !(d_init_cptr_ && d_init_loc_ && d_init_src_);
  if (bt_.own_init) bucket_value_map(S, cptr, loc, src);
  std::vector<int64_t> diag;
  batch_diag_positions(S, diag);
  TableStager tab;
  tab.add(&bt_.units, bt_.prog.units);
  tab.add(&bt_.tiles, bt_.prog.tiles);
  tab.add(&bt_.chain, bt_.prog.chain_units);
  tab.add(&bt_.relpos, bt_.prog.relpos);
  if (bt_.own_init) {
    tab.add(&bt_.init_cptr, cptr);
    tab.add(&bt_.init_loc, loc);
    tab.add(&bt_.init_src, src);
  }
  tab.add(&bt_.diag, diag);
  tab.add(&bt_.sunits, bt_.sprog.units);
  tab.add(&bt_.slist, bt_.sprog.diag_list);
  tab.add(&bt_.stiles, bt_.sprog.tiles);
  // (a failure here leaves the single factorization usable: the engine's status is not touched)
  auto t = take();
  t.tables(tab, &bt_.d_tab);
  if (t.ok()) t.check(ensure_order());
  if (!t.ok()) {
    feature_err_ = std::string("batched factorization: the program tables could not be uploaded (") + hipGetErrorString(t.error()) + ")";
    return alloc_code(t.error());
  }
  t.commit();
  if (!bt_.own_init) {
    bt_.init_cptr = d_init_cptr_;
    bt_.init_loc = d_init_loc_;
    bt_.init_src = d_init_src_;
  }
  // experiment knob of scripts/factor_batch_bench.py (the A/B of the two grid mappings)
  if (const char* env = std::getenv("SPLLT_BATCH_MEMBER_FAST")) bt_.member_fast = std::atoi(env) != 0;
  bt_.ready = true;
  return 0;
}

// arenas, dinv scratch, flags and log-det slots for nbatch members; all or nothing
int Engine::reserve_batch(int nbatch, bool deterministic) {
  const bool want_f = deterministic && brp_.prog.scratch_size > 0;
  if (nbatch <= bt_.capacity) {
    if (!want_f || (brp_.fscratch && brp_.f_capacity >= bt_.capacity)) return 0;
    // the batch stands and the switch came later: the factor scratch alone, for the members the batch holds
    give_back(brp_.fscratch);
    brp_.f_capacity = 0;
    auto t = take();
    t(&brp_.fscratch, sizeof(double) * (size_t)brp_.fstride * (size_t)bt_.capacity);
    if (!t.ok()) {
      feature_err_ = "batched factorization: not enough device memory for the scratch of the deterministic program (" +
                     std::to_string((sizeof(double) * (size_t)brp_.fstride * (size_t)bt_.capacity) >> 20) + " MiB): " +
                     hipGetErrorString(t.error());
      return alloc_code(t.error());
    }
    t.commit();
    brp_.f_capacity = bt_.capacity;
    return 0;
  }
  const bool take_f = want_f || brp_.fscratch;      // (a scratch that is held grows with the batch)
  give_back(bt_.L, bt_.dinv, bt_.flag, bt_.out, brp_.fscratch);   // (a larger batch: everything again)
  bt_.capacity = bt_.nbatch = 0;
  brp_.f_capacity = 0;
  bt_.hflag.clear();
  // member strides: multiples of 32 doubles, so that every member starts 256-byte aligned
  bt_.lstride = std::max<int64_t>(32, (S_->arena + 31) / 32 * 32);
  bt_.dstride = std::max<int64_t>(32, (bt_.prog.dinv_size + 31) / 32 * 32);
  const size_t lb = sizeof(double) * (size_t)bt_.lstride * (size_t)nbatch;
  const size_t db = sizeof(double) * (size_t)bt_.dstride * (size_t)nbatch;
  auto t = take();
  t(&bt_.L, lb);
  t(&bt_.dinv, db);
  t(&bt_.flag, sizeof(int) * (size_t)nbatch);
  t(&bt_.out, sizeof(double) * (size_t)nbatch);
  const size_t fb = take_f ? sizeof(double) * (size_t)brp_.fstride * (size_t)nbatch : 0;
  if (take_f) t(&brp_.fscratch, fb);
  if (!t.ok()) {
    feature_err_ = "batched factorization: not enough device memory for " + std::to_string(nbatch) + " members (" +
                   std::to_string((lb + db + fb) >> 20) + " MiB): " + hipGetErrorString(t.error());
    return alloc_code(t.error());
  }
  t.commit();
  bt_.capacity = nbatch;
  if (take_f) brp_.f_capacity = nbatch;
  return 0;
}

// ---- bit-reproducible batch: the deterministic program and its tables, built and uploaded once per engine
int Engine::prepare_batch_repro() {
  if (brp_.ready) return 0;
  int rc = build_batch_program(*S_, brp_.prog, &feature_err_, true);
  if (rc) return rc;
  if (brp_.prog.dinv_size != bt_.prog.dinv_size) {   // (both follow from the block columns and pw = cb = 64 alone)
    feature_err_ = "batched factorization: the deterministic program lays the dinv scratch out differently";
    return -99;
  }
  TableStager tab;
  tab.add(&brp_.units, brp_.prog.units);
  tab.add(&brp_.tiles, brp_.prog.tiles);
  tab.add(&brp_.chain, brp_.prog.chain_units);
  tab.add(&brp_.relpos, brp_.prog.relpos);
  tab.add(&brp_.gtiles, brp_.prog.gather_tiles);
  tab.add(&brp_.gitems, brp_.prog.gather_items);
  auto t = take();
  t.tables(tab, &brp_.d_tab);
  if (!t.ok()) {
    feature_err_ = std::string("batched factorization: the tables of the deterministic program could not be uploaded (") +
                   hipGetErrorString(t.error()) + ")";
    return alloc_code(t.error());
  }
  t.commit();
  // member stride: a multiple of 32 doubles, as the arena's
  brp_.fstride = std::max<int64_t>(32, (brp_.prog.scratch_size + 31) / 32 * 32);
  brp_.ready = true;
  return 0;
}

BatchReproView Engine::brepro_factor_view(int nbatch) const {
  BatchReproView s;
  s.v = batch_view();
  s.v.nbatch = nbatch;
  s.scratch = brp_.fscratch;
  s.sstride = brp_.fstride;
  return s;
}

int Engine::grow_batch_buffer(double** p, size_t* have, size_t need, const char* what) {
  if (const hipError_t e = grow(p, have, need)) {
    feature_err_ = std::string("batch: not enough device memory for ") + what + " (" +
                   std::to_string((sizeof(double) * need) >> 20) + " MiB): " + hipGetErrorString(e);
    return alloc_code(e);
  }
  return 0;
}

int Engine::factor_batch(const double* val, bool on_device, int nbatch, int64_t ldval) {
  feature_err_.clear();
  if (status_) return status_;
  const int64_t nnz = S_->nnzA;
  if (!val || nbatch < 0 || ldval < nnz) return -10;
  if (opt_.nranks > 1) return -98;
  if (pending_) return -10;          // (the caller waits first)
  if (nbatch == 0) return 0;
  HIPCHK(hipSetDevice(device_), "hipSetDevice");
  int rc = prepare_batch();
  if (rc) return rc;
  const bool det = brp_on_;          // (the deterministic program: batch_repro.hip)
  if (det && (rc = prepare_batch_repro())) return rc;
  if ((rc = reserve_batch(nbatch, det))) return rc;
  bt_.nbatch = 0;                    // (no batch until this one is finished)
  bt_.z_valid = false;               // (the members' inverses belong to the factors this call replaces)
  bt_.g_state = FADJ_UNSEEDED;       // (... and so do their adjoints)
  ++bt_.generation;                 // (... and what the constraints of the batch built from them)
  bt_.hflag.clear();
  const double* vd = val;
  int64_t ld = ldval;
  if (!on_device) {
    if ((rc = grow_batch_buffer(&bt_.stage, &bt_.stage_elems, (size_t)nbatch * (size_t)nnz, "the staged values"))) return rc;
    if (nnz > 0 && (rc = copy_vectors_to_device(bt_.stage, val, ldval, nbatch, "batch val H2D", nnz)))
      return rc;
    vd = bt_.stage;
    ld = nnz;
  }
  BatchView v = batch_view();
  v.nbatch = nbatch;
  bool fits = true;
  int nl = 0;
  auto count = [&](int k) { if (k < 0) fits = false; else nl += k; };
  count(launch_batch_init(stream_, v, S_->arena, vd, ld, bt_.init_cptr, bt_.init_loc, bt_.init_src));
  if (det) {
    const BatchReproView s = brepro_factor_view(nbatch);
    // debug: a buffered entry that is gathered without having been stored by this factorization shows up as NaN
    if (batch_repro_poison() && brp_.fscratch)
      (void)hipMemsetAsync(brp_.fscratch, 0xFF, sizeof(double) * (size_t)brp_.fstride * (size_t)brp_.f_capacity, stream_);
    for (const Launch& l : brp_.prog.launches) {
      if (l.count <= 0 || !fits) continue;
      if (l.kind == L_CHAIN)
        count(launch_batch_chain(stream_, v, brp_.chain + l.first, l.count));
      else if (l.kind == L_GATHER)
        count(launch_bdet_gather(stream_, s, brp_.gtiles + l.first, l.count, brp_.gitems, brp_.relpos, d_rlist_));
      else
        count(launch_bdet_update(stream_, s, l.tile, brp_.tiles + l.first, l.count, brp_.units, d_bc_off_, d_bc_w_));
    }
  } else {
    for (const Launch& l : bt_.prog.launches) {
      if (l.count <= 0 || !fits) continue;
      if (l.kind == L_CHAIN)
        count(launch_batch_chain(stream_, v, bt_.chain + l.first, l.count));
      else
        count(launch_batch_update(stream_, v, l.tile, bt_.tiles + l.first, l.count, bt_.units, d_bc_off_, d_bc_w_,
                                  bt_.relpos, d_rlist_));
    }
  }
  HIPCHK(hipGetLastError(), "batch factor launch");
  // (the destination of the copy lives in bt_: a wait that runs into its deadline leaves it in flight)
  bt_.hflag_pending.assign((size_t)nbatch, 0);
  HIPCHK(hipMemcpyAsync(bt_.hflag_pending.data(), bt_.flag, sizeof(int) * (size_t)nbatch, hipMemcpyDeviceToHost, stream_), "batch flags D2H");
  if ((rc = sync_stream(stream_, "batch factor sync"))) return rc;
  if (!fits) {
    feature_err_ = "batched factorization: a launch of the program has more work items for ONE member than a grid holds";
    return -99;
  }
  bt_.launches = nl;
  bt_.nbatch = nbatch;
  bt_.hflag = bt_.hflag_pending;
  brp_.last_det = det;
  return batch_failed();
}

int Engine::solve_batch(double* x, bool on_device, int nrhs, int64_t ldx, int job, bool pivot_order) {
  feature_err_.clear();
  if (status_) return status_;
  const int n = S_->n;
  if (!x || nrhs < 0 || ldx < n || job < 0 || job > 2 || bt_.nbatch <= 0) return -10;
  if (nrhs == 0 || n == 0) return 0;
  if (brp_on_) {   // the reproducible batch: every sweep goes through the dispatch point of the blocked solve
    const int rc = solve_many_batch(x, on_device, nrhs, ldx, job, pivot_order);
    bt_.solve_launches = (int)bsm_info_[2];
    return rc;
  }
  HIPCHK(hipSetDevice(device_), "hipSetDevice");
  const size_t nvec = (size_t)bt_.nbatch * (size_t)nrhs;
  int rc = grow_batch_buffer(&bt_.Y, &bt_.y_elems, nvec * (size_t)n, "the solve workspace");
  if (rc) return rc;
  double* xd = x;
  int64_t ld = ldx;
  if (!on_device) {
    // the caller's n-vectors only, packed (what lies between them is neither read nor written)
    if ((rc = grow_batch_buffer(&bt_.stage, &bt_.stage_elems, nvec * (size_t)n, "the staged right-hand sides"))) return rc;
    if ((rc = copy_vectors(true, bt_.stage, x, ldx, (int64_t)nvec, "batch rhs H2D"))) return rc;
    xd = bt_.stage;
    ld = n;
  }
  const BatchView v = batch_view();
  const int* order = pivot_order ? nullptr : d_order_;
  // (a launch whose work items for one member overflow a grid: every launch has at most as many work items as
  // the pack, which is checked first -- n / 256 blocks against the block columns and strips of n rows)
  int nl = launch_batch_pack(stream_, v, false, xd, ld, nrhs, order, n, bt_.Y);
  if (nl < 0) {
    feature_err_ = "batch solve: nrhs vectors of one member are more work items than a grid holds";
    return -99;
  }
  bool fits = true;
  auto run = [&](const std::vector<SolveLaunch>& ls) {
    for (const SolveLaunch& l : ls) {
      const int k = launch_batch_solve(stream_, v, l.kind, bt_.slist, bt_.stiles, l.first, l.count, bt_.sunits, d_rlist_,
                                       bt_.Y, nrhs, n);
      if (k < 0) fits = false;
      else nl += k;
    }
  };
  if (job == 0 || job == 1) run(bt_.sprog.fwd);
  if (job == 0 || job == 2) run(bt_.sprog.bwd);
  nl += std::max(0, launch_batch_pack(stream_, v, true, xd, ld, nrhs, order, n, bt_.Y));
  bt_.solve_launches = nl;   // (read by the refined solve of the batch)
  HIPCHK(hipGetLastError(), "batch solve launch");
  // (the vectors of a failed member come back as they went: nothing on the device touched them)
  if (!on_device && (rc = copy_vectors(false, bt_.stage, x, ldx, (int64_t)nvec, "batch x D2H"))) return rc;
  if ((rc = sync_stream(stream_, "batch solve sync"))) return rc;
  if (!fits) {
    feature_err_ = "batch solve: a launch has more work items for one member than a grid holds (the vectors are not solved)";
    return -99;
  }
  return batch_failed();
}

int Engine::download_batch(int member, double* out, int64_t count) {
  feature_err_.clear();
  if (status_) return status_;
  if (!out || member < 0 || member >= bt_.nbatch || count < 0) return -10;
  HIPCHK(hipSetDevice(device_), "hipSetDevice");
  return staged_d2h(out, bt_.L + (int64_t)member * bt_.lstride, sizeof(double) * (size_t)std::min<int64_t>(count, S_->arena));
}

double* Engine::device_batch(int64_t* member_stride) {
  if (member_stride) *member_stride = bt_.nbatch > 0 ? bt_.lstride : 0;
  return bt_.nbatch > 0 ? bt_.L : nullptr;
}

int Engine::log_det_batch(double* out) {
  feature_err_.clear();
  if (status_) return status_;
  if (!out || bt_.nbatch <= 0) return -10;
  HIPCHK(hipSetDevice(device_), "hipSetDevice");
  launch_batch_log_det(stream_, batch_view(), bt_.diag, S_->n, bt_.out);
  HIPCHK(hipGetLastError(), "batch log det launch");
  HIPCHK(hipMemcpyAsync(out, bt_.out, sizeof(double) * (size_t)bt_.nbatch, hipMemcpyDeviceToHost, stream_), "batch log det D2H");
  return sync_stream(stream_, "batch log det sync");
}

// the batch's storage back to the pool (the shared tables stay: they are small and per pattern)
int Engine::release_batch() {
  feature_err_.clear();
  if (status_) return status_;
  bt_.z_valid = false;
  bt_.g_state = FADJ_UNSEEDED;
  bt_.fa_launches = 0;
  // (the batch's own storage, and what its features say of theirs)
  if (!bt_.L && !bt_.Y && !bt_.stage && !bt_.Z && !bt_.G && !bm_ready_ && !d_bmmean_ && !bsm_ready_ && !brp_.swscratch && !brf_held() && !bcn_.C && !bud_.W && !bss_.tab) { bt_.nbatch = 0; return 0; }
  HIPCHK(hipSetDevice(device_), "hipSetDevice");
  if (int rc = sync_stream(stream_, "batch release")) return rc;
  drop_factor_mult_batch();   // (the workspaces of the batched products belong to the batch)
  drop_solve_many_batch();    // (... and that of the blocked solve)
  drop_solve_repro_batch();   // (... and the scratch of its reproducible form)
  drop_refine_batch();        // (... and those of the refined solves)
  drop_constraints_batch();   // (... and the constraints of the batch, C included)
  drop_updown_batch();        // (... and the work arrays of its update / downdate)
  ss_drop(bss_);              // (... and the tables, outputs and workspaces of its sparse solves)
  give_back(bt_.L, bt_.dinv, bt_.flag, bt_.out, bt_.Y, bt_.stage, bt_.Z, bt_.G, bt_.siscratch, brp_.fscratch);
  brp_.f_capacity = 0;
  brp_.last_det = false;
  bt_.sc_users = Shared{};
  bt_.z_capacity = bt_.g_capacity = bt_.sc_capacity = 0;
  bt_.si_launches = 0;
  bt_.capacity = bt_.nbatch = 0;
  bt_.y_elems = bt_.stage_elems = 0;
  bt_.hflag.clear();
  bt_.launches = 0;
  return 0;
}

// ---- batched selected inversion ---------------------------------------------------------------------
namespace {
std::atomic<bool> g_batch_selinv_fused{true};
}
void set_batch_selinv_fused(bool on) { g_batch_selinv_fused.store(on); }
bool batch_selinv_fused() { return g_batch_selinv_fused.load(); }

BatchSelinvView Engine::batch_selinv_view() const {
  BatchSelinvView s;
  s.v = batch_view();
  s.Z = bt_.Z;
  s.scratch = bt_.siscratch;
  s.sstride = bt_.sstride;
  return s;
}

// the selected-inversion program of the batch (pw = cb = 64: the panels and dinv slots k_batch_chain
// leaves) and its tables: built and uploaded once per engine, shared by all members
int Engine::prepare_batch_selinv() {
  if (bt_.si_ready) return 0;
  if (build_selinv_program(*S_, 64, 64, bt_.siprog)) {
    feature_err_ = "batched selected inversion: the row structure of a node is not contained in its ancestors'";
    return -10;
  }
  // a step = [SYMM] [SCALE] DIAG; the fused kernel takes it when every unit has at most 64 rows below its
  // panel and at most one K slice (decided here, from the host copy of the units; the program is unchanged)
  const SelinvProgram& P = bt_.siprog;
  bt_.si_fusable.assign(P.launches.size(), 0);
  for (size_t i = 0; i < P.launches.size(); ++i) {
    const SelinvLaunch& l = P.launches[i];
    if (l.kind != SI_DIAG) continue;
    bool ok = l.count > 0;
    for (int64_t q = l.first; q < l.first + l.count && ok; ++q)
      ok = P.units[(size_t)q].nR <= kSelinvTile && P.units[(size_t)q].nsplit <= 1;
    bt_.si_fusable[i] = ok;
  }
  TableStager tab;
  tab.add(&bt_.siunits, P.units);
  tab.add(&bt_.sitiles, P.tiles);
  tab.add(&bt_.sirows, P.rows);
  tab.add(&bt_.sirelpos, P.relpos);
  auto t = take();
  t.tables(tab, &bt_.d_sitab);
  if (!t.ok()) {
    feature_err_ = std::string("batched selected inversion: the program tables could not be uploaded (") + hipGetErrorString(t.error()) + ")";
    return alloc_code(t.error());
  }
  t.commit();
  bt_.sstride = std::max<int64_t>(32, (P.scratch_size + 31) / 32 * 32);
  bt_.si_ready = true;
  return 0;
}

// One set of arenas of the batch (Z or G: *capacity x lstride doubles) and the step scratch for nbatch members.  The
// scratch is shared by the inversion and the factor adjoint (a step leaves nothing in it): each set of arenas is a
// user of it while it is held.  All or nothing: a failure keeps neither the arenas nor this set's hold of the
// scratch, and leaves the batch factor usable.  *retaken: the arenas are new memory (what they held is gone).
int Engine::reserve_batch_arenas(double** arena, int* capacity, int nbatch, const char* feature, const char* which,
                                 bool* retaken) {
  *retaken = false;
  if (nbatch <= *capacity && *arena && nbatch <= bt_.sc_capacity && bt_.siscratch) return 0;
  const size_t an = (size_t)bt_.lstride * (size_t)nbatch, sn = (size_t)bt_.sstride * (size_t)nbatch;
  const bool held = *arena != nullptr;   // (this set is a user of the scratch already)
  size_t have = (size_t)bt_.lstride * (size_t)*capacity, sc_have = (size_t)bt_.sstride * (size_t)bt_.sc_capacity;
  hipError_t e = hipSuccess;
  if (nbatch > *capacity || !*arena) {
    *retaken = true;
    e = grow(arena, &have, an);
  }
  if (e == hipSuccess) e = grow(&bt_.siscratch, &sc_have, sn);
  if (!bt_.siscratch) bt_.sc_capacity = 0;
  if (e != hipSuccess) {
    give_back(*arena);
    *capacity = 0;
    *retaken = true;
    if (held) bt_.sc_users.drop([this] { give_back(bt_.siscratch); bt_.sc_capacity = 0; });
    feature_err_ = std::string(feature) + ": not enough device memory for the " + which + " of " + std::to_string(nbatch) +
                   " members (" + std::to_string((sizeof(double) * (an + sn)) >> 20) + " MiB): " + hipGetErrorString(e);
    return -1;
  }
  if (!held) bt_.sc_users.hold();
  *capacity = nbatch;
  bt_.sc_capacity = std::max(bt_.sc_capacity, nbatch);
  return 0;
}

// Z arenas and step scratch for nbatch members; all or nothing (a failure leaves the batch factor usable)
int Engine::reserve_batch_inverse(int nbatch) {
  bool retaken;
  const int rc = reserve_batch_arenas(&bt_.Z, &bt_.z_capacity, nbatch, "batched selected inversion", "inverse arenas",
                                      &retaken);
  if (retaken) bt_.z_valid = false;
  return rc;
}

template <class Fused, class One>
int Engine::walk_batch_steps(bool fused, Fused&& fused_step, One&& one_launch) {
  const SelinvProgram& P = bt_.siprog;
  int nl = 0;
  for (size_t i = 0; i < P.launches.size();) {
    size_t j = i;
    while (P.launches[j].kind != SI_DIAG) ++j;     // (every step ends with its DIAG launch)
    const bool whole = fused && bt_.si_fusable[j];
    for (size_t k = whole ? j : i; k <= j; ++k) {
      const int made = whole ? fused_step(P.launches[k]) : one_launch(P.launches[k]);
      if (made < 0) return -1;
      nl += made;
    }
    i = j + 1;
  }
  return nl;
}

int Engine::selected_inverse_batch() {
  feature_err_.clear();
  if (status_) return status_;
  if (opt_.nranks > 1) return -98;
  if (pending_ || bt_.nbatch <= 0) return -10;
  HIPCHK(hipSetDevice(device_), "hipSetDevice");
  int rc = prepare_batch_selinv();
  if (rc) return rc;
  if ((rc = reserve_batch_inverse(bt_.nbatch))) return rc;
  bt_.z_valid = false;
  const BatchSelinvView s = batch_selinv_view();
  const int nl = walk_batch_steps(
      batch_selinv_fused(),
      [&](const SelinvLaunch& d) { return launch_batch_selinv_fused(stream_, s, bt_.siunits + d.first, d.count, bt_.sirows, bt_.sirelpos); },
      [&](const SelinvLaunch& l) { return launch_batch_selinv(stream_, s, l, bt_.siunits, bt_.sitiles, bt_.sirows, bt_.sirelpos); });
  HIPCHK(hipGetLastError(), "batch selinv launch");
  if ((rc = sync_stream(stream_, "batch selinv sync"))) return rc;
  if (nl < 0) {
    feature_err_ = "batched selected inversion: a launch of the program has more work items for ONE member than a grid holds";
    return -99;
  }
  bt_.si_launches = nl;
  bt_.z_valid = true;
  for (int fl : bt_.hflag)
    if (fl != INT_MAX) return kErrNotPosDef;
  return 0;
}

int Engine::download_inverse_batch(int member, double* out, int64_t count) {
  feature_err_.clear();
  if (status_) return status_;
  if (!bt_.z_valid || !out || member < 0 || member >= bt_.nbatch || count < 0) return -10;
  if (bt_.hflag[(size_t)member] != INT_MAX) return kErrNotPosDef;
  HIPCHK(hipSetDevice(device_), "hipSetDevice");
  return staged_d2h(out, bt_.Z + (int64_t)member * bt_.lstride, sizeof(double) * (size_t)std::min<int64_t>(count, S_->arena));
}

double* Engine::device_inverse_batch(int64_t* member_stride) {
  const bool ok = bt_.z_valid && bt_.nbatch > 0;
  if (member_stride) *member_stride = ok ? bt_.lstride : 0;
  return ok ? bt_.Z : nullptr;
}

int Engine::inverse_diag_batch(double* out, int64_t ldout) {
  feature_err_.clear();
  if (status_) return status_;
  const int n = S_->n;
  if (!bt_.z_valid || !out || ldout < n || bt_.nbatch <= 0) return -10;
  if (n == 0) return 0;
  HIPCHK(hipSetDevice(device_), "hipSetDevice");
  int rc = grow_batch_buffer(&bt_.stage, &bt_.stage_elems, (size_t)bt_.nbatch * (size_t)n, "the gathered diagonals");
  if (rc) return rc;
  if (launch_batch_selinv_diag_gather(stream_, batch_selinv_view(), bt_.diag, d_order_, n, bt_.stage, n) < 0) {
    feature_err_ = "batch inverse diagonal: one member's entries are more work items than a grid holds";
    return -99;
  }
  HIPCHK(hipGetLastError(), "batch inverse diag launch");
  if ((rc = copy_vectors(false, bt_.stage, out, ldout, bt_.nbatch, "batch inverse diag D2H"))) return rc;
  return sync_stream(stream_, "batch inverse diag sync");
}

int Engine::inverse_on_pattern_batch(double* out, int64_t ldout) {
  feature_err_.clear();
  if (status_) return status_;
  const int64_t nnz = S_->nnzA;
  if (!bt_.z_valid || !out || ldout < nnz || bt_.nbatch <= 0) return -10;
  if (nnz == 0) return 0;
  HIPCHK(hipSetDevice(device_), "hipSetDevice");
  int rc = grow_batch_buffer(&bt_.stage, &bt_.stage_elems, (size_t)bt_.nbatch * (size_t)nnz, "the gathered entries");
  if (rc) return rc;
  if (launch_batch_selinv_pattern(stream_, batch_selinv_view(), d_map_dst_, d_map_src_, nmap_, bt_.stage, nnz) < 0) {
    feature_err_ = "batch inverse on pattern: one member's entries are more work items than a grid holds";
    return -99;
  }
  HIPCHK(hipGetLastError(), "batch inverse on pattern launch");
  if ((rc = copy_vectors(false, bt_.stage, out, ldout, bt_.nbatch, "batch inverse on pattern D2H", nnz))) return rc;
  return sync_stream(stream_, "batch inverse on pattern sync");
}

int Engine::inverse_on_pattern_batch_dev(double* out_dev, int64_t ldout) {
  feature_err_.clear();
  if (status_) return status_;
  const int64_t nnz = S_->nnzA;
  if (!bt_.z_valid || !out_dev || ldout < nnz || bt_.nbatch <= 0) return -10;
  if (nnz == 0) return 0;
  HIPCHK(hipSetDevice(device_), "hipSetDevice");
  if (launch_batch_selinv_pattern(stream_, batch_selinv_view(), d_map_dst_, d_map_src_, nmap_, out_dev, ldout) < 0) {
    feature_err_ = "batch inverse on pattern: one member's entries are more work items than a grid holds";
    return -99;
  }
  HIPCHK(hipGetLastError(), "batch inverse on pattern launch");
  return sync_stream(stream_, "batch inverse on pattern sync");
}

// the inverse arenas and the step scratch back to the pool; the batch factor and its solve stay
int Engine::release_inverse_batch() {
  feature_err_.clear();
  if (status_) return status_;
  bt_.z_valid = false;
  bt_.si_launches = 0;
  if (!bt_.Z) return 0;
  HIPCHK(hipSetDevice(device_), "hipSetDevice");
  if (int rc = sync_stream(stream_, "batch inverse release")) return rc;
  give_back(bt_.Z);
  bt_.z_capacity = 0;
  bt_.sc_users.drop([this] { give_back(bt_.siscratch); bt_.sc_capacity = 0; });
  return 0;
}

// ---- reverse-mode derivative of the factors of a batch ------------------------------------------------
// (off by default: measured, DESIGN.md section 23 -- not slower than the three-launch form from 4 members on, 0.4 %
// slower with ONE member of a 128 x 128 Poisson problem)
namespace {
std::atomic<bool> g_batch_fadj_fused{false};
}
void set_batch_fadj_fused(bool on) { g_batch_fadj_fused.store(on); }
bool batch_fadj_fused() { return g_batch_fadj_fused.load(); }

// program tables, seed tables, the adjoint arenas and the step scratch for the current batch; all or nothing
// (a failure keeps nothing new and leaves the batch factor, its solves and its inversion usable)
int Engine::reserve_batch_adjoint() {
  int rc = prepare_batch_selinv();
  if (rc) return rc;
  if ((rc = prepare_fadj_tables())) return rc;
  bool retaken;
  rc = reserve_batch_arenas(&bt_.G, &bt_.g_capacity, bt_.nbatch, "batch factor adjoint", "adjoint arenas", &retaken);
  if (retaken) bt_.g_state = FADJ_UNSEEDED;
  return rc;
}

BatchSelinvView Engine::batch_adjoint_view() const {
  BatchSelinvView s = batch_selinv_view();
  s.Z = bt_.G;
  return s;
}

int Engine::fadj_seed_batch(int nvec, const double* a, const double* b, int64_t ld, double alpha, bool accumulate,
                            int order_flags, bool dev) {
  feature_err_.clear();
  if (status_) return status_;
  if (opt_.nranks > 1) return -98;
  const int n = S_->n;
  if (pending_ || !a || !b || nvec < 0 || ld < n || bt_.nbatch <= 0) return -10;
  if (accumulate && bt_.g_state != FADJ_SEEDED) {
    feature_err_ = "batch factor adjoint: accumulate = 1 needs seeded adjoint arenas of the current batch (these are " +
                   std::string(bt_.g_state == FADJ_SWEPT ? "swept" : "unseeded or stale") + ")";
    return -10;
  }
  HIPCHK(hipSetDevice(device_), "hipSetDevice");
  int rc = reserve_batch_adjoint();
  if (rc) return rc;
  const int nbatch = bt_.nbatch;
  constexpr int kGroup = 32;   // vectors per member of one staged group of the host entry point
  const int gmax = std::min(nvec, kGroup);
  if (!dev && nvec > 0 && n > 0 &&
      (rc = grow_batch_buffer(&bt_.stage, &bt_.stage_elems, 2 * (size_t)nbatch * (size_t)gmax * (size_t)n, "the staged seed vectors")))
    return rc;
  if (!accumulate) bt_.g_state = FADJ_UNSEEDED;
  const BatchSelinvView s = batch_adjoint_view();
  bool fits = true;
  auto seed = [&](int nv, const double* ad, const double* bd, int64_t ldd, bool acc) {
    if (launch_batch_fadj_seed(stream_, s, d_fatiles_, fa_ntiles_, d_facols_, d_rlist_, d_faporder_, nv, ad, bd, ldd, alpha,
                               acc, order_flags) < 0)
      fits = false;
  };
  if (dev || nvec == 0 || n == 0) {
    seed(nvec, a, b, ld, accumulate);
  } else {
    // (one stage for all groups: the copies of a group are ordered on the stream behind the launch that read the last)
    for (int q0 = 0; q0 < nvec && fits; q0 += kGroup) {
      const int nv = std::min(kGroup, nvec - q0);
      double* sa = bt_.stage;
      double* sb = bt_.stage + (int64_t)nbatch * nv * n;
      for (int m = 0; m < nbatch; ++m) {
        const int64_t src = ((int64_t)m * nvec + q0) * ld, dst = (int64_t)m * nv * n;
        if ((rc = copy_vectors_to_device(sa + dst, a + src, ld, nv, "batch seed H2D"))) return rc;
        if ((rc = copy_vectors_to_device(sb + dst, b + src, ld, nv, "batch seed H2D"))) return rc;
      }
      seed(nv, sa, sb, n, accumulate || q0 > 0);
    }
  }
  HIPCHK(hipGetLastError(), "batch factor adjoint seed launch");
  if ((rc = sync_stream(stream_, "batch factor adjoint seed sync"))) return rc;
  if (!fits) {
    feature_err_ = "batch factor adjoint: the seed has more work items for ONE member than a grid holds";
    return -99;
  }
  bt_.g_state = FADJ_SEEDED;
  return 0;
}

int Engine::fadj_upload_batch(const double* host_arenas, int64_t ldarena) {
  feature_err_.clear();
  if (status_) return status_;
  if (opt_.nranks > 1) return -98;
  if (pending_ || !host_arenas || ldarena < S_->arena || bt_.nbatch <= 0) return -10;
  HIPCHK(hipSetDevice(device_), "hipSetDevice");
  int rc = reserve_batch_adjoint();
  if (rc) return rc;
  bt_.g_state = FADJ_UNSEEDED;
  if (S_->arena > 0)
    for (int m = 0; m < bt_.nbatch; ++m)
      HIPCHK(hipMemcpyAsync(bt_.G + (int64_t)m * bt_.lstride, host_arenas + (int64_t)m * ldarena,
                            sizeof(double) * (size_t)S_->arena, hipMemcpyHostToDevice, stream_), "batch adjoint H2D");
  if ((rc = sync_stream(stream_, "batch factor adjoint upload sync"))) return rc;
  bt_.g_state = FADJ_SEEDED;
  return 0;
}

int Engine::fadj_download_batch(int member, double* out, int64_t count) {
  feature_err_.clear();
  if (status_) return status_;
  if (bt_.g_state == FADJ_UNSEEDED || !out || member < 0 || member >= bt_.nbatch || count < 0) return -10;
  HIPCHK(hipSetDevice(device_), "hipSetDevice");
  return staged_d2h(out, bt_.G + (int64_t)member * bt_.lstride, sizeof(double) * (size_t)std::min<int64_t>(count, S_->arena));
}

double* Engine::device_G_batch(int64_t* member_stride) {
  const bool ok = bt_.g_state != FADJ_UNSEEDED && bt_.nbatch > 0 && bt_.G;
  if (member_stride) *member_stride = ok ? bt_.lstride : 0;
  return ok ? bt_.G : nullptr;
}

int Engine::fadj_sweep_batch(double* gval, int64_t ldout, bool dev) {
  feature_err_.clear();
  if (status_) return status_;
  if (opt_.nranks > 1) return -98;
  const int64_t nnz = S_->nnzA;
  if (pending_ || !gval || ldout < nnz || bt_.nbatch <= 0) return -10;
  if (bt_.g_state != FADJ_SEEDED) {
    feature_err_ = "batch factor adjoint: the sweep needs freshly seeded adjoint arenas of the current batch (these are " +
                   std::string(bt_.g_state == FADJ_SWEPT ? "already swept" : "unseeded or stale") + ")";
    return -10;
  }
  HIPCHK(hipSetDevice(device_), "hipSetDevice");
  int rc = reserve_batch_adjoint();   // (seeded: everything is held; the scratch may have gone with the inversion)
  if (rc) return rc;
  if (!dev && nnz > 0 &&
      (rc = grow_batch_buffer(&bt_.stage, &bt_.stage_elems, (size_t)bt_.nbatch * (size_t)nnz, "the gathered gradients")))
    return rc;
  bt_.g_state = FADJ_UNSEEDED;   // (a sweep that fails half way leaves nothing to read)
  const BatchSelinvView s = batch_adjoint_view();
  int nl = walk_batch_steps(
      batch_fadj_fused(),
      [&](const SelinvLaunch& d) { return launch_batch_fadj_fused(stream_, s, bt_.siunits + d.first, d.count, bt_.sirows, bt_.sirelpos); },
      [&](const SelinvLaunch& l) { return launch_batch_fadj(stream_, s, l, bt_.siunits, bt_.sitiles, bt_.sirows, bt_.sirelpos); });
  if (nl >= 0 && nnz > 0) {
    const int k = launch_batch_selinv_pattern(stream_, s, d_map_dst_, d_map_src_, nmap_, dev ? gval : bt_.stage, dev ? ldout : nnz);
    nl = k < 0 ? -1 : nl + k;
  }
  const bool fits = nl >= 0;
  HIPCHK(hipGetLastError(), "batch factor adjoint launch");
  if (fits && !dev && nnz > 0 &&
      (rc = copy_vectors(false, bt_.stage, gval, ldout, bt_.nbatch, "batch factor adjoint D2H", nnz)))
    return rc;
  if ((rc = sync_stream(stream_, "batch factor adjoint sync"))) return rc;
  if (!fits) {
    feature_err_ = "batch factor adjoint: a launch of the program has more work items for ONE member than a grid holds";
    return -99;
  }
  bt_.fa_launches = nl;
  bt_.g_state = FADJ_SWEPT;
  return batch_failed();
}

// the adjoint arenas back to the pool, the step scratch too unless the inversion holds it
int Engine::release_factor_adjoint_batch() {
  feature_err_.clear();
  if (status_) return status_;
  bt_.g_state = FADJ_UNSEEDED;
  bt_.fa_launches = 0;
  if (!bt_.G) return 0;
  HIPCHK(hipSetDevice(device_), "hipSetDevice");
  if (int rc = sync_stream(stream_, "batch factor adjoint release")) return rc;
  give_back(bt_.G);
  bt_.g_capacity = 0;
  bt_.sc_users.drop([this] { give_back(bt_.siscratch); bt_.sc_capacity = 0; });
  return 0;
}

// Per-launch device time of one factorization from HIP events on the stream each launch
// runs on.  serial = true: the whole program on one stream, launch after launch (the
// kernels alone on the chip).  serial = false: the real multi-stream program; every
// launch is bracketed by two events on ITS stream, recorded behind its dependency waits, so
// the elapsed time is the launch's duration under the contention of whatever runs beside it.
int Engine::profile_launches(const double* val_host, int64_t nnz, std::vector<float>& ms, bool serial) {
  if (status_) return status_;
  if (nnz != S_->nnzA) return -10;
  if (!prog_.exchanges.empty()) return -98;   // single-GPU programs only
  z_valid_ = false;                           // (L is factored again from val)
  fadj_state_ = FADJ_UNSEEDED;
  const Symbolic& S = *S_;
  HIPCHK(hipSetDevice(device_), "hipSetDevice");
  HIPCHK(hipMemcpy(d_val_, val_host, sizeof(double) * (size_t)nnz, hipMemcpyHostToDevice), "val H2D");
  HIPCHK(hipMemsetAsync(d_L_, 0, sizeof(double) * (size_t)S.arena, stream_), "memset arena");
  *h_flag_ = INT_MAX;
  HIPCHK(hipMemcpyAsync(d_flag_, h_flag_, sizeof(int), hipMemcpyHostToDevice, stream_), "flag init");
  launch_scatter_val(stream_, d_L_, d_val_, d_map_dst_, d_map_src_, nmap_);
  size_t nl = prog_.launches.size();
  std::vector<hipEvent_t> ev(2 * nl);
  for (auto& e : ev) HIPCHK(hipEventCreate(&e), "event create");
  for (size_t i = 0; i < nl; ++i) {
    const Launch& l = prog_.launches[i];
    hipStream_t st = serial ? stream_ : streams_[l.stream];
    if (!serial)
      for (int w : l.wait)
        if (w >= 0) HIPCHK(hipStreamWaitEvent(st, dag_events_[w], 0), "stream wait");
    HIPCHK(hipEventRecord(ev[2 * i], st), "event");
    Launch bare = l;                       // waits already issued above; keep the record
    for (int& w : bare.wait) w = -1;
    bare.record = -1;
    enqueue_launch(bare, serial);
    HIPCHK(hipEventRecord(ev[2 * i + 1], st), "event");
    if (!serial && l.record >= 0) HIPCHK(hipEventRecord(dag_events_[l.record], st), "event record");
  }
  if (!serial) {
    if (prog_.final_event >= 0)
      HIPCHK(hipStreamWaitEvent(stream_, dag_events_[prog_.final_event], 0), "final wait");
  }
  HIPCHK(hipStreamSynchronize(stream_), "sync");
  ms.assign(nl, 0.f);
  for (size_t i = 0; i < nl; ++i) hipEventElapsedTime(&ms[i], ev[2 * i], ev[2 * i + 1]);
  for (auto& e : ev) hipEventDestroy(e);
  return 0;
}

// When every event of the real multi-stream program was reached, in ms after the value scatter:
// the program exactly as factor_async submits it, except that its events are timing-enabled ones
// of this call (nothing is added to the streams: the records are the program's own).  t[i] = time
// of the event launch i records (-1: the launch records none); t[nl] = the end of the program.
int Engine::timeline(const double* val_host, int64_t nnz, std::vector<float>& t) {
  if (status_) return status_;
  if (nnz != S_->nnzA) return -10;
  if (!prog_.exchanges.empty()) return -98;   // single-GPU programs only
  z_valid_ = false;                           // (L is factored again from val)
  fadj_state_ = FADJ_UNSEEDED;
  const Symbolic& S = *S_;
  HIPCHK(hipSetDevice(device_), "hipSetDevice");
  HIPCHK(hipMemcpy(d_val_, val_host, sizeof(double) * (size_t)nnz, hipMemcpyHostToDevice), "val H2D");
  HIPCHK(hipMemsetAsync(d_L_, 0, sizeof(double) * (size_t)S.arena, stream_), "memset arena");
  if (!prog_.panel_units.empty())
    HIPCHK(hipMemsetAsync(d_panel_cnt_, 0, sizeof(int) * 2 * prog_.panel_units.size(), stream_), "memset counters");
  *h_flag_ = INT_MAX;
  HIPCHK(hipMemcpyAsync(d_flag_, h_flag_, sizeof(int), hipMemcpyHostToDevice, stream_), "flag init");
  launch_scatter_val(stream_, d_L_, d_val_, d_map_dst_, d_map_src_, nmap_);
  const size_t nl = prog_.launches.size();
  std::vector<hipEvent_t> timed((size_t)prog_.nevents + 2);
  for (auto& e : timed) HIPCHK(hipEventCreate(&e), "event create");
  std::vector<hipEvent_t> keep;
  keep.swap(dag_events_);
  dag_events_.assign(timed.begin(), timed.begin() + prog_.nevents);
  hipEvent_t e0 = timed[(size_t)prog_.nevents], e1 = timed[(size_t)prog_.nevents + 1];
  int rc = 0;
  hipError_t he = hipEventRecord(e0, stream_);
  for (int s = 0; s < ST_COUNT && he == hipSuccess; ++s)
    if (streams_[s] != stream_) he = hipStreamWaitEvent(streams_[s], e0, 0);
  if (he == hipSuccess) rc = enqueue_range(0, nl);
  if (he == hipSuccess && !rc && prog_.final_event >= 0) he = hipStreamWaitEvent(stream_, dag_events_[prog_.final_event], 0);
  if (he == hipSuccess && !rc) he = hipEventRecord(e1, stream_);
  if (he == hipSuccess && !rc) he = hipStreamSynchronize(stream_);
  if (he == hipSuccess && !rc) {
    t.assign(nl + 1, -1.f);
    for (size_t i = 0; i < nl; ++i) {
      const int r = prog_.launches[i].record;
      if (r >= 0) hipEventElapsedTime(&t[i], e0, dag_events_[(size_t)r]);
    }
    hipEventElapsedTime(&t[nl], e0, e1);
  }
  dag_events_.swap(keep);
  for (auto& e : timed) hipEventDestroy(e);
  if (he != hipSuccess) return fail(kErrHip, "timeline", he);
  return rc;
}

// ---------------------------------------------------------------------------
// Submission under a deadline.  Everything spllt_factor does before it returns -- engine
// creation (stream / event borrowing, allocations, synchronous table upload), the staging of
// val, ~650 launches -- is a sequence of runtime calls that normally take microseconds but that
// nobody can interrupt once one of them sits in the driver (the one hang of round 2 that was not
// in a wait sat here).  They run on ONE helper thread per process; the caller waits for the job
// with the deadline of the other waits.  A job that does not come back marks the runtime as
// wedged: that call and every later one fail with SPLLT_ERROR_HIP and the name of the last step
// reached, instead of blocking the caller forever.  (SPLLT_HIP_TIMEOUT_S=0: no helper thread,
// the calls run inline.)
// ---------------------------------------------------------------------------
namespace {
struct SubmitJob {
  std::function<int()> fn;
  std::mutex mu;
  std::condition_variable cv;
  bool done = false;
  int rc = 0;
};
struct SubmitWorker {
  std::mutex mu;
  std::condition_variable cv;
  std::deque<std::shared_ptr<SubmitJob>> queue;
  std::atomic<bool> wedged{false};
  SubmitWorker() {
    std::thread([this] {
      for (;;) {
        std::shared_ptr<SubmitJob> job;
        {
          std::unique_lock<std::mutex> lk(mu);
          cv.wait(lk, [this] { return !queue.empty(); });
          job = queue.front();
          queue.pop_front();
        }
        const int rc = job->fn();
        {
          std::lock_guard<std::mutex> lk(job->mu);
          job->rc = rc;
          job->done = true;
        }
        job->cv.notify_all();
      }
    }).detach();
  }
};
SubmitWorker& submit_worker() {
  static SubmitWorker* w = new SubmitWorker();   // never destroyed: its thread outlives main()
  return *w;
}
}  // namespace

void mark_runtime_wedged() { g_runtime_wedged.store(true); }
bool runtime_wedged() { return g_runtime_wedged.load(); }
void run_pools_teardown_for_test() { pools_teardown(); }

int run_with_deadline(std::function<int()> fn, std::string* why) {
  // (SPLLT_HIP_SUBMIT_TIMEOUT_S: a deadline of its own -- a wait may legitimately be given a few
  // milliseconds by a caller that polls, engine creation may not)
  static const double limit_s = [] {
    const char* e = std::getenv("SPLLT_HIP_SUBMIT_TIMEOUT_S");
    if (e && *e) return std::atof(e);
    return hip_deadline_s() <= 0 ? 0.0 : 180.0;
  }();
  static const bool inline_env = std::getenv("SPLLT_HIP_SUBMIT_INLINE") != nullptr;
  if (limit_s <= 0 || inline_env) return fn();
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) return fn();     // (no device: the engine reports that itself)
  SubmitWorker& w = submit_worker();
  if (w.wedged.load()) {
    if (why) *why = std::string("the HIP runtime did not return from an earlier call (") + last_crumb() + ")";
    return kErrHip;
  }
  auto job = std::make_shared<SubmitJob>();
  job->fn = [fn, dev]() -> int {
    (void)hipSetDevice(dev);                             // the caller's device, not the helper thread's default
    return fn();
  };
  {
    std::lock_guard<std::mutex> lk(w.mu);
    w.queue.push_back(job);
  }
  w.cv.notify_one();
  std::unique_lock<std::mutex> lk(job->mu);
  if (job->cv.wait_for(lk, std::chrono::duration<double>(limit_s), [&] { return job->done; })) return job->rc;
  w.wedged.store(true);
  mark_runtime_wedged();
  if (why)
    *why = std::string("submission did not return within ") + std::to_string((int)limit_s) + " s; last step: " +
           last_crumb();
  std::fprintf(stderr, "spllt-hip: %s\n", why ? why->c_str() : "submission deadline");
  return kErrHip;
}

}  // namespace spx
