// The solve family of the Engine: the substitution program on the device (solve, solve_dev), the blocked solve
// for many right-hand sides, the reproducible solve, the factor products and samplers, their batched forms and
// the refined solves.  They share one walk over the program's launches, one table view, one order table and one
// staging helper; the vector entry points share one preamble (enter), the blocked features one walk over the
// blocks of a call (walk_blocks, around each feature's enqueue_*_block) and one width fallback for their
// storage (take_block_buffers).  The block rules themselves are in engine_detail.hpp.
#include <atomic>
#include <chrono>
#include <climits>
#include <cstdlib>
#include <limits>

#include "engine.hpp"
#include "engine_detail.hpp"
#include "refine.hpp"
#include "refine_driver.hpp"

namespace spx {

int Engine::prepare_solve() {
  if (solve_ready_) return 0;
  const Symbolic& S = *S_;
  build_solve_program(S, prog_.pw, prog_.cb, sprog_, opt_.nranks > 1 ? owner_.data() : nullptr, opt_.rank);
  if (!loc_off_.empty())
    for (size_t b = 0; b < sprog_.units.size(); ++b)   // (units of block columns not held here are never launched)
      if (loc_off_[b] >= 0) sprog_.units[b].off = loc_off_[b];
  {
    TableStager tab;
    tab.add(&d_sunits_, sprog_.units);
    tab.add(&d_slist_, sprog_.diag_list);
    tab.add(&d_stiles_, sprog_.tiles);
    HIPCHK(tab.commit(&d_solve_tables_, [this](void** q, size_t b) { return dalloc(q, b); }), "upload solve tables");
  }
  HIPCHK(dalloc((void**)&d_y_, sizeof(double) * 4 * (size_t)std::max(1, S.n)), "hipMalloc(y)");
  {
    const char* e = std::getenv("SPLLT_SOLVE_DIAG4");
    solve_four_ = prog_.pw == 64 && prog_.cb == 64 && !(e && std::atoi(e) == 0);
  }
  // per launch, once (solve_launch_info), and per block column where it sits in the launches (sv_slots_)
  auto info = [&](const std::vector<SolveLaunch>& ls, std::vector<SolveLaunchInfo>& out) {
    out.assign(ls.size(), SolveLaunchInfo{false, nullptr});
    for (size_t i = 0; i < ls.size(); ++i) out[i] = solve_launch_info(ls[i], sprog_.diag_list.data(), sprog_.tiles.data());
  };
  info(sprog_.fwd, sv_fwd_);
  info(sprog_.bwd, sv_bwd_);
  sv_slots_ = build_solve_slots(sprog_);
  solve_ready_ = true;
  return 0;
}

// block columns of at most four 64-wide panels take the diagonal kernel that reads L in one round trip; a launch
// on ONE block column (every step of the upper levels) passes its descriptor by value.  list / tiles: the
// arrays l.first indexes.
SolveLaunchInfo Engine::solve_launch_info(const SolveLaunch& l, const int* list, const UpdTile* tiles) const {
  SolveLaunchInfo out{false, nullptr};
  const bool diag = l.kind == SV_DIAG_FWD || l.kind == SV_DIAG_BWD;
  bool four = solve_four_ && diag;
  for (int64_t q = l.first; four && q < l.first + l.count; ++q) four = sprog_.units[(size_t)list[q]].w <= 256;
  out.four = four;
  if (l.count <= 0) return out;
  if (diag) {
    if (l.count == 1) out.one = &sprog_.units[(size_t)list[l.first]];
  } else {
    const UpdTile* tl = tiles + l.first;
    bool same = true;
    for (int64_t q = 0; same && q < l.count; ++q) same = tl[q].unit == tl[0].unit && tl[q].ti == (short)q;
    if (same && l.count < 32768) out.one = &sprog_.units[(size_t)tl[0].unit];
  }
  return out;
}

// the launches of the substitution program that `job` (0 both sweeps, 1 forward, 2 backward) and `phase` (-1
// everything; 0 / 1 / 2: the phases of a partitioned solve, schedule.hpp) ask for, in program order
template <class F>
void Engine::for_each_solve_launch(int job, int phase, F&& f) const {
  auto run = [&](const std::vector<SolveLaunch>& ls, const std::vector<SolveLaunchInfo>& li, size_t a, size_t b) {
    for (size_t i = a; i < b; ++i) f(ls[i], li[i]);
  };
  const bool do_fwd = job == 0 || job == 1, do_bwd = job == 0 || job == 2;
  if (do_fwd && (phase == -1 || phase == 0)) run(sprog_.fwd, sv_fwd_, 0, sprog_.fwd_nsub);
  if (do_fwd && (phase == -1 || phase == 1)) run(sprog_.fwd, sv_fwd_, sprog_.fwd_nsub, sprog_.fwd.size());
  if (do_bwd && (phase == -1 || phase == 1)) run(sprog_.bwd, sv_bwd_, 0, sprog_.bwd_ntop);
  if (do_bwd && (phase == -1 || phase == 2)) run(sprog_.bwd, sv_bwd_, sprog_.bwd_ntop, sprog_.bwd.size());
}

bool Engine::enter(bool args_ok, bool empty, int* rc) {
  feature_err_.clear();
  // (-98: a rank of a partition holds a part of L only; pending_: the caller waits first)
  *rc = status_ ? status_ : !args_ok ? -10 : opt_.nranks > 1 ? -98 : pending_ ? -10 : 0;
  if (*rc || empty) return false;
  const hipError_t e = hipSetDevice(device_);
  if (e != hipSuccess) *rc = fail(kErrHip, "hipSetDevice", e);
  return e == hipSuccess;
}

bool Engine::enter_release(bool held, const char* what, int* rc) {
  feature_err_.clear();
  *rc = status_;
  if (*rc || !held) return false;
  const hipError_t e = hipSetDevice(device_);
  *rc = e != hipSuccess ? fail(kErrHip, "hipSetDevice", e) : sync_stream(stream_, what);
  return *rc == 0;
}

template <class Enq>
int Engine::walk_blocks(const BlockWalk& w, Enq&& enqueue, BlockTally* tally) {
  const int n = S_->n;
  const std::string label(w.label), launch = label + " launch", sync = label + " sync";
  // the block at `done` of every member between the caller's host array and the staging buffer (a failed member's
  // vectors make the round trip unchanged: nothing on the device touches them)
  auto stage = [&](bool up, int done, int nv) -> int {
    const std::string what = label + (up ? " H2D" : " D2H");
    for (int b = 0; b < w.members; ++b)
      if (int rc = copy_vectors(up, w.stage + (int64_t)b * nv * n, w.x + ((int64_t)b * w.total + done) * w.ldx, w.ldx, nv,
                                what.c_str()))
        return rc;
    return 0;
  };
  BlockTally t;
  const int rc = for_each_block(w.total, w.cap, [&](int done, int nv, int rb) -> int {
    int r = 0;
    if (!w.on_device && w.upload && (r = stage(true, done, nv))) return r;
    const int k = w.on_device ? enqueue(done, w.x + (int64_t)done * w.ldx, (int64_t)w.total * w.ldx, w.ldx, nv, rb, w.pivot_order)
                              : enqueue(done, w.stage, (int64_t)nv * n, (int64_t)n, nv, rb, false);
    ++t.blocks;
    t.launches += std::max(k, 0);
    if (!w.on_device) {
      HIPCHK(hipGetLastError(), launch.c_str());
      if (k >= 0 && (r = stage(false, done, nv))) return r;
      if ((r = sync_stream(stream_, sync.c_str()))) return r;
    }
    return std::min(k, 0);
  });
  if (w.on_device) {
    HIPCHK(hipGetLastError(), launch.c_str());
    if (int r = sync_stream(stream_, sync.c_str())) return r;
  }
  if (tally) *tally = t;
  return rc;
}

hipError_t Engine::take_block_buffers(std::initializer_list<BlockBuffer> bufs, int* rb, size_t* want) {
  for (*rb = 32;; *rb /= 2) {
    auto t = take();
    for (const BlockBuffer& b : bufs) t.block(b.p, b.bytes * (size_t)*rb);
    *want = t.bytes();
    t.commit();
    if (t.ok() || *rb == 16 || alloc_code(t.error()) != -1) return t.error();   // (out of memory: once more with half of it)
  }
}

// Substitution on device vectors in pivot order (y[q * n + p], q < nrhs), in place.
// phase -1: everything that `job` asks for; 0/1/2: the three phases of a
// partitioned solve (schedule.hpp, SolveProgram).
int Engine::solve_dev(double* y_dev, int nrhs, int job, int phase) {
  if (status_) return status_;
  if (job < 0 || job > 2 || phase < -1 || phase > 2 || nrhs < 0 || !y_dev) return -10;
  if (repro_on_ && phase == -1 && opt_.nranks == 1) return solve_repro_dev(y_dev, nrhs, (int64_t)S_->n, job, true);
  HIPCHK(hipSetDevice(device_), "hipSetDevice");
  int rc = prepare_solve();
  if (rc) return rc;
  const int n = S_->n;
  const SolveTablesView tv = solve_tables();
  for_each_group4(nrhs, [&](int done, int cur) {
    double* y = y_dev + (int64_t)done * n;
    for_each_solve_launch(job, phase, [&](const SolveLaunch& l, const SolveLaunchInfo& li) {
      launch_solve(stream_, tv, l, li, y, cur, (int64_t)n);
    });
    return 0;
  });
  HIPCHK(hipGetLastError(), "solve launch");
  return sync_stream(stream_, "solve sync");
}

int Engine::solve(double* x_host, int nrhs, int job) {
  if (status_) return status_;
  if (job < 0 || job > 2) return -10;
  const Symbolic& S = *S_;
  if (repro_on_ && opt_.nranks == 1 && nrhs >= 0 && x_host) return solve_repro(x_host, nrhs, (int64_t)S.n, job);
  HIPCHK(hipSetDevice(device_), "hipSetDevice");
  int rc = prepare_solve();
  if (rc) return rc;
  const int n = S.n;
  // up to four right-hand sides per sweep: every entry of L is read once for all of them
  std::vector<double> yh((size_t)n * 4);
  return for_each_group4(nrhs, [&](int done, int cur) -> int {
    for (int q = 0; q < cur; ++q) {
      const double* xr = x_host + (int64_t)(done + q) * n;
      double* yq = yh.data() + (size_t)q * n;
      for (int i = 0; i < n; ++i) yq[S.order[i]] = xr[i];
    }
    HIPCHK(hipMemcpyAsync(d_y_, yh.data(), sizeof(double) * (size_t)n * cur, hipMemcpyHostToDevice, stream_), "rhs H2D");
    if (comm_ && opt_.nranks > 1) {
      // partitioned solve inside the library (every rank passes the same right-hand sides and gets
      // the same solution): forward substitution on the own subtrees, all-reduce of the vector,
      // the top tree on every rank, backward substitution on the own subtrees, all-reduce
      if (job != 0) return -98;
      Rccl& R = rccl();
      launch_mask(stream_, d_y_, d_owned_, n, cur, (int64_t)n);
      if ((rc = solve_dev(d_y_, cur, 0, 0))) return rc;
      NCCLCHK(R.all_reduce(d_y_, d_y_, (size_t)n * cur, kNcclDouble, kNcclSum, comm_, stream_), "ncclAllReduce(rhs)");
      if ((rc = solve_dev(d_y_, cur, 0, 1))) return rc;
      if ((rc = solve_dev(d_y_, cur, 0, 2))) return rc;
      launch_mask(stream_, d_y_, d_owned_, n, cur, (int64_t)n);
      NCCLCHK(R.all_reduce(d_y_, d_y_, (size_t)n * cur, kNcclDouble, kNcclSum, comm_, stream_), "ncclAllReduce(x)");
      if ((rc = sync_stream(stream_, "solve sync"))) return rc;
    } else {
      rc = solve_dev(d_y_, cur, job, -1);
      if (rc) return rc;
    }
    HIPCHK(hipMemcpy(yh.data(), d_y_, sizeof(double) * (size_t)n * cur, hipMemcpyDeviceToHost), "x D2H");
    for (int q = 0; q < cur; ++q) {
      double* xr = x_host + (int64_t)(done + q) * n;
      const double* yq = yh.data() + (size_t)q * n;
      for (int i = 0; i < n; ++i) xr[i] = yq[S.order[i]];
    }
    return 0;
  });
}

// ---- blocked solve for many right-hand sides ---------------------------------------------------
int Engine::prepare_solve_many(bool host_stage) {
  int rc = prepare_solve();
  if (rc) return rc;
  const Symbolic& S = *S_;
  const size_t wb = sizeof(double) * 32 * (size_t)std::max(1, S.n);
  // (a failure here leaves the factor and the existing solve usable: the engine's status is not touched)
  auto t = take();
  if (!d_smW_) t(&d_smW_, wb);
  if (t.ok()) t.check(ensure_order());
  if (host_stage && !d_smstage_) t(&d_smstage_, wb);
  if (!t.ok()) {
    feature_err_ = "solve_many: not enough device memory for the workspace of 32 right-hand sides (" +
                   std::to_string(wb >> 20) + " MiB): " + hipGetErrorString(t.error());
    return alloc_code(t.error());
  }
  t.commit();
  return 0;
}

// one block of nv <= rb vectors: pack, the sweeps `job` asks for, unpack (enqueue only)
void Engine::enqueue_solve_many_block(double* x_dev, int64_t ldx, int nv, int rb, int job, bool pivot_order) {
  const int n = S_->n;
  const int* order = pivot_order ? nullptr : d_order_;
  const SolveTablesView tv = solve_tables();
  launch_solve_many_pack(stream_, x_dev, ldx, order, n, nv, rb, d_smW_);
  for_each_solve_launch(job, -1, [&](const SolveLaunch& l, const SolveLaunchInfo& li) {
    launch_solve_many(stream_, tv, l, li, d_smW_, rb);
  });
  launch_solve_many_unpack(stream_, x_dev, ldx, order, n, nv, rb, d_smW_);
}

// the blocked solve on device vectors, or on host vectors through the staging block (a block goes up in the caller's
// layout, its n-vectors only: the permutation happens on the device)
int Engine::run_solve_many(double* x, bool on_device, int nrhs, int64_t ldx, int job, bool pivot_order) {
  int rc;
  if (!enter(job >= 0 && job <= 2 && nrhs >= 0 && x && ldx >= S_->n, nrhs == 0 || S_->n == 0, &rc)) return rc;
  if ((rc = prepare_solve_many(!on_device))) return rc;
  return walk_blocks({"solve_many", x, on_device, nrhs, ldx, 1, d_smstage_, 32, pivot_order},
                     [&](int, double* xd, int64_t, int64_t ld, int nv, int rb, bool po) {
                       enqueue_solve_many_block(xd, ld, nv, rb, job, po);
                       return 0;
                     });
}

int Engine::solve_many_dev(double* x_dev, int nrhs, int64_t ldx, int job, bool pivot_order) {
  return run_solve_many(x_dev, true, nrhs, ldx, job, pivot_order);
}

int Engine::solve_many(double* x_host, int nrhs, int64_t ldx, int job) {
  return run_solve_many(x_host, false, nrhs, ldx, job, false);
}

// ---- sparse right-hand sides and selected outputs, of the handle and of the members of a batch -------
// The sequence of a call is ss_driver.hpp's; here are what it runs on: the planning and the upload of a group, the
// storage, and the two backends (solve_sparse.hip, batch_solve_sparse.hip).
static std::atomic<bool> g_ss_poison{false};
void set_solve_sparse_poison(bool on) { g_ss_poison.store(on); }
static std::atomic<bool> g_bss_poison{false};
void set_solve_sparse_batch_poison(bool on) { g_bss_poison.store(on); }

// the launches of one sweep of P that hold a block column of `set`, compacted into g (ss_filter.hpp)
void Engine::ss_filter(const SolveProgram& P, const SolveSlots& sl, bool bwd, const std::vector<int>& set, SsGroup& g) {
  filter_solve_program(P, sl.slot, bwd, set, bwd ? g.bwd : g.fwd, g.list, g.tiles, g.info);
}

// plan, filter and stage one group (host only) on program P with its slots.  zero_ranges: the rows to clear when
// they are not the group's own touched rows (gram: those of the whole call)
void Engine::ss_plan_group(const SolveProgram& prog, const SolveSlots& sl, bool launch_info, SsGroup& g, const int* bptr,
                           const int* brow, int nsel, const int* sel, int job, const std::vector<int>* zero_ranges) {
  const Symbolic& S = *S_;
  SolveSparsePlan P;
  build_solve_sparse_plan(S, g.c0, g.c0 + g.nv, bptr, brow, nsel, sel, job, P);
  ss_filter(prog, sl, false, P.fwd, g);
  if (!P.bwd.empty() && P.bwd.size() == prog.units.size()) {
    // every block column: the backward sweep is the program's own, on the tables that are resident already
    g.bwd_full = true;
    g.info[1] += (int64_t)prog.units.size();
    g.info[3] += sl.entries;
    g.info[5] += sl.bwd_wgs;
  } else {
    ss_filter(prog, sl, true, P.bwd, g);
  }
  if (launch_info) {
    g.fwd_i.resize(g.fwd.size());
    g.bwd_i.resize(g.bwd.size());
    for (size_t i = 0; i < g.fwd.size(); ++i) g.fwd_i[i] = solve_launch_info(g.fwd[i], g.list.data(), g.tiles.data());
    for (size_t i = 0; i < g.bwd.size(); ++i) g.bwd_i[i] = solve_launch_info(g.bwd[i], g.list.data(), g.tiles.data());
  }
  const std::vector<int>& rg = zero_ranges ? *zero_ranges : P.range;
  for (size_t r = 0; r + 1 < rg.size(); r += 2)
    for (int o = 0; o < rg[r + 1]; o += kSsChunkRows) {
      g.chunks.push_back(rg[r] + o);
      g.chunks.push_back(std::min(kSsChunkRows, rg[r + 1] - o));
    }
  // the entries of B in touched rows (job 2: what lies outside the closure of the wanted rows cannot reach them)
  auto touched = [&](int p) {
    size_t lo = 0, hi = P.range.size() / 2;
    while (lo < hi) {
      const size_t mid = (lo + hi) / 2;
      if (P.range[2 * mid] + P.range[2 * mid + 1] <= p) lo = mid + 1; else hi = mid;
    }
    return lo < P.range.size() / 2 && P.range[2 * lo] <= p;
  };
  for (int q = 0; q < g.nv; ++q)
    for (int e = bptr[g.c0 + q] - 1; e < bptr[g.c0 + q + 1] - 1; ++e) {
      const int p = S.order[(size_t)brow[e] - 1];
      if (job == 2 && !touched(p)) continue;
      g.pos.push_back((int64_t)p * g.rb + q);
      g.ent.push_back(e);   // (the upload packs the values of these entries)
    }
  if (sel && nsel >= 0)
    for (int t = 0; t < nsel; ++t) g.selpos.push_back(S.order[(size_t)sel[t] - 1]);
}

// the size ss_upload lays a group out in: 256-byte aligned slots of at least 8 bytes (TableStager), the values last
size_t Engine::ss_table_bytes(const SsGroup& g, size_t copies) {
  size_t bytes = 0;
  for (size_t b : {g.list.size() * sizeof(int), g.tiles.size() * sizeof(UpdTile), g.chunks.size() * sizeof(int),
                   g.selpos.size() * sizeof(int), g.pos.size() * sizeof(int64_t), copies * g.ent.size() * sizeof(double)})
    bytes = (bytes + 255) / 256 * 256 + std::max<size_t>(b, 8);
  return bytes;
}

int Engine::ss_upload(const SsState& s, const SsGroup& g, const double* bval, int64_t ldb, size_t copies, SsTables& t) {
  const size_t count = g.ent.size();
  std::vector<double> vals(copies * count);
  for (size_t b = 0; b < copies; ++b)
    for (size_t i = 0; i < count; ++i) vals[b * count + i] = bval[(int64_t)b * ldb + g.ent[i]];
  TableStager tab;
  tab.add(&t.list, g.list);
  tab.add(&t.tiles, g.tiles);
  tab.add(&t.chunks, g.chunks);
  tab.add(&t.selpos, g.selpos);
  tab.add(&t.pos, g.pos);
  tab.add(&t.val, vals);
  char* blob = nullptr;
  HIPCHK(tab.commit(&blob, [&s](void** q, size_t b) {
    *q = s.tab;
    return b <= s.tab_cap ? hipSuccess : hipErrorOutOfMemory;
  }), "upload the tables of a sparse solve");
  return 0;
}

// 0, or -99 when a substitution program does not have the shape the filter relies on (build_solve_slots)
static const char* const kSsShape = ": the substitution program holds a block column in more than one diagonal launch or "
                                    "with strips that are not one run of one launch; filtering it is not implemented";
int Engine::ss_filterable() {
  if (sv_slots_.ok) return 0;
  feature_err_ = std::string("solve_sparse") + kSsShape;
  return -99;
}

void Engine::ss_drop(SsState& s) {
  give_back(s.tab, s.out, s.gramW);
  s.tab_cap = s.out_cap = s.gram_cap = 0;
}

int Engine::ss_release(SsState& s, const char* what) {
  int rc;
  if (!enter_release(s.tab || s.out || s.gramW, what, &rc)) return rc;
  ss_drop(s);
  return 0;
}

int Engine::release_solve_sparse() { return ss_release(ss_, "solve_sparse release"); }
int Engine::release_solve_sparse_batch() { return ss_release(bss_, "solve_sparse_batch release"); }

// the slots of the batch's own program (once), the workspace of the blocked batch solve and the order table
int Engine::bss_enter() {
  if (!bss_.slots_ready) {
    bss_.slots = build_solve_slots(bt_.sprog);
    bss_.slots_ready = true;
  }
  if (!bss_.slots.ok) {
    feature_err_ = std::string("solve_sparse_batch") + kSsShape;
    return -99;
  }
  return prepare_solve_many_batch();
}

// the three buffers of a call, kept while each is large enough; else all three again in ONE transaction (a
// failure leaves none of them)
int Engine::bss_take(size_t tab_bytes, size_t out_elems, size_t gram_elems, const char* what) {
  if (bss_.tab && bss_.tab_cap >= tab_bytes && bss_.out_cap >= out_elems && bss_.gram_cap >= gram_elems) return 0;
  tab_bytes = std::max(tab_bytes, bss_.tab_cap);
  out_elems = std::max(out_elems, bss_.out_cap);
  gram_elems = std::max(gram_elems, bss_.gram_cap);
  ss_drop(bss_);
  auto t = take();
  t(&bss_.tab, std::max<size_t>(tab_bytes, 8));
  if (out_elems) t(&bss_.out, sizeof(double) * out_elems);
  if (gram_elems) t(&bss_.gramW, sizeof(double) * gram_elems);
  if (!t.ok()) {
    feature_err_ = std::string(what) + ": not enough device memory for the tables, the outputs and the workspaces of " +
                   std::to_string(bt_.nbatch) + " members (" + std::to_string(t.bytes() >> 20) + " MiB): " +
                   hipGetErrorString(t.error());
    return alloc_code(t.error());
  }
  t.commit();
  bss_.tab_cap = tab_bytes;
  bss_.out_cap = out_elems;
  bss_.gram_cap = gram_elems;
  return 0;
}

// What the two backends of the sequence share: the columns of the call, planning and upload of a group on the
// backend's program, the copies to a host caller (member b's column q of a group: on the device at
// x + (b k + c0 + q) ldx, else packed in the output buffer), the checks.
struct Engine::SsBackend {
  using Group = SsGroup;
  Engine& e;
  const std::string what;
  const SolveProgram& prog;
  const SolveSlots& slots;
  const bool launch_info;   // the kernels take a SolveLaunchInfo per filtered launch
  SsState& st;
  double* const W0;
  const int cap, members;
  const int *bptr, *brow;
  const double* bval;
  const int64_t ldb;        // between the members' sets of values; 0: one set
  const int nsel;
  const int* sel;
  const int n = e.S_->n;
  const hipStream_t s = e.stream_;
  const size_t copies = ldb ? (size_t)members : 1;
  SolveSparsePlan rows;     // gram: of the whole call
  SsTables t{};             // of the group uploaded last

  int fail(int code, const char* w, hipError_t err) { return e.fail(code, w, err); }
  void plan_rows(int k) {
    static const int none = 0;
    build_solve_sparse_plan(*e.S_, 0, k, bptr, brow, 0, &none, 1, rows);
  }
  SsGroup plan(int c0, int nv, int rb, int job, bool gram) {
    static const int none = 0;
    SsGroup g;
    g.c0 = c0, g.nv = nv, g.rb = rb;
    if (gram) e.ss_plan_group(prog, slots, launch_info, g, bptr, brow, 0, &none, 1, &rows.range);
    else e.ss_plan_group(prog, slots, launch_info, g, bptr, brow, nsel, sel, job, nullptr);
    g.bytes = ss_table_bytes(g, copies);
    return g;
  }
  int upload(const SsGroup& g) { return e.ss_upload(st, g, bval, ldb, copies, t); }
  int launch_check() {
    HIPCHK(hipGetLastError(), (what + " launch").c_str());
    return 0;
  }
  int sync() { return e.sync_stream(s, (what + " sync").c_str()); }
  int copy_out(const SsGroup& g, const SsSolveCall& c) {
    for (int b = 0; b < members; ++b)
      if (int rc = e.copy_vectors(false, st.out + (int64_t)b * g.nv * c.nout, c.x + ((int64_t)b * c.k + g.c0) * c.ldx, c.ldx,
                                  g.nv, "x D2H", c.nout))
        return rc;
    return 0;
  }
  int copy_gram(double* G, double* gout, int64_t ldg, int k) {
    return e.copy_vectors(false, G, gout, ldg, (int64_t)members * k, "G D2H", k);
  }
  int overflow() {
    e.feature_err_ = what + ": a launch has more work items for one member than a grid holds (the outputs are not all "
                            "written)";
    return -99;
  }
};

// The single handle: its own program and launch infos, the workspace of solve_many, three buffers that grow.
struct Engine::SsHandleBackend : Engine::SsBackend {
  SsHandleBackend(Engine& e, const char* what, const int* bptr, const int* brow, const double* bval, int nsel,
                  const int* sel)
      : SsBackend{e, what, e.sprog_, e.sv_slots_, true, e.ss_, e.d_smW_, 32, 1, bptr, brow, bval, 0, nsel, sel} {}

  // (the capacities are in elements: bytes of the tables, doubles of the other two)
  int take(size_t tab_bytes, size_t out_elems, size_t gram_elems) {
    hipError_t err = e.grow(&st.tab, &st.tab_cap, tab_bytes);
    if (err == hipSuccess && out_elems) err = e.grow(&st.out, &st.out_cap, out_elems);
    if (err == hipSuccess && gram_elems) err = e.grow(&st.gramW, &st.gram_cap, gram_elems);
    if (err != hipSuccess) {
      e.ss_drop(st);
      e.feature_err_ = what + ": not enough device memory (" +
                       std::to_string((tab_bytes + sizeof(double) * (out_elems + gram_elems)) >> 20) + " MiB): " +
                       hipGetErrorString(err);
      return alloc_code(err);
    }
    for (int64_t& v : st.info) v = 0;
    return 0;
  }
  // zero the touched rows of W, scatter the group's entries, the filtered sweeps `job` asks for (enqueue only)
  int enqueue(const SsGroup& g, int job, double* W) {
    if (g_ss_poison.load()) (void)hipMemsetAsync(W, 0xFF, sizeof(double) * (size_t)g.rb * (size_t)n, s);
    launch_ss_zero(s, t.chunks, (int)(g.chunks.size() / 2), g.rb, W);
    launch_ss_scatter(s, t.pos, t.val, (int64_t)g.pos.size(), W);
    SolveTablesView tv = e.solve_tables();
    tv.list = t.list;
    tv.tiles = t.tiles;
    if (job != 2)
      for (size_t i = 0; i < g.fwd.size(); ++i) launch_solve_many(s, tv, g.fwd[i], g.fwd_i[i], W, g.rb);
    const std::vector<SolveLaunch>& bwd = g.bwd_full ? prog.bwd : g.bwd;
    const std::vector<SolveLaunchInfo>& bwd_i = g.bwd_full ? e.sv_bwd_ : g.bwd_i;
    const SolveTablesView tb = g.bwd_full ? e.solve_tables() : tv;
    if (job != 1)
      for (size_t i = 0; i < bwd.size(); ++i) launch_solve_many(s, tb, bwd[i], bwd_i[i], W, g.rb);
    return (g.chunks.empty() ? 0 : 1) + (g.pos.empty() ? 0 : 1) + (int)(job != 2 ? g.fwd.size() : 0) +
           (int)(job != 1 ? bwd.size() : 0);
  }
  int gather(const SsGroup& g, const SsSolveCall& c) {
    double* xg = c.dev ? c.x + (int64_t)g.c0 * c.ldx : st.out;
    const int64_t ldo = c.dev ? c.ldx : c.nout;
    if (c.all) launch_solve_many_unpack(s, xg, ldo, e.d_order_, n, g.nv, g.rb, W0);
    else launch_ss_gather(s, xg, ldo, t.selpos, nsel, g.nv, g.rb, W0);
    return 1;
  }
  int pair(const SsGroup& gi, const SsGroup& gj, double* WI, double* WJ, int nchunk, double* part, bool diag, double* Gij,
           double* Gji, int64_t ld) {
    launch_ss_gram(s, t.chunks, nchunk, WI, gi.rb, WJ, gj.rb, part);
    launch_ss_gram_reduce(s, part, nchunk, gi.nv, gj.nv, diag, Gij, Gji, ld);
    return nchunk ? 2 : 1;
  }
  // (a failed call leaves the sums of the groups it completed)
  void progress(const int64_t info[6]) { std::copy(info, info + 6, st.info); }
  int finish(const int64_t*) { return 0; }
};

// The members of a batch: the batch's program on the workspaces of its blocked solve, every launch carrying all
// members and able to overflow a grid, one transaction for the three buffers.
struct Engine::SsBatchBackend : Engine::SsBackend {
  const int k;
  const BatchView v = e.batch_view();
  const BssView bs{e.bt_.flag, members};

  SsBatchBackend(Engine& e, const char* what, int k, const int* bptr, const int* brow, const double* bval, int64_t ldb,
                 int nsel, const int* sel)
      : SsBackend{e,    what, e.bt_.sprog, e.bss_.slots, false, e.bss_, e.d_bsmW_, e.bsm_rb_, e.bt_.nbatch,
                  bptr, brow, bval,        ldb,          nsel,  sel},
        k(k) {}

  // (one aligned slot more than the tables take, as this path has requested from its first version: the ledger
  // of a call is part of what the tests record)
  int take(size_t tab_bytes, size_t out_elems, size_t gram_elems) {
    return e.bss_take(tab_bytes + 256, out_elems, gram_elems, what.c_str());
  }
  // poison (debug), zero, scatter and the filtered sweeps `job` asks for on the workspaces W (enqueue only);
  // launches made, -1: a launch overflows a grid
  int enqueue(const SsGroup& g, int job, double* W) {
    const int64_t ws = (int64_t)g.rb * n, ldv = ldb ? (int64_t)g.pos.size() : 0;
    if (g_bss_poison.load()) {
      const size_t elems =
          W == W0 ? (size_t)e.bsm_capacity_ * (size_t)e.bsm_rb_ * (size_t)n : (size_t)members * 32 * (size_t)n;
      (void)hipMemsetAsync(W, 0xFF, sizeof(double) * elems, s);
    }
    int nl = 0;
    bool fits = true;
    auto count = [&](int made) { if (made < 0) fits = false; else nl += made; };
    count(launch_bss_zero(s, bs, t.chunks, (int)(g.chunks.size() / 2), g.rb, W, ws));
    count(launch_bss_scatter(s, bs, t.pos, t.val, ldv, (int64_t)g.pos.size(), W, ws));
    if (job != 2)
      for (const SolveLaunch& l : g.fwd)
        count(launch_batch_solve_many(s, v, l, t.list, t.tiles, e.bt_.sunits, e.d_rlist_, W, g.rb, n));
    if (job != 1) {
      // (all entries wanted: the program's own backward launches on the resident tables of the batch)
      const std::vector<SolveLaunch>& bwd = g.bwd_full ? prog.bwd : g.bwd;
      for (const SolveLaunch& l : bwd)
        count(launch_batch_solve_many(s, v, l, g.bwd_full ? e.bt_.slist : t.list, g.bwd_full ? e.bt_.stiles : t.tiles,
                                      e.bt_.sunits, e.d_rlist_, W, g.rb, n));
    }
    return fits ? nl : -1;
  }
  // (all entries: the order table is the list of wanted positions)
  int gather(const SsGroup& g, const SsSolveCall& c) {
    double* xg = c.dev ? c.x + (int64_t)g.c0 * c.ldx : st.out;
    const int64_t ldo = c.dev ? c.ldx : c.nout, xs = c.dev ? (int64_t)k * c.ldx : (int64_t)g.nv * c.nout;
    return launch_bss_gather(s, bs, xg, xs, ldo, c.all ? e.d_order_ : t.selpos, c.nout, g.nv, g.rb, W0, (int64_t)g.rb * n);
  }
  int pair(const SsGroup& gi, const SsGroup& gj, double* WI, double* WJ, int nchunk, double* part, bool diag, double* Gij,
           double* Gji, int64_t ld) {
    const int a = launch_bss_gram(s, bs, t.chunks, nchunk, WI, (int64_t)gi.rb * n, gi.rb, WJ, (int64_t)gj.rb * n, gj.rb, part);
    if (a < 0) return -1;
    const int b = launch_bss_gram_reduce(s, bs, part, nchunk, gi.nv, gj.nv, diag, Gij, Gji, (int64_t)k * ld, ld);
    return b < 0 ? -1 : a + b;
  }
  void progress(const int64_t*) {}   // (a failed call leaves zeros)
  int finish(const int64_t info[6]) {
    std::copy(info, info + 6, st.info);
    st.info[5] *= members;
    for (int fl : e.bt_.hflag) ++st.info[fl == INT_MAX ? 6 : 7];
    return e.batch_failed();
  }
};

int Engine::solve_sparse(int k, const int* bptr, const int* brow, const double* bval, int nsel, const int* sel,
                         double* x, int64_t ldx, int job, bool dev) {
  feature_err_.clear();
  if (status_) return status_;
  const int n = S_->n;
  const bool all = !sel || nsel < 0;
  const int64_t nout = all ? n : nsel;
  if (job < 0 || job > 2 || k < 0 || !bptr || !x || ldx < nout) return -10;
  if (opt_.nranks > 1) return -98;   // a rank of a partition holds a part of L only
  if (k == 0 || nout == 0 || n == 0) return 0;
  HIPCHK(hipSetDevice(device_), "hipSetDevice");
  int rc = prepare_solve_many(false);
  if (rc) return rc;
  if ((rc = ss_filterable())) return rc;
  SsHandleBackend be(*this, "solve_sparse", bptr, brow, bval, all ? -1 : nsel, all ? nullptr : sel);
  return ss_solve_sequence(be, SsSolveCall{k, job, all, dev, x, ldx, nout});
}

int Engine::gram_sparse(int k, const int* bptr, const int* brow, const double* bval, double* g_host, int64_t ldg) {
  feature_err_.clear();
  if (status_) return status_;
  const int n = S_->n;
  if (k < 0 || !bptr || !g_host || ldg < k) return -10;
  if (opt_.nranks > 1) return -98;
  if (k == 0) return 0;
  if (n == 0) {
    for (int j = 0; j < k; ++j)
      for (int i = 0; i < k; ++i) g_host[(int64_t)j * ldg + i] = 0.0;
    return 0;
  }
  HIPCHK(hipSetDevice(device_), "hipSetDevice");
  int rc = prepare_solve_many(false);
  if (rc) return rc;
  if ((rc = ss_filterable())) return rc;
  SsHandleBackend be(*this, "gram_sparse", bptr, brow, bval, -1, nullptr);
  return ss_gram_sequence(be, k, false, g_host, ldg);
}

static const char* const kBssRepro =
    "not available while the reproducible batch is switched on (spllt_hip_set_batch_reproducible): the filtered sweeps "
    "run the kernels that add with atomics";

int Engine::solve_sparse_batch(int k, const int* bptr, const int* brow, const double* bval, int64_t ldb, int nsel,
                               const int* sel, double* x, int64_t ldx, int job, bool dev) {
  feature_err_.clear();
  if (status_) return status_;
  const int n = S_->n, nbatch = bt_.nbatch;
  const bool all = !sel || nsel < 0;
  const int64_t nout = all ? n : nsel;
  if (job < 0 || job > 2 || k < 0 || !bptr || !x || ldx < nout) return -10;
  if (k > 0 && ((bptr[k] > bptr[0] && !bval) || (ldb != 0 && ldb < (int64_t)bptr[k] - 1))) return -10;
  if (opt_.nranks > 1) return -98;   // a rank of a partition holds a part of L only
  if (pending_ || nbatch <= 0) return -10;
  if (brp_on_) {
    feature_err_ = std::string("solve_sparse_batch: ") + kBssRepro;
    return -98;
  }
  for (int64_t& v : bss_.info) v = 0;
  if (k == 0 || nout == 0 || n == 0) return 0;
  HIPCHK(hipSetDevice(device_), "hipSetDevice");
  if (int rc = bss_enter()) return rc;
  SsBatchBackend be(*this, "solve_sparse_batch", k, bptr, brow, bval, ldb, all ? -1 : nsel, all ? nullptr : sel);
  return ss_solve_sequence(be, SsSolveCall{k, job, all, dev, x, ldx, nout});
}

int Engine::gram_sparse_batch(int k, const int* bptr, const int* brow, const double* bval, int64_t ldb, double* gout,
                              int64_t ldg, bool dev) {
  feature_err_.clear();
  if (status_) return status_;
  const int n = S_->n, nbatch = bt_.nbatch;
  if (k < 0 || !bptr || !gout || ldg < k) return -10;
  if (k > 0 && ((bptr[k] > bptr[0] && !bval) || (ldb != 0 && ldb < (int64_t)bptr[k] - 1))) return -10;
  if (opt_.nranks > 1) return -98;
  if (pending_ || nbatch <= 0) return -10;
  if (brp_on_) {
    feature_err_ = std::string("gram_sparse_batch: ") + kBssRepro;
    return -98;
  }
  for (int64_t& v : bss_.info) v = 0;
  if (k == 0) return 0;
  HIPCHK(hipSetDevice(device_), "hipSetDevice");
  if (n == 0) {   // (no member can be flagged)
    if (dev) {
      for (int64_t c = 0; c < (int64_t)nbatch * k; ++c)
        HIPCHK(hipMemsetAsync(gout + c * ldg, 0, sizeof(double) * (size_t)k, stream_), "gram_sparse_batch clear");
      return sync_stream(stream_, "gram_sparse_batch sync");
    }
    for (int64_t c = 0; c < (int64_t)nbatch * k; ++c)
      for (int i = 0; i < k; ++i) gout[c * ldg + i] = 0.0;
    return 0;
  }
  if (int rc = bss_enter()) return rc;
  SsBatchBackend be(*this, "gram_sparse_batch", k, bptr, brow, bval, ldb, -1, nullptr);
  return ss_gram_sequence(be, k, dev, gout, ldg);
}

// ---- reproducible solve ----------------------------------------------------------------------------
static std::atomic<bool> g_rsolve_poison{false};
void set_rsolve_poison(bool on) { g_rsolve_poison.store(on); }

// the RsolveTables of the substitution program, uploaded once; rs_stride_ = max(frows, bsize)
void Engine::ensure_rsolve_tables(FeatureTake& t) {
  if (d_rstab_) return;
  RsolveTables R;
  build_rsolve_tables(*S_, sprog_, R);
  rs_stride_ = std::max<int64_t>(1, std::max(R.frows, R.bsize));
  TableStager tab;
  tab.add(&d_rsfslot_, R.fslot);
  tab.add(&d_rsbfirst_, R.bfirst);
  tab.add(&d_rsgptr_, R.gptr);
  tab.add(&d_rsgsrc_, R.gsrc);
  tab.add(&d_rsbslot_, R.bslot);
  t.tables(tab, &d_rstab_);
}

void Engine::unhold_rsolve_tables() {
  rs_users_.drop([this] { give_back(d_rstab_); });
}

int Engine::prepare_solve_repro() {
  int rc = prepare_solve();
  if (rc) return rc;
  if (rs_ready_) return 0;
  const Symbolic& S = *S_;
  // (a failure here leaves the factor and the other solves usable: the engine's status is not touched)
  auto t = take();
  ensure_rsolve_tables(t);
  const size_t sb = sizeof(double) * 4 * (size_t)rs_stride_;
  if (t.ok()) t.check(ensure_order());
  t(&d_rsscratch_, sb);
  t(&d_rsstage_, sizeof(double) * 4 * (size_t)std::max(1, S.n));
  if (!t.ok()) {
    feature_err_ = "solve_repro: not enough device memory for the tables and the scratch of 4 right-hand sides (" +
                   std::to_string(sb >> 20) + " MiB): " + hipGetErrorString(t.error());
    return alloc_code(t.error());
  }
  t.commit();
  rs_users_.hold();
  rs_ready_ = true;
  return 0;
}

int Engine::release_solve_repro() {
  int rc;
  if (!enter_release(rs_ready_, "solve_repro release", &rc)) return rc;
  give_back(d_rsscratch_, d_rsstage_);
  rs_ready_ = false;
  unhold_rsolve_tables();
  return 0;
}

// the sweeps `job` asks for on cur = 1, 2 or 4 vectors in pivot order, y[q * ldy + p] (enqueue only)
int Engine::enqueue_solve_repro(double* y, int64_t ldy, int cur, int job) {
  const RsolveView rv{d_rsfslot_, d_rsbfirst_, d_rsgptr_, d_rsgsrc_, d_rsbslot_, d_rsscratch_, rs_stride_};
  const SolveTablesView tv = solve_tables();
  for (int sweep = 1; sweep <= 2; ++sweep) {   // forward, backward
    if (job != 0 && job != sweep) continue;
    // debug: a slot that is read without having been written in this sweep shows up as NaN
    if (g_rsolve_poison.load())
      HIPCHK(hipMemsetAsync(d_rsscratch_, 0xFF, sizeof(double) * 4 * (size_t)rs_stride_, stream_), "poison the scratch");
    for_each_solve_launch(sweep, -1, [&](const SolveLaunch& l, const SolveLaunchInfo& li) {
      launch_solve_repro(stream_, tv, l, li, y, cur, ldy, rv);
    });
  }
  return 0;
}

int Engine::solve_repro_dev(double* x_dev, int nrhs, int64_t ldx, int job, bool pivot_order) {
  int rc;
  if (!enter(job >= 0 && job <= 2 && nrhs >= 0 && x_dev && ldx >= S_->n, nrhs == 0 || S_->n == 0, &rc)) return rc;
  if ((rc = prepare_solve_repro())) return rc;
  const int n = S_->n;
  rc = for_each_group4(nrhs, [&](int done, int cur) -> int {
    double* xg = x_dev + (int64_t)done * ldx;
    if (pivot_order) return enqueue_solve_repro(xg, ldx, cur, job);
    launch_permute_vectors(stream_, false, xg, ldx, d_order_, n, cur, d_y_);
    if (int r = enqueue_solve_repro(d_y_, (int64_t)n, cur, job)) return r;
    launch_permute_vectors(stream_, true, xg, ldx, d_order_, n, cur, d_y_);
    return 0;
  });
  if (rc) return rc;
  HIPCHK(hipGetLastError(), "solve_repro launch");
  return sync_stream(stream_, "solve_repro sync");
}

int Engine::solve_repro(double* x_host, int nrhs, int64_t ldx, int job) {
  int rc;
  if (!enter(job >= 0 && job <= 2 && nrhs >= 0 && x_host && ldx >= S_->n, nrhs == 0 || S_->n == 0, &rc)) return rc;
  if ((rc = prepare_solve_repro())) return rc;
  const int n = S_->n;
  return for_each_group4(nrhs, [&](int done, int cur) -> int {
    double* xg = x_host + (int64_t)done * ldx;
    // the group in the caller's layout, its n-vectors only (the permutation happens on the device)
    if ((rc = copy_vectors(true, d_rsstage_, xg, ldx, cur, "rhs H2D"))) return rc;
    launch_permute_vectors(stream_, false, d_rsstage_, (int64_t)n, d_order_, n, cur, d_y_);
    if ((rc = enqueue_solve_repro(d_y_, (int64_t)n, cur, job))) return rc;
    launch_permute_vectors(stream_, true, d_rsstage_, (int64_t)n, d_order_, n, cur, d_y_);
    HIPCHK(hipGetLastError(), "solve_repro launch");
    if ((rc = copy_vectors(false, d_rsstage_, xg, ldx, cur, "x D2H"))) return rc;
    return sync_stream(stream_, "solve_repro sync");
  });
}

// ---- products with the factor, Gaussian sampling ---------------------------------------------------
static std::atomic<bool> g_fmult_poison{false};
void set_fmult_poison(bool on) { g_fmult_poison.store(on); }
void set_fmult_alloc_fail(int n) { fmult_alloc_fail_left().store(n); }
void set_alloc_fail_at(int k) { alloc_fail_countdown().store(std::max(k, 0)); }
bool alloc_fail_armed() { return alloc_fail_countdown().load() > 0; }

// the tables of the products: the RsolveTables and the (block column, chunk of 64 pivot positions) pairs of the
// diagonal launches, block columns ascending
void Engine::ensure_fmult_tables(FeatureTake& t) {
  if (d_fmtab_) return;
  std::vector<UpdTile> chunks;
  for (size_t b = 0; b < sprog_.units.size(); ++b)
    for (int c = 0; c * 64 < sprog_.units[b].w; ++c) chunks.push_back(UpdTile{(int)b, (short)c, 0});
  fm_nchunks_ = (int64_t)chunks.size();
  ensure_rsolve_tables(t);
  TableStager tab;
  tab.add(&d_fmchunks_, chunks);
  t.tables(tab, &d_fmtab_);
}

// (after the commit of the transaction that ensured them)
void Engine::hold_fmult_tables() {
  if (fm_users_.users == 0) rs_users_.hold();
  fm_users_.hold();
}

void Engine::unhold_fmult_tables() {
  fm_users_.drop([this] {
    give_back(d_fmtab_);
    d_fmchunks_ = nullptr;
    unhold_rsolve_tables();
  });
}

int Engine::prepare_factor_mult(bool host_stage) {
  int rc = prepare_solve_many(host_stage);
  if (rc) return rc;
  if (fm_ready_) return 0;
  const size_t n1 = (size_t)std::max(1, S_->n);
  // (a failure here leaves the factor and every solve usable: the engine's status is not touched)
  auto t = take();
  ensure_fmult_tables(t);
  size_t want = 0;
  // (per vector the same sums in the same order at either width)
  if (t.ok())
    t.check(take_block_buffers({{(void**)&d_fmW_, sizeof(double) * n1}, {(void**)&d_fmscratch_, sizeof(double) * (size_t)rs_stride_}},
                               &fm_rb_, &want));
  if (const hipError_t e = t.error()) {
    feature_err_ = "factor_mult: not enough device memory for the tables, the second workspace and the scratch of 16 "
                   "vectors (" + std::to_string(want >> 20) + " MiB): " + hipGetErrorString(e);
    return alloc_code(e);
  }
  t.commit();
  hold_fmult_tables();
  fm_ready_ = true;
  return 0;
}

int Engine::release_factor_mult() {
  int rc;
  if (!enter_release(fm_ready_ || d_fmmean_, "factor_mult release", &rc)) return rc;
  give_back(d_fmW_, d_fmscratch_, d_fmmean_);
  if (fm_ready_) unhold_fmult_tables();
  fm_ready_ = false;
  return 0;
}

// one block of nv <= rb vectors: pack, the products `job` asks for (factor_mult_sequence), unpack (enqueue only)
void Engine::enqueue_factor_mult_block(double* x_dev, int64_t ldx, int nv, int rb, int job, bool pivot_order) {
  const int n = S_->n;
  const int* order = pivot_order ? nullptr : d_order_;
  const SolveTablesView tv = solve_tables();
  const FmultView fv{d_rsfslot_, d_rsbfirst_, d_rsgptr_, d_rsgsrc_, d_rsbslot_, d_fmscratch_};
  const int64_t ntiles = (int64_t)sprog_.tiles.size();
  auto product = [&](bool transpose, const double* X, double* Y) {
    // debug: a slot that is read without having been written by this product shows up as NaN
    if (g_fmult_poison.load())
      (void)hipMemsetAsync(d_fmscratch_, 0xFF, sizeof(double) * (size_t)fm_rb_ * (size_t)rs_stride_, stream_);
    launch_factor_mult(stream_, tv, ntiles, d_fmchunks_, fm_nchunks_, transpose, X, Y, rb, fv);
  };
  launch_solve_many_pack(stream_, x_dev, ldx, order, n, nv, rb, d_smW_);
  launch_solve_many_unpack(stream_, x_dev, ldx, order, n, nv, rb, factor_mult_sequence(job, d_smW_, d_fmW_, product));
}

int Engine::run_factor_mult(double* x, bool on_device, int nvec, int64_t ldx, int job, bool pivot_order) {
  int rc;
  if (!enter(job >= 0 && job <= 2 && nvec >= 0 && x && ldx >= S_->n, nvec == 0 || S_->n == 0, &rc)) return rc;
  if ((rc = prepare_factor_mult(!on_device))) return rc;
  return walk_blocks({"factor_mult", x, on_device, nvec, ldx, 1, d_smstage_, fm_rb_, pivot_order},
                     [&](int, double* xd, int64_t, int64_t ld, int nv, int rb, bool po) {
                       enqueue_factor_mult_block(xd, ld, nv, rb, job, po);
                       return 0;
                     });
}

int Engine::factor_mult_dev(double* x_dev, int nvec, int64_t ldx, int job, bool pivot_order) {
  return run_factor_mult(x_dev, true, nvec, ldx, job, pivot_order);
}

int Engine::factor_mult(double* x_host, int nvec, int64_t ldx, int job) {
  return run_factor_mult(x_host, false, nvec, ldx, job, false);
}

int Engine::white_noise_dev(double* z_dev, int nsamp, int64_t ldz, uint64_t seed, uint64_t first) {
  int rc;
  if (!enter(nsamp >= 0 && z_dev && ldz >= S_->n, nsamp == 0 || S_->n == 0, &rc)) return rc;
  launch_white_noise(stream_, z_dev, ldz, nullptr, S_->n, nsamp, seed, first);
  HIPCHK(hipGetLastError(), "white_noise launch");
  return sync_stream(stream_, "white_noise sync");
}

// The noise is written where the operation that follows expects a pivot-order vector laid out in user
// positions (x[i] = z[order[i]]): the product and the sweeps then run through their own entry points.
int Engine::sample(double* x, int nsamp, int64_t ldx, int kind, uint64_t seed, uint64_t first, const double* mean,
                   bool dev) {
  const int n = S_->n;
  int rc;
  if (!enter(kind >= 0 && kind <= 1 && nsamp >= 0 && x && ldx >= n, nsamp == 0 || n == 0, &rc)) return rc;
  rc = kind == 1 ? prepare_factor_mult(!dev) : (repro_on_ ? prepare_solve_repro() : 0);
  if (!rc) rc = prepare_solve_many(!dev);   // (the order table; the staging block of the host entry point)
  if (rc) return rc;
  const double* dmean = mean;
  if (mean && !dev) {
    if (!d_fmmean_) {
      auto t = take();
      t(&d_fmmean_, sizeof(double) * (size_t)n);
      if (!t.ok()) {
        feature_err_ = std::string("sample: not enough device memory for the mean: ") + hipGetErrorString(t.error());
        return alloc_code(t.error());
      }
      t.commit();
    }
    HIPCHK(hipMemcpyAsync(d_fmmean_, mean, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, stream_), "mean H2D");
    dmean = d_fmmean_;
  }
  // one group on device vectors xg (vector q at xg + q * ld): noise, the operation, the mean
  auto group = [&](double* xg, int64_t ld, int nv, uint64_t s0) -> int {
    launch_white_noise(stream_, xg, ld, d_order_, n, nv, seed, s0);
    int r = 0;
    if (kind == 1) r = factor_mult_dev(xg, nv, ld, 1, false);
    else if (repro_on_) r = solve_repro_dev(xg, nv, ld, 2, false);
    else r = solve_many_dev(xg, nv, ld, 2, false);
    if (r) return r;
    if (dmean) launch_add_mean(stream_, xg, ld, dmean, n, nv);
    HIPCHK(hipGetLastError(), "sample launch");
    return 0;
  };
  if (dev) {
    if ((rc = group(x, ldx, nsamp, first))) return rc;
    return sync_stream(stream_, "sample sync");
  }
  // groups of at most 32 (what the staging block holds): min(left, 32) is the block rule's nv at cap 32 for every left
  return walk_blocks({"sample", x, false, nsamp, ldx, 1, d_smstage_, 32, false, false},
                     [&](int done, double* xg, int64_t, int64_t ld, int nv, int, bool) {
                       return group(xg, ld, nv, first + (uint64_t)done);
                     });
}

// ---- the products and the samplers for every member of a batch ---------------------------------------
void Engine::drop_factor_mult_batch() {
  give_back(d_bmW_[0], d_bmW_[1], d_bmscratch_, d_bmmean_);
  bm_mean_elems_ = 0;
  bm_capacity_ = 0;
  if (bm_ready_) unhold_fmult_tables();
  bm_ready_ = false;
}

// tables (shared with the single-handle products), two workspaces and the scratch for the members of the last
// batch; all or nothing
int Engine::prepare_factor_mult_batch() {
  int rc = prepare_solve();   // (the handle's solve_units / solve_tiles: they describe every member's arena)
  if (rc) return rc;
  const int nbatch = bt_.nbatch;
  if (bm_ready_ && nbatch <= bm_capacity_) return 0;
  if (bm_ready_) drop_factor_mult_batch();   // (a larger batch: everything again)
  const size_t n1 = (size_t)std::max(1, S_->n);
  // (a failure here leaves the batch, its solve and the single factorization usable)
  auto t = take();
  t.check(ensure_order());
  ensure_fmult_tables(t);
  size_t want = 0;
  if (t.ok()) {
    const size_t wb = sizeof(double) * (size_t)nbatch * n1, sb = sizeof(double) * (size_t)nbatch * (size_t)rs_stride_;
    t.check(take_block_buffers({{(void**)&d_bmW_[0], wb}, {(void**)&d_bmW_[1], wb}, {(void**)&d_bmscratch_, sb}}, &bm_rb_, &want));
  }
  if (const hipError_t e = t.error()) {
    feature_err_ = "factor_mult_batch: not enough device memory for the tables, two workspaces and the scratch of 16 "
                   "vectors for each of " + std::to_string(nbatch) + " members (" + std::to_string(want >> 20) +
                   " MiB): " + hipGetErrorString(e);
    return alloc_code(e);
  }
  // experiment knob of scripts/factor_mult_batch_bench.py (the A/B of the two grid orders)
  if (const char* env = std::getenv("SPLLT_BATCH_MULT_MEMBER_FAST")) bm_member_fast_ = std::atoi(env) != 0;
  t.commit();
  hold_fmult_tables();
  bm_capacity_ = nbatch;
  bm_ready_ = true;
  return 0;
}

int Engine::release_factor_mult_batch() {
  int rc;
  if (!enter_release(bm_ready_ || d_bmmean_, "factor_mult_batch release", &rc)) return rc;
  drop_factor_mult_batch();
  return 0;
}

BmultView Engine::bmult_view(int rb) const {
  return BmultView{bt_.L, bt_.flag, bt_.lstride, (int64_t)rb * S_->n, (int64_t)rb * rs_stride_, bt_.nbatch, bm_member_fast_};
}

int Engine::batch_failed() const {
  for (int fl : bt_.hflag)
    if (fl != INT_MAX) return kErrNotPosDef;
  return 0;
}

// one block of nv <= rb vectors of every member (member b's at x_dev + b * xstride): pack, the products `job`
// asks for, unpack (enqueue only); the workspaces play the parts of enqueue_factor_mult_block
void Engine::enqueue_factor_mult_batch_block(double* x_dev, int64_t xstride, int64_t ldx, int nv, int rb, int job,
                                             bool pivot_order) {
  const int n = S_->n;
  const int* order = pivot_order ? nullptr : d_order_;
  const SolveTablesView tv = solve_tables();
  const BmultView v = bmult_view(rb);
  const FmultView fv{d_rsfslot_, d_rsbfirst_, d_rsgptr_, d_rsgsrc_, d_rsbslot_, d_bmscratch_};
  const int64_t ntiles = (int64_t)sprog_.tiles.size();
  auto product = [&](bool transpose, const double* X, double* Y) {
    // debug: a slot that is read without having been written by this product shows up as NaN
    if (g_fmult_poison.load())
      (void)hipMemsetAsync(d_bmscratch_, 0xFF, sizeof(double) * (size_t)bm_capacity_ * (size_t)bm_rb_ * (size_t)rs_stride_,
                           stream_);
    launch_batch_mult(stream_, v, tv, ntiles, d_fmchunks_, fm_nchunks_, transpose, X, Y, rb, fv);
  };
  launch_batch_mult_pack(stream_, v, false, x_dev, xstride, ldx, order, n, nv, rb, d_bmW_[0]);
  launch_batch_mult_pack(stream_, v, true, x_dev, xstride, ldx, order, n, nv, rb,
                         factor_mult_sequence(job, d_bmW_[0], d_bmW_[1], product));
}

// device vectors, or groups of at most 32 host vectors per member through the batch's staging buffer
int Engine::run_factor_mult_batch(double* x, bool on_device, int nvec, int64_t ldx, int job, bool pivot_order) {
  const int n = S_->n, nbatch = bt_.nbatch;
  int rc;
  if (!enter(x && nvec >= 0 && ldx >= n && job >= 0 && job <= 2 && nbatch > 0, nvec == 0 || n == 0, &rc)) return rc;
  if ((rc = prepare_factor_mult_batch())) return rc;
  if (!on_device &&
      (rc = grow_batch_buffer(&bt_.stage, &bt_.stage_elems, (size_t)nbatch * (size_t)std::min(nvec, 32) * (size_t)n,
                              "the staged vectors")))
    return rc;
  rc = walk_blocks({"factor_mult_batch", x, on_device, nvec, ldx, nbatch, bt_.stage, bm_rb_, pivot_order},
                   [&](int, double* xd, int64_t xs, int64_t ld, int nv, int rb, bool po) {
                     enqueue_factor_mult_batch_block(xd, xs, ld, nv, rb, job, po);
                     return 0;
                   });
  return rc ? rc : batch_failed();
}

int Engine::factor_mult_batch_dev(double* x_dev, int nvec, int64_t ldx, int job, bool pivot_order) {
  return run_factor_mult_batch(x_dev, true, nvec, ldx, job, pivot_order);
}

int Engine::factor_mult_batch(double* x_host, int nvec, int64_t ldx, int job) {
  return run_factor_mult_batch(x_host, false, nvec, ldx, job, false);
}

int Engine::white_noise_batch_dev(double* z_dev, int nsamp, int64_t ldz, uint64_t seed, uint64_t first, uint32_t stream0,
                                  int stream_step) {
  int rc;
  if (!enter(z_dev && nsamp >= 0 && ldz >= S_->n && stream_step >= 0 && stream_step <= 1 && bt_.nbatch > 0,
             nsamp == 0 || S_->n == 0, &rc))
    return rc;
  launch_batch_white_noise(stream_, bmult_view(16), z_dev, (int64_t)nsamp * ldz, ldz, nullptr, S_->n, nsamp, seed, first,
                           stream0, stream_step);
  HIPCHK(hipGetLastError(), "white_noise_batch launch");
  if ((rc = sync_stream(stream_, "white_noise_batch sync"))) return rc;
  return batch_failed();
}

// As Engine::sample: the noise is written where the operation that follows expects a pivot-order vector laid out in
// user positions, the product and the sweep then run through their own batch entry points.
int Engine::sample_batch(double* x, int nsamp, int64_t ldx, int kind, uint64_t seed, uint64_t first, uint32_t stream0,
                         int stream_step, const double* mean, int64_t ldmean, bool dev) {
  const int n = S_->n, nbatch = bt_.nbatch;
  int rc;
  if (!enter(x && nsamp >= 0 && ldx >= n && kind >= 0 && kind <= 1 && stream_step >= 0 && stream_step <= 1 &&
                 !(mean && ldmean != 0 && ldmean < n) && nbatch > 0,
             nsamp == 0 || n == 0, &rc))
    return rc;
  if (kind == 1 && (rc = prepare_factor_mult_batch())) return rc;
  if (hipError_t e = ensure_order()) {
    (void)hipGetLastError();
    feature_err_ = std::string("sample_batch: the order table could not be uploaded: ") + hipGetErrorString(e);
    return alloc_code(e);
  }
  const double* dmean = mean;
  int64_t ldm = ldmean;
  if (mean && !dev) {
    const size_t nm = ldmean == 0 ? 1 : (size_t)nbatch;
    if ((rc = grow_batch_buffer(&d_bmmean_, &bm_mean_elems_, nm * (size_t)n, "the means"))) return rc;
    if ((rc = copy_vectors_to_device(d_bmmean_, mean, ldmean, (int64_t)nm, "mean H2D"))) return rc;
    dmean = d_bmmean_;
    ldm = ldmean == 0 ? 0 : n;
  }
  // one group of nv samples per member on device vectors (member b's at xg + b * xs, sample q at + q * ld)
  auto group = [&](double* xg, int64_t xs, int64_t ld, int nv, uint64_t s0) -> int {
    launch_batch_white_noise(stream_, bmult_view(16), xg, xs, ld, d_order_, n, nv, seed, s0, stream0, stream_step);
    if (kind == 1) {
      for_each_block(nv, bm_rb_, [&](int done, int cur, int rb) {
        enqueue_factor_mult_batch_block(xg + (int64_t)done * ld, xs, ld, cur, rb, 1, false);
        return 0;
      });
    } else {
      // (xs = nv * ld: the layout of solve_batch; its -20 is this call's own: the failed members keep their NaN)
      const int r = bsm_on_ ? solve_many_batch(xg, true, nv, ld, 2, false) : solve_batch(xg, true, nv, ld, 2, false);
      if (r && r != kErrNotPosDef) return r;
    }
    if (dmean) launch_batch_add_mean(stream_, bmult_view(16), xg, xs, ld, dmean, ldm, n, nv);
    HIPCHK(hipGetLastError(), "sample_batch launch");
    return 0;
  };
  if (dev) {
    if ((rc = group(x, (int64_t)nsamp * ldx, ldx, nsamp, first))) return rc;
    if ((rc = sync_stream(stream_, "sample_batch sync"))) return rc;
    return batch_failed();
  }
  // groups of at most 32 samples per member through the batch's staging buffer, packed (vector q of member b at
  // (b * nv + q) * n: the layout of solve_batch, which stages nothing for vectors that are on the device)
  // (min(left, 32) is the block rule's nv at cap 32 for every left)
  if ((rc = grow_batch_buffer(&bt_.stage, &bt_.stage_elems, (size_t)nbatch * (size_t)std::min(nsamp, 32) * (size_t)n,
                              "the staged samples")))
    return rc;
  rc = walk_blocks({"sample_batch", x, false, nsamp, ldx, nbatch, bt_.stage, 32, false, false},
                   [&](int done, double* xg, int64_t xs, int64_t ld, int nv, int, bool) {
                     return group(xg, xs, ld, nv, first + (uint64_t)done);
                   });
  return rc ? rc : batch_failed();
}

// ---- blocked solve for every member of a batch -------------------------------------------------------
void Engine::drop_solve_many_batch() {
  give_back(d_bsmW_);
  bsm_capacity_ = 0;
  bsm_ready_ = false;
  bsm_info_[0] = bsm_info_[3] = 0;
}

// the workspace for the members of the last batch: 32 vectors per member, or 16 when that does not fit
int Engine::prepare_solve_many_batch() {
  const int nbatch = bt_.nbatch;
  // the reproducible form needs its tables and its scratch besides; a scratch that only fits blocks of 16 narrows
  // the blocks of the walk (the workspace holds them either way)
  auto repro = [&]() -> int {
    if (!brp_sweep()) return 0;
    if (int rc = prepare_solve_repro_batch()) return rc;
    if (brp_.sw_rb < bsm_rb_) bsm_info_[0] = bsm_rb_ = brp_.sw_rb;
    return 0;
  };
  if (bsm_ready_ && nbatch <= bsm_capacity_) return repro();
  if (bsm_ready_) drop_solve_many_batch();   // (a larger batch: the workspace again)
  const size_t n1 = (size_t)std::max(1, S_->n);
  // (a failure here leaves the batch, solve_batch and the single factorization usable)
  hipError_t e = ensure_order();
  size_t want = 0;
  if (e == hipSuccess) e = take_block_buffers({{(void**)&d_bsmW_, sizeof(double) * (size_t)nbatch * n1}}, &bsm_rb_, &want);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    feature_err_ = "solve_many_batch: not enough device memory for the workspace of 16 right-hand sides for each of " +
                   std::to_string(nbatch) + " members (" + std::to_string(want >> 20) + " MiB): " + hipGetErrorString(e);
    return alloc_code(e);
  }
  bsm_capacity_ = nbatch;
  bsm_ready_ = true;
  bsm_info_[0] = bsm_rb_;
  bsm_info_[3] = (int64_t)want;
  return repro();
}

// ---- the reproducible form of the blocked sweep (batch_repro.hip) ----------------------------------------
static std::atomic<bool> g_batch_repro_poison{false};
void set_batch_repro_poison(bool on) { g_batch_repro_poison.store(on); }
bool batch_repro_poison() { return g_batch_repro_poison.load(); }

void Engine::drop_solve_repro_batch() {
  give_back(brp_.swscratch, brp_.d_swtab);
  brp_.fslot = brp_.bfirst = brp_.gptr = brp_.gsrc = brp_.bslot = nullptr;
  brp_.sw_rb = brp_.sw_capacity = brp_.last_rb = 0;
}

// the tables of the batch's own solve program and rb max(frows, bsize) doubles per member of the last batch, one
// transaction (taken again together when a later batch has more members): rb = 32, or 16 when that does not fit
int Engine::prepare_solve_repro_batch() {
  const int nbatch = bt_.nbatch;
  if (brp_.swscratch && nbatch <= brp_.sw_capacity) return 0;
  drop_solve_repro_batch();   // (a larger batch: the scratch again)
  RsolveTables R;
  build_rsolve_tables(*S_, bt_.sprog, R);
  brp_.slots = std::max<int64_t>(1, std::max(R.frows, R.bsize));
  TableStager tab;
  tab.add(&brp_.fslot, R.fslot);
  tab.add(&brp_.bfirst, R.bfirst);
  tab.add(&brp_.gptr, R.gptr);
  tab.add(&brp_.gsrc, R.gsrc);
  tab.add(&brp_.bslot, R.bslot);
  // (a failure here leaves the batch, every other solve and the single factorization usable)
  auto t = take();
  t.tables(tab, &brp_.d_swtab);
  size_t want = 0;
  int rb = 32;
  if (t.ok())
    t.check(take_block_buffers({{(void**)&brp_.swscratch, sizeof(double) * (size_t)nbatch * (size_t)brp_.slots}}, &rb, &want));
  if (const hipError_t e = t.error()) {
    give_back(brp_.swscratch);
    feature_err_ = "reproducible batch sweep: not enough device memory for the tables and the scratch of 16 right-hand "
                   "sides for each of " + std::to_string(nbatch) + " members (" + std::to_string(want >> 20) + " MiB): " +
                   hipGetErrorString(e);
    return alloc_code(e);
  }
  t.commit();
  brp_.sw_rb = rb;
  brp_.sw_capacity = nbatch;
  return 0;
}

int Engine::release_batch_repro() {
  int rc;
  if (!enter_release(brp_.swscratch || brp_.d_swtab, "batch_repro release", &rc)) return rc;
  drop_solve_repro_batch();
  return 0;
}

void Engine::batch_repro_info(int64_t out[6]) const {
  out[0] = brp_on_ ? 1 : 0;
  out[1] = bt_.nbatch > 0 && brp_.last_det ? 1 : 0;
  out[2] = out[1] ? bt_.launches : 0;
  out[3] = brp_.last_rb;
  out[4] = (int64_t)sizeof(double) * brp_.fstride * brp_.f_capacity;
  out[5] = (int64_t)sizeof(double) * brp_.slots * brp_.sw_rb * brp_.sw_capacity;
}

int Engine::solve_repro_batch(double* x, bool on_device, int nrhs, int64_t ldx, int job, bool pivot_order) {
  brp_force_ = true;
  const int rc = solve_many_batch(x, on_device, nrhs, ldx, job, pivot_order);
  brp_force_ = false;
  return rc;
}

int Engine::release_solve_many_batch() {
  int rc;
  if (!enter_release(bsm_ready_, "solve_many_batch release", &rc)) return rc;
  drop_solve_many_batch();
  return 0;
}

// one block of nv <= rb vectors of every member (member b's at x_dev + b * xstride): pack, the sweeps `job` asks
// for in the order of solve_batch, unpack (enqueue only)
int Engine::enqueue_solve_many_batch_block(double* x_dev, int64_t xstride, int64_t ldx, int nv, int rb, int job,
                                           bool pivot_order) {
  const int n = S_->n;
  const int* order = pivot_order ? nullptr : d_order_;
  const BatchView v = batch_view();
  int nl = 0;
  bool fits = true;
  auto count = [&](int k) { if (k < 0) fits = false; else nl += k; };
  // the reproducible batch: the same launches in the same order by the kernels of batch_repro.hip (the caller's
  // prepare_solve_many_batch has taken their tables and scratch; without them nothing is launched)
  const bool repro = brp_sweep();
  if (repro && !(brp_.swscratch && rb <= brp_.sw_rb)) return -1;
  count(launch_batch_solve_many_pack(stream_, v, false, x_dev, xstride, ldx, order, n, nv, rb, d_bsmW_));
  if (!fits) return -1;   // (nothing was launched: the vectors are as they were)
  const BatchReproView rs{v, brp_.swscratch, (int64_t)brp_.sw_rb * brp_.slots};
  const RsmTables tb{brp_.fslot, brp_.bfirst, brp_.gptr, brp_.gsrc, brp_.bslot};
  if (repro) brp_.last_rb = rb;
  auto run = [&](const std::vector<SolveLaunch>& ls) {
    // debug: a slot that is read without having been written in this sweep shows up as NaN
    if (repro && batch_repro_poison())
      (void)hipMemsetAsync(brp_.swscratch, 0xFF, sizeof(double) * (size_t)rs.sstride * (size_t)brp_.sw_capacity, stream_);
    for (const SolveLaunch& l : ls)
      count(repro ? launch_batch_solve_repro(stream_, rs, l, bt_.slist, bt_.stiles, bt_.sunits, d_rlist_, tb, d_bsmW_, rb, n)
                  : launch_batch_solve_many(stream_, v, l, bt_.slist, bt_.stiles, bt_.sunits, d_rlist_, d_bsmW_, rb, n));
  };
  if (job == 0 || job == 1) run(bt_.sprog.fwd);
  if (job == 0 || job == 2) run(bt_.sprog.bwd);
  count(launch_batch_solve_many_pack(stream_, v, true, x_dev, xstride, ldx, order, n, nv, rb, d_bsmW_));
  return fits ? nl : -1;
}

int Engine::solve_many_batch(double* x, bool on_device, int nrhs, int64_t ldx, int job, bool pivot_order) {
  const int n = S_->n, nbatch = bt_.nbatch;
  int rc;
  if (!enter(x && nrhs >= 0 && ldx >= n && job >= 0 && job <= 2 && nbatch > 0, nrhs == 0 || n == 0, &rc)) return rc;
  if ((rc = prepare_solve_many_batch())) return rc;
  if (!on_device &&
      (rc = grow_batch_buffer(&bt_.stage, &bt_.stage_elems, (size_t)nbatch * (size_t)std::min(nrhs, 32) * (size_t)n,
                              "the staged right-hand sides")))
    return rc;
  BlockTally t;
  rc = walk_blocks({"solve_many_batch", x, on_device, nrhs, ldx, nbatch, bt_.stage, bsm_rb_, pivot_order},
                   [&](int, double* xd, int64_t xs, int64_t ld, int nv, int rb, bool po) {
                     return enqueue_solve_many_batch_block(xd, xs, ld, nv, rb, job, po);
                   }, &t);
  if (rc == -1) {   // (of the enqueue; the walk's own failures are kErrHip)
    feature_err_ = "solve_many_batch: a launch has more work items for one member than a grid holds (the vectors are not "
                   "all solved)";
    return -99;
  }
  if (rc) return rc;
  bsm_info_[1] = t.blocks;
  bsm_info_[2] = t.launches;
  return batch_failed();
}

// ---- refined solves --------------------------------------------------------------------------------
// Operator tables (once per engine) and the work vectors of one group, all or nothing: a failed allocation
// gives back what it got and leaves the factor and every other solve usable.
void Engine::ensure_refine_tables(FeatureTake& t) {
  if (d_rftab_) return;
  const Symbolic& S = *S_;
  std::vector<int64_t> rowptr;
  std::vector<int> col, src, rows;
  build_matvec_tables(S, rowptr, col, src);
  // rows by length: at most 16 entries -> 4 lanes per row, at most 128 -> 16 lanes, longer -> a wavefront
  rows.reserve((size_t)S.n);
  for (int c = 0; c < 3; ++c) {
    rf_nrows_[c] = 0;
    for (int p = 0; p < S.n; ++p) {
      const int64_t len = rowptr[(size_t)p + 1] - rowptr[(size_t)p];
      const int cls = len <= 16 ? 0 : (len <= 128 ? 1 : 2);
      if (cls == c) { rows.push_back(p); ++rf_nrows_[c]; }
    }
  }
  TableStager tab;
  tab.add(&d_rfrowptr_, rowptr);
  tab.add(&d_rfcol_, col);
  tab.add(&d_rfsrc_, src);
  tab.add(&d_rfrows_, rows);
  t.tables(tab, &d_rftab_);
  if (t.ok()) t.check(ensure_order());
}

RfOperator Engine::refine_operator() const {
  return RfOperator{d_rfrowptr_, d_rfcol_, d_rfsrc_, d_rfrows_, {rf_nrows_[0], rf_nrows_[1], rf_nrows_[2]}};
}

void Engine::unhold_refine_tables() {
  rf_users_.drop([this] { give_back(d_rftab_); });
}

int Engine::prepare_refine(bool host_val) {
  const Symbolic& S = *S_;
  const size_t n1 = (size_t)std::max(1, S.n);
  auto t = take();
  size_t want = 0;
  if (!refine_ready_) {
    ensure_refine_tables(t);
    const RfOperator op = refine_operator();
    const size_t slots = (size_t)std::max(std::max(spmv_slots(op), vec_slots(S.n)), RF_AMAX_WG);
    want = sizeof(double) * 6 * RF_G * n1;
    t(&d_rfwork_, want);
    t(&d_rfpart_, sizeof(double) * 2 * RF_G * slots);
    t(&d_rfds_, sizeof(double) * RF_DS);
    t(&d_rfis_, sizeof(int) * RF_IS);
    if (t.ok()) t.check(hipMemsetAsync(d_rfis_, 0, sizeof(int) * RF_IS, stream_));
    if (t.ok()) t.check(hipMemsetAsync(d_rfds_, 0, sizeof(double) * RF_DS, stream_));
  }
  if (t.ok() && host_val && !d_rfval_) {
    want = sizeof(double) * (size_t)std::max<int64_t>(1, S.nnzA);
    t(&d_rfval_, want);
  }
  if (!t.ok()) {
    feature_err_ = "refined solve: not enough device memory for the operator and the work vectors (" +
                   std::to_string(want >> 20) + " MiB): " + hipGetErrorString(t.error());
    return alloc_code(t.error());
  }
  t.commit();
  if (!refine_ready_) rf_users_.hold();
  refine_ready_ = true;
  return 0;
}

int Engine::release_refine() {
  int rc;
  if (!enter_release(refine_ready_ || d_rfval_, "refine release", &rc)) return rc;
  give_back(d_rfwork_, d_rfpart_, d_rfds_, d_rfis_, d_rfval_);
  if (refine_ready_) unhold_refine_tables();
  refine_ready_ = false;
  return 0;
}

int Engine::matvec(const double* val, int nvec, const double* x, int64_t ldx, double* y, int64_t ldy, bool dev,
                   bool pivot_order) {
  const int n = S_->n;
  int rc;
  if (!enter(val && x && y && nvec >= 0 && ldx >= n && ldy >= n, nvec == 0 || n == 0, &rc)) return rc;
  if ((rc = prepare_refine(!dev))) return rc;
  const double* dval = val;
  if (!dev) {
    HIPCHK(hipMemcpyAsync(d_rfval_, val, sizeof(double) * (size_t)S_->nnzA, hipMemcpyHostToDevice, stream_), "val H2D");
    dval = d_rfval_;
  }
  const RfOperator op = refine_operator();
  const size_t gn = (size_t)RF_G * (size_t)n;
  double *wb = d_rfwork_, *wr = d_rfwork_ + 2 * gn, *wq = d_rfwork_ + 4 * gn;
  for (int done = 0; done < nvec;) {
    const int nv = std::min(RF_G, nvec - done);
    const double* xg = x + (int64_t)done * ldx;
    double* yg = y + (int64_t)done * ldy;
    if (dev && pivot_order) {
      launch_spmv(stream_, op, dval, xg, ldx, nullptr, yg, ldy, nv, nullptr, 0, nullptr);
    } else if (dev) {
      launch_permute_vectors(stream_, false, const_cast<double*>(xg), ldx, d_order_, n, nv, wb);   // (reads xg)
      launch_spmv(stream_, op, dval, wb, n, nullptr, wr, n, nv, nullptr, 0, nullptr);
      launch_permute_vectors(stream_, true, yg, ldy, d_order_, n, nv, wr);
    } else {
      if ((rc = copy_vectors_to_device(wq, xg, ldx, nv, "x H2D"))) return rc;
      launch_permute_vectors(stream_, false, wq, n, d_order_, n, nv, wb);
      launch_spmv(stream_, op, dval, wb, n, nullptr, wr, n, nv, nullptr, 0, nullptr);
      launch_permute_vectors(stream_, true, wq, n, d_order_, n, nv, wr);
      if ((rc = copy_vectors(false, wq, yg, ldy, nv, "y D2H"))) return rc;
    }
    HIPCHK(hipGetLastError(), "matvec launch");
    if (!dev && (rc = sync_stream(stream_, "matvec sync"))) return rc;
    done += nv;
  }
  return sync_stream(stream_, "matvec sync");
}

// both sweeps with the current factor on nv work vectors (pivot order, ld = n), through the existing paths.
// The sweeps take all nv columns, frozen vectors included (their columns are zero: launch_rf_copy), since the
// existing paths know no mask; the columns of a sweep are independent of each other.
int Engine::refine_apply_factor(double* v, int nv) {
  // (reproducible: every group size through that path, in sweeps of 4)
  if (repro_on_) return solve_repro_dev(v, nv, (int64_t)S_->n, 0, true);
  return nv <= 4 ? solve_dev(v, nv, 0, -1) : solve_many_dev(v, nv, (int64_t)S_->n, 0, true);
}

// refine_iterate on one group of nv <= RF_G vectors of the handle: work arrays of RF_G vectors each, the scalars at
// their RFD_* / RFI_* offsets, out[q] = best confirmed error, out[RF_G + q] = state
struct Engine::RefineBackend {
  Engine& e;
  const double* dval;
  int nv;
  double* x;   // the caller's vectors of this group
  int64_t ldx;
  bool dev;
  double tol;
  const int n = e.S_->n;
  const RfOperator op = e.refine_operator();
  const hipStream_t s = e.stream_;

  int fail(int code, const char* what, hipError_t err) { return e.fail(code, what, err); }
  double* w(RfVec k) const { return k == RFV_NONE ? nullptr : e.d_rfwork_ + (size_t)k * RF_G * (size_t)n; }
  const int* sel(RfSel k) const {
    constexpr int off[] = {0, RFI_ST, RFI_DECL, RFI_IMPROVE};
    return k == RFSEL_ALL ? nullptr : e.d_rfis_ + off[k];
  }
  double* part(bool partials) const { return partials ? e.d_rfpart_ : nullptr; }

  int pairs() const { return nv; }
  int stride() const { return RF_G; }
  int vslots() const { return vec_slots(n); }
  int sslots() const { return spmv_slots(op); }
  bool fits() const { return true; }
  int permute_in() {
    if (dev) {
      launch_permute_vectors(s, false, x, ldx, e.d_order_, n, nv, w(RFV_B));
      return 0;
    }
    if (int rc = e.copy_vectors(true, w(RFV_Q), x, ldx, nv, "rhs H2D")) return rc;
    launch_permute_vectors(s, false, w(RFV_Q), n, e.d_order_, n, nv, w(RFV_B));
    return 0;
  }
  void dot(RfVec a, RfVec b, RfSel k, int want, bool) { launch_rf_dot(s, n, nv, w(a), w(b), sel(k), want, e.d_rfpart_); }
  void finalize(int stage, int nslots, int flag) {
    launch_rf_finalize(s, stage, e.d_rfpart_, nslots, nv, tol, flag, e.d_rfds_, e.d_rfis_);
  }
  void copy(RfVec dst, RfVec src, RfSel k, int want, bool zero_others) {
    launch_rf_copy(s, n, nv, w(dst), w(src), sel(k), want, zero_others);
  }
  int apply_factor(RfVec v) { return e.refine_apply_factor(w(v), nv); }
  void spmv(RfVec xv, RfVec b, RfVec y, RfSel k, int want, bool partials) {
    launch_spmv(s, op, dval, w(xv), n, w(b), w(y), n, nv, sel(k), want, part(partials));
  }
  void axpy(bool alpha, RfVec xv, RfVec p, RfVec r, RfVec q, RfSel k, int want, bool partials) {
    launch_rf_axpy(s, n, nv, alpha ? e.d_rfds_ + RFD_ALPHA : nullptr, w(xv), w(p), w(r), w(q), sel(k), want, part(partials));
  }
  void pupdate(RfVec p, RfVec z, RfSel k, int want) {
    launch_rf_pupdate(s, n, nv, e.d_rfds_ + RFD_BETA, w(p), w(z), sel(k), want);
  }
  // the one array that crosses the bus per iteration
  int readback(std::vector<double>& out) {
    HIPCHK(hipGetLastError(), "refine launch");
    HIPCHK(hipMemcpyAsync(out.data(), e.d_rfds_ + RFD_OUT, sizeof(double) * 2 * RF_G, hipMemcpyDeviceToHost, s),
           "refine state D2H");
    return e.sync_stream(s, "refine sync");
  }
  int permute_out(RfVec src) {
    if (dev) {
      launch_permute_vectors(s, true, x, ldx, e.d_order_, n, nv, w(src));
      return 0;
    }
    launch_permute_vectors(s, true, w(RFV_Q), n, e.d_order_, n, nv, w(src));
    return e.copy_vectors(false, w(RFV_Q), x, ldx, nv, "x D2H");
  }
  int finish() {
    HIPCHK(hipGetLastError(), "refine launch");
    return e.sync_stream(s, "refine sync");
  }
};

int Engine::solve_refined(const double* val, int nrhs, double* x, int64_t ldx, bool dev, int method, double tol,
                          int max_iter, int* iterations, double* error) {
  feature_err_.clear();
  if (status_) return status_;
  const int n = S_->n;
  if (!val || !x || nrhs < 0 || ldx < n || method < 0 || method > 1 || !(tol > 0.0) || max_iter < 0) return -10;
  if (opt_.nranks > 1) return -98;
  if (pending_ || !factored_) return -10;   // (the caller waits first)
  if (nrhs == 0) return 0;
  if (n == 0) {
    for (int q = 0; q < nrhs; ++q) {
      if (iterations) iterations[q] = 0;
      if (error) error[q] = 0.0;
    }
    return 0;
  }
  HIPCHK(hipSetDevice(device_), "hipSetDevice");
  int rc = prepare_refine(!dev);
  if (rc) return rc;
  const double* dval = val;
  if (!dev) {
    HIPCHK(hipMemcpyAsync(d_rfval_, val, sizeof(double) * (size_t)S_->nnzA, hipMemcpyHostToDevice, stream_), "val H2D");
    dval = d_rfval_;
  }
  launch_rf_absmax(stream_, dval, S_->nnzA, d_rfpart_);
  launch_rf_finalize(stream_, RFS_AMAX, d_rfpart_, RF_AMAX_WG, 0, tol, 0, d_rfds_, d_rfis_);
  int worst = 0;
  std::vector<int> its;
  std::vector<double> out;
  for (int done = 0; done < nrhs;) {
    const int nv = std::min(RF_G, nrhs - done);
    RefineBackend be{*this, dval, nv, x + (int64_t)done * ldx, ldx, dev, tol};
    if ((rc = refine_iterate(be, method, max_iter, its, out))) return rc;
    for (int q = 0; q < nv; ++q) {
      if (iterations) iterations[done + q] = its[(size_t)q];
      if (error) error[done + q] = out[(size_t)q];
      if (out[(size_t)RF_G + q] != 1.0) worst = 1;
    }
    done += nv;
  }
  return worst;
}

// ---- refined solves for the members of a batch ---------------------------------------------------------
void Engine::drop_refine_batch() {
  give_back(d_brfwork_, d_brfpart_, d_brfds_, d_brfis_, d_brfval_, d_brfmv_);
  brf_val_elems_ = brf_mv_elems_ = 0;
  brf_capacity_ = 0;
  brf_rb_ = 0;
  brf_info_[0] = brf_info_[3] = 0;
  if (brf_ready_) unhold_refine_tables();
  if (brf_mv_held_) unhold_refine_tables();   // (the hold of the products)
  brf_ready_ = brf_mv_held_ = false;
}

// the operator tables (those of the single handle) and the storage of a pass for `members` members: six work
// arrays, the partial sums, the scalars and the states, all or nothing; 32 vectors per member, else 16, else 8
int Engine::prepare_refine_batch(int members) {
  if (brf_ready_ && members <= brf_capacity_) return 0;
  if (brf_ready_) drop_refine_batch();   // (a larger batch: everything again)
  const size_t n1 = (size_t)std::max(1, S_->n), nb = (size_t)members;
  // (a failure here leaves the batch, its solves and the single factorization usable)
  auto tables = take();
  ensure_refine_tables(tables);
  hipError_t e = tables.error();
  size_t want = 0;
  if (e == hipSuccess) {
    const RfOperator op = refine_operator();
    const size_t slots = (size_t)std::max(spmv_slots(op), vec_slots(S_->n));
    for (int rb = RF_G; rb >= 8; rb /= 2) {   // (one transaction per width)
      const size_t np = nb * (size_t)rb;
      const size_t wb = sizeof(double) * 6 * np * n1;
      const size_t pb = sizeof(double) * std::max(2 * slots * np, nb * (size_t)RF_AMAX_WG);
      const size_t db = sizeof(double) * (2 * nb + BRF_DS * np), ib = sizeof(int) * (RF_IS / RF_G) * np;
      want = wb + pb + db + ib;
      auto t = take();
      t.block(&d_brfwork_, wb);
      t(&d_brfpart_, pb);
      t(&d_brfds_, db);
      t(&d_brfis_, ib);
      if (t.ok()) t.check(hipMemsetAsync(d_brfds_, 0, db, stream_));
      if (t.ok()) t.check(hipMemsetAsync(d_brfis_, 0, ib, stream_));
      t.commit();
      e = t.error();
      if (e == hipSuccess) brf_rb_ = rb;
      if (e == hipSuccess || alloc_code(e) != -1) break;   // (out of memory: once more with half of it)
    }
  }
  if (e != hipSuccess) {
    feature_err_ = "solve_refined_batch: not enough device memory for the operator and six work arrays of 8 vectors for "
                   "each of " + std::to_string(members) + " members (" + std::to_string(want >> 20) + " MiB): " +
                   hipGetErrorString(e);
    return alloc_code(e);
  }
  tables.commit();
  rf_users_.hold();
  brf_capacity_ = members;
  brf_ready_ = true;
  brf_info_[0] = brf_rb_;
  brf_info_[3] = (int64_t)want;
  return 0;
}

int Engine::release_refine_batch() {
  int rc;
  if (!enter_release(brf_held(), "refine_batch release", &rc)) return rc;
  drop_refine_batch();
  return 0;
}

namespace {
// from this many vectors per member in a pass on, M^-1 is the blocked solve (experiment knob of
// scripts/refine_batch_bench.py: SPLLT_BRF_BLOCKED_MIN)
int brf_blocked_min() {
  if (const char* env = std::getenv("SPLLT_BRF_BLOCKED_MIN")) return std::max(1, std::atoi(env));
  return BRF_BLOCKED_MIN;
}
}  // namespace

int Engine::matvec_batch(const double* val, int64_t ldval, int nbatch, int nvec, const double* x, int64_t ldx, double* y,
                         int64_t ldy, bool dev, bool pivot_order) {
  const int n = S_->n;
  const int64_t nnz = S_->nnzA;
  int rc;
  if (!enter(val && x && y && nbatch >= 0 && nvec >= 0 && ldval >= nnz && ldx >= n && ldy >= n,
             nbatch == 0 || nvec == 0 || n == 0, &rc))
    return rc;
  // device vectors in pivot order need the tables only; else a workspace of the product's own (permuted x, y, and
  // the staged vectors of a host call), one pass of at most 32 vectors per member -- not the solver's six arrays
  const bool direct = dev && pivot_order;
  const int cap = RF_G;
  const bool first = !brf_mv_held_;
  if (first) {
    auto t = take();
    ensure_refine_tables(t);
    if (!t.ok()) {
      feature_err_ = std::string("matvec_batch: the operator tables could not be uploaded: ") + hipGetErrorString(t.error());
      return alloc_code(t.error());
    }
    t.commit();
    rf_users_.hold();
    brf_mv_held_ = true;
  }
  const size_t gcap = (size_t)nbatch * (size_t)std::min(cap, nvec) * (size_t)n;
  if (!direct && (rc = grow_batch_buffer(&d_brfmv_, &brf_mv_elems_, (dev ? 2 : 3) * gcap, "the workspace of the product"))) {
    if (first) {   // (what this call held)
      brf_mv_held_ = false;
      unhold_refine_tables();
    }
    return rc;
  }
  const double* dval = val;
  int64_t ldv = ldval;
  if (!dev) {
    if ((rc = grow_batch_buffer(&d_brfval_, &brf_val_elems_, (size_t)nbatch * (size_t)std::max<int64_t>(nnz, 1), "the staged values")))
      return rc;
    if (nnz > 0 && (rc = copy_vectors_to_device(d_brfval_, val, ldval, nbatch, "matvec_batch val H2D", nnz))) return rc;
    dval = d_brfval_;
    ldv = nnz;
  }
  const RfOperator op = refine_operator();
  BrfTally t;
  for (int done = 0; done < nvec && t.fits;) {
    const int nv = std::min(cap, nvec - done);
    const BrfView v{nullptr, nbatch, nv, nullptr, nullptr, nullptr, nullptr, nullptr};
    const size_t gn = (size_t)nbatch * (size_t)nv * (size_t)n;
    double *wb = d_brfmv_, *wr = wb ? wb + gn : nullptr, *wq = wb && !dev ? wb + 2 * gn : nullptr;
    const double* xg = x + (int64_t)done * ldx;
    double* yg = y + (int64_t)done * ldy;
    if (direct) {
      t.add(launch_bspmv(stream_, op, v, dval, ldv, xg, (int64_t)nvec * ldx, ldx, nullptr, yg, (int64_t)nvec * ldy, ldy,
                         nullptr, 0, false));
    } else {
      if (!dev)
        for (int b = 0; b < nbatch; ++b)
          if ((rc = copy_vectors_to_device(wq + (size_t)b * nv * n, xg + (int64_t)b * nvec * ldx, ldx, nv, "matvec_batch x H2D")))
            return rc;
      // (the permutation reads its source only)
      t.add(dev ? launch_brf_permute(stream_, v, false, const_cast<double*>(xg), (int64_t)nvec * ldx, ldx, d_order_, n, wb)
                : launch_brf_permute(stream_, v, false, wq, (int64_t)nv * n, n, d_order_, n, wb));
      t.add(launch_bspmv(stream_, op, v, dval, ldv, wb, (int64_t)nv * n, n, nullptr, wr, (int64_t)nv * n, n, nullptr, 0, false));
      t.add(dev ? launch_brf_permute(stream_, v, true, yg, (int64_t)nvec * ldy, ldy, d_order_, n, wr)
                : launch_brf_permute(stream_, v, true, wq, (int64_t)nv * n, n, d_order_, n, wr));
      HIPCHK(hipGetLastError(), "matvec_batch launch");
      if (!dev && t.fits) {
        for (int b = 0; b < nbatch; ++b)
          if ((rc = copy_vectors(false, wq + (size_t)b * nv * n, yg + (int64_t)b * nvec * ldy, ldy, nv, "matvec_batch y D2H")))
            return rc;
        if ((rc = sync_stream(stream_, "matvec_batch sync"))) return rc;
      }
    }
    done += nv;
  }
  HIPCHK(hipGetLastError(), "matvec_batch launch");
  if ((rc = sync_stream(stream_, "matvec_batch sync"))) return rc;
  if (!t.fits) {
    feature_err_ = "matvec_batch: a launch has more work items for one member than a grid holds (the product is not complete)";
    return -99;
  }
  return 0;
}

// both sweeps with the members' factors on nv work vectors per member (pivot order, ld = n), through the batch's
// own paths; -20 is not this call's (the members without a factor are skipped by every kernel here as well).
// The sweeps know no member mask: a member whose vectors are all frozen rides along with zero columns.
int Engine::refine_batch_apply_factor(double* v, int nv, int64_t* launches) {
  int rc;
  if (nv < brf_blocked_min()) {
    rc = solve_batch(v, true, nv, (int64_t)S_->n, 0, true);
    if (rc == 0 || rc == kErrNotPosDef) *launches += bt_.solve_launches;
  } else {
    rc = solve_many_batch(v, true, nv, (int64_t)S_->n, 0, true);
    *launches += bsm_info_[2];
  }
  return rc == kErrNotPosDef ? 0 : rc;
}

BrfView Engine::brf_view(int nv) const {
  return BrfView{bt_.flag, bt_.nbatch, nv, d_brfds_, d_brfds_ + brf_capacity_, d_brfds_ + 2 * brf_capacity_, d_brfis_, d_brfpart_};
}

// refine_iterate on one pass: nv <= brf_rb_ vectors of every member, np = nbatch * nv pairs.  A member without a
// factor is neither copied nor permuted.  The launches of the pass and of its sweeps are added to brf_info_[2]; a
// launch that does not fit a grid makes the pass end with -99.
struct Engine::RefineBatchBackend {
  Engine& e;
  const double* dval;
  int64_t ldval;
  int nv;
  double* x;   // vector 0 of this pass of member 0
  int64_t xstride, ldx;
  bool dev;
  double tol;
  const int n = e.S_->n, nbatch = e.bt_.nbatch;
  const RfOperator op = e.refine_operator();
  const BrfView v = e.brf_view(nv);
  const hipStream_t s = e.stream_;
  const int64_t ws = (int64_t)nv * n;   // a member's stride in the work arrays
  BrfTally t;

  int fail(int code, const char* what, hipError_t err) { return e.fail(code, what, err); }
  bool ok(int b) const { return e.bt_.hflag[(size_t)b] == INT_MAX; }
  double* w(RfVec k) const { return k == RFV_NONE ? nullptr : e.d_brfwork_ + (int64_t)k * nbatch * ws; }
  const int* sel(RfSel k) const {
    return k == RFSEL_ALL ? nullptr : (k == RFSEL_ST ? v.st() : (k == RFSEL_DECL ? v.decl() : v.improve()));
  }

  int pairs() const { return v.np(); }
  int stride() const { return v.np(); }
  int vslots() const { return vec_slots(n); }
  int sslots() const { return spmv_slots(op); }
  bool fits() const { return t.fits; }
  int permute_in() {
    if (dev) {
      t.add(launch_brf_permute(s, v, false, x, xstride, ldx, e.d_order_, n, w(RFV_B)));
      return 0;
    }
    for (int b = 0; b < nbatch; ++b)
      if (int rc = ok(b) ? e.copy_vectors(true, w(RFV_Q) + b * ws, x + b * xstride, ldx, nv, "refine_batch rhs H2D") : 0)
        return rc;
    t.add(launch_brf_permute(s, v, false, w(RFV_Q), ws, n, e.d_order_, n, w(RFV_B)));
    return 0;
  }
  void dot(RfVec a, RfVec b, RfSel k, int want, bool residual_like) {
    t.add(launch_brf_dot(s, v, n, w(a), w(b), sel(k), want, residual_like));
  }
  void finalize(int stage, int nslots, int flag) { t.add(launch_brf_finalize(s, v, stage, nslots, tol, flag)); }
  void copy(RfVec dst, RfVec src, RfSel k, int want, bool zero_others) {
    t.add(launch_brf_copy(s, v, n, w(dst), w(src), sel(k), want, zero_others));
  }
  int apply_factor(RfVec k) { return e.refine_batch_apply_factor(w(k), nv, &e.brf_info_[2]); }
  void spmv(RfVec xv, RfVec b, RfVec y, RfSel k, int want, bool partials) {
    t.add(launch_bspmv(s, op, v, dval, ldval, w(xv), ws, n, w(b), w(y), ws, n, sel(k), want, partials));
  }
  void axpy(bool alpha, RfVec xv, RfVec p, RfVec r, RfVec q, RfSel k, int want, bool partials) {
    t.add(launch_brf_axpy(s, v, n, alpha ? v.alpha() : nullptr, w(xv), w(p), w(r), w(q), sel(k), want, partials));
  }
  void pupdate(RfVec p, RfVec z, RfSel k, int want) { t.add(launch_brf_pupdate(s, v, n, v.beta(), w(p), w(z), sel(k), want)); }
  // the one array that crosses the bus per iteration
  int readback(std::vector<double>& out) {
    HIPCHK(hipGetLastError(), "refine_batch launch");
    HIPCHK(hipMemcpyAsync(out.data(), v.out(), sizeof(double) * 2 * (size_t)v.np(), hipMemcpyDeviceToHost, s),
           "refine_batch state D2H");
    return e.sync_stream(s, "refine_batch sync");
  }
  int permute_out(RfVec src) {
    if (dev) {
      t.add(launch_brf_permute(s, v, true, x, xstride, ldx, e.d_order_, n, w(src)));
      return 0;
    }
    t.add(launch_brf_permute(s, v, true, w(RFV_Q), ws, n, e.d_order_, n, w(src)));
    HIPCHK(hipGetLastError(), "refine_batch launch");
    for (int b = 0; b < nbatch; ++b)
      if (int rc = ok(b) ? e.copy_vectors(false, w(RFV_Q) + b * ws, x + b * xstride, ldx, nv, "refine_batch x D2H") : 0)
        return rc;
    return 0;
  }
  int finish() {
    HIPCHK(hipGetLastError(), "refine_batch launch");
    if (int rc = e.sync_stream(s, "refine_batch sync")) return rc;
    e.brf_info_[2] += t.n;
    if (t.fits) return 0;
    if (e.feature_err_.empty())
      e.feature_err_ = "solve_refined_batch: a launch has more work items for one member than a grid holds";
    return -99;
  }
};

int Engine::solve_refined_batch(const double* val, int64_t ldval, int nrhs, double* x, int64_t ldx, bool dev, int method,
                                double tol, int max_iter, int* iterations, double* error) {
  const int n = S_->n, nbatch = bt_.nbatch;
  const int64_t nnz = S_->nnzA;
  int rc;
  if (!enter(val && x && nrhs >= 0 && ldval >= nnz && ldx >= n && method >= 0 && method <= 1 && tol > 0.0 && max_iter >= 0 &&
                 nbatch > 0,
             nrhs == 0, &rc))
    return rc;
  brf_info_[1] = brf_info_[2] = 0;
  if (n == 0) {
    for (int64_t o = 0; o < (int64_t)nbatch * nrhs; ++o) {
      if (iterations) iterations[o] = 0;
      if (error) error[o] = 0.0;
    }
    return 0;
  }
  if ((rc = prepare_refine_batch(nbatch))) return rc;
  const double* dval = val;
  int64_t ldv = ldval;
  if (!dev) {
    if ((rc = grow_batch_buffer(&d_brfval_, &brf_val_elems_, (size_t)nbatch * (size_t)std::max<int64_t>(nnz, 1), "the staged values")))
      return rc;
    for (int b = 0; b < nbatch; ++b)   // (a member without a factor: its values are not read)
      if (bt_.hflag[(size_t)b] == INT_MAX &&
          (rc = copy_vectors_to_device(d_brfval_ + (int64_t)b * nnz, val + (int64_t)b * ldval, nnz, 1, "refine_batch val H2D", nnz)))
        return rc;
    dval = d_brfval_;
    ldv = nnz;
  }
  {
    const int k = launch_brf_absmax(stream_, brf_view(1), dval, ldv, nnz);
    if (k < 0) return -99;
    brf_info_[2] = k;
  }
  int worst = 0, passes = 0;
  std::vector<int> its;
  std::vector<double> out;
  for (int done = 0; done < nrhs;) {
    const int nv = std::min(brf_rb_, nrhs - done);
    RefineBatchBackend be{*this, dval, ldv, nv, x + (int64_t)done * ldx, (int64_t)nrhs * ldx, ldx, dev, tol};
    if ((rc = refine_iterate(be, method, max_iter, its, out))) {
      brf_info_[2] = 0;   // (the counts of a call that went through)
      return rc;
    }
    const size_t np = (size_t)nbatch * (size_t)nv;
    for (int b = 0; b < nbatch; ++b)
      for (int q = 0; q < nv; ++q) {
        const size_t g = (size_t)b * nv + q, o = (size_t)b * nrhs + done + q;
        const bool ok = bt_.hflag[(size_t)b] == INT_MAX;   // (else: a member without a factor)
        if (iterations) iterations[o] = ok ? its[g] : 0;
        if (error) error[o] = ok ? out[g] : std::numeric_limits<double>::quiet_NaN();
        if (ok && out[np + g] != 1.0) worst = 1;
      }
    ++passes;
    done += nv;
  }
  brf_info_[1] = passes;
  const int failed = batch_failed();
  return failed ? failed : worst;
}

// ---- hard linear constraints C x = e ----------------------------------------------------------------------
void Engine::drop_constraints() {
  give_back(cn_.C, cn_.U, cn_.G, cn_.part, cn_.T);
  const int64_t rebuilds = cn_.rebuilds;
  cn_ = CnState{};
  cn_.rebuilds = rebuilds;
}

int Engine::release_constraints() {
  int rc;
  if (!enter_release(cn_.k > 0, "constraints release", &rc)) return rc;
  drop_constraints();
  return 0;
}

void Engine::constraints_info(int64_t out[4], double stat[2]) const {
  out[0] = cn_.k;
  out[1] = cn_.rebuilds;
  out[2] = (int64_t)cn_.bytes;
  out[3] = cn_.launches;
  stat[0] = cn_.logdet;
  stat[1] = cn_.minrel;
}

// U, G, log det S and the smallest relative pivot from the stored C and the current factor
int Engine::build_constraints(int64_t serial) {
  const int n = S_->n, k = cn_.k;
  int rc = prepare_solve_many(false);
  if (!rc && repro_on_) rc = prepare_solve_repro();
  if (rc) return rc;
  cn_.serial = -1;
  HIPCHK(hipMemcpyAsync(cn_.U, cn_.C, sizeof(double) * (size_t)k * (size_t)n, hipMemcpyDeviceToDevice, stream_), "constraints W");
  if ((rc = repro_on_ ? solve_repro_dev(cn_.U, k, (int64_t)n, 0, false) : solve_many_dev(cn_.U, k, (int64_t)n, 0, false)))
    return rc;
  double* dstat = cn_.G + kCnMaxRows * kCnMaxRows;
  launch_cn_dot(stream_, cn_.C, (int64_t)n, k, cn_.U, (int64_t)n, k, n, cn_.part, kCnMaxRows, true);
  launch_cn_chol(stream_, cn_.part, cn_nchunks(n), k, cn_.G, dstat);
  cn_.launches += 2;
  HIPCHK(hipGetLastError(), "constraints launch");
  double stat[3] = {0.0, 0.0, 0.0};
  HIPCHK(hipMemcpyAsync(stat, dstat, sizeof stat, hipMemcpyDeviceToHost, stream_), "constraints D2H");
  if ((rc = sync_stream(stream_, "constraints sync"))) return rc;
  if (stat[2] != 0.0) {
    feature_err_ = "set_constraints: row " + std::to_string((int)stat[2]) + " of C depends on the rows before it (its pivot of "
                   "S = C A^-1 C^T is <= 2^-26 S_jj or not finite): the handle holds no constraints";
    return kErrNotPosDef;
  }
  launch_cn_scale(stream_, cn_.U, (int64_t)n, n, k, cn_.G);
  ++cn_.launches;
  HIPCHK(hipGetLastError(), "constraints launch");
  if ((rc = sync_stream(stream_, "constraints sync"))) return rc;
  cn_.logdet = stat[0];
  cn_.minrel = stat[1];
  cn_.serial = serial;
  ++cn_.rebuilds;
  return 0;
}

int Engine::set_constraints(int k, const double* c, int64_t ldc, bool dev, int64_t serial) {
  if (k == 0) return release_constraints();
  const int n = S_->n;
  int rc;
  if (!enter(k > 0 && k <= kCnMaxRows && c && ldc >= n && n > 0, false, &rc)) return rc;
  if ((rc = prepare_solve_many(false))) return rc;
  if (cn_.k != k) {
    // (a failure here leaves the factor and every solve usable: the engine's status is not touched)
    drop_constraints();
    const size_t kn = sizeof(double) * (size_t)k * (size_t)n, gb = sizeof(double) * (kCnMaxRows * kCnMaxRows + 8),
                 pb = sizeof(double) * (size_t)cn_nchunks(n) * kCnMaxRows * kCnMaxRows,
                 tb = sizeof(double) * 3 * kCnPass * kCnMaxRows;
    auto t = take();
    t.block(&cn_.C, kn);
    t.block(&cn_.U, kn);
    t.block(&cn_.G, gb);
    t.block(&cn_.part, pb);
    t.block(&cn_.T, tb);
    if (!t.ok()) {
      feature_err_ = "set_constraints: not enough device memory for C, U and the partial sums (" +
                     std::to_string(t.bytes() >> 20) + " MiB): " + hipGetErrorString(t.error());
      return alloc_code(t.error());
    }
    t.commit();
    cn_.bytes = t.bytes();
    cn_.k = k;
  }
  cn_.launches = 0;
  const hipError_t e = hipMemcpy2DAsync(cn_.C, sizeof(double) * (size_t)n, c, sizeof(double) * (size_t)ldc, sizeof(double) * (size_t)n,
                                        (size_t)k, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream_);
  if (e != hipSuccess) {
    drop_constraints();
    return fail(kErrHip, "constraints C copy", e);
  }
  if ((rc = build_constraints(serial))) {
    const std::string why = feature_err_;
    if (!poisoned_) drop_constraints();
    feature_err_ = why;
  }
  return rc;
}

// one pass of nv <= kCnPass device vectors: r = C x - e, t = G^-1 r (and lambda), x -= U t (enqueue only)
int Engine::cn_pass(double* xd, int64_t ld, int nv, const double* e, int64_t lde, double* lambda, int64_t ldl) {
  const int n = S_->n, k = cn_.k;
  launch_cn_dot(stream_, cn_.C, (int64_t)n, k, xd, ld, nv, n, cn_.part, kCnPass, false);
  launch_cn_small(stream_, cn_.part, cn_nchunks(n), k, nv, cn_.G, e, lde, cn_.T, lambda, ldl);
  launch_cn_apply(stream_, xd, ld, nv, n, cn_.U, (int64_t)n, k, cn_.T);
  cn_.launches += 3;
  return 0;
}

int Engine::constrain(int op, int nvec, double* x, int64_t ldx, const double* e, int64_t lde, double* lambda, int64_t ldl,
                      bool dev, int64_t serial, uint64_t seed, uint64_t first, const double* mean) {
  const int n = S_->n, k = cn_.k;
  int rc;
  if (!enter(op >= CN_CORRECT && op <= CN_SAMPLE && nvec >= 0 && x && ldx >= n && k > 0 && (lde == 0 || lde >= k) &&
                 (!lambda || ldl >= k),
             nvec == 0 || n == 0, &rc))
    return rc;
  cn_.launches = 0;
  if (cn_.serial != serial && (rc = build_constraints(serial))) {
    const std::string why = feature_err_;
    if (!poisoned_) drop_constraints();
    feature_err_ = why;
    return rc;
  }
  if ((rc = prepare_solve_many(!dev))) return rc;
  if (op == CN_SAMPLE && repro_on_ && (rc = prepare_solve_repro())) return rc;
  double* estage = cn_.T + kCnPass * kCnMaxRows;
  double* lstage = estage + kCnPass * kCnMaxRows;
  const double* dmean = mean;
  if (mean && !dev) {
    if (!d_fmmean_) {
      auto t = take();
      t(&d_fmmean_, sizeof(double) * (size_t)n);
      if (!t.ok()) {
        feature_err_ = std::string("sample_constrained: not enough device memory for the mean: ") + hipGetErrorString(t.error());
        return alloc_code(t.error());
      }
      t.commit();
    }
    HIPCHK(hipMemcpyAsync(d_fmmean_, mean, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, stream_), "mean H2D");
    dmean = d_fmmean_;
  }
  if (e && !dev && lde == 0 && (rc = copy_vectors_to_device(estage, e, (int64_t)k, 1, "constrain e H2D", (int64_t)k))) return rc;
  rc = for_each_block(nvec, kCnPass, [&](int done, int nv, int) -> int {
    int r = 0;
    double* xd = dev ? x + (int64_t)done * ldx : d_smstage_;
    const int64_t ld = dev ? ldx : (int64_t)n;
    if (!dev && op != CN_SAMPLE && (r = copy_vectors(true, d_smstage_, x + (int64_t)done * ldx, ldx, nv, "constrain H2D"))) return r;
    if (op == CN_SOLVE) {
      if ((r = solve_many_dev(xd, nv, ld, 0, false))) return r;
    } else if (op == CN_SAMPLE) {
      launch_white_noise(stream_, xd, ld, d_order_, n, nv, seed, first + (uint64_t)done);
      if ((r = repro_on_ ? solve_repro_dev(xd, nv, ld, 2, false) : solve_many_dev(xd, nv, ld, 2, false))) return r;
      if (dmean) launch_add_mean(stream_, xd, ld, dmean, n, nv);
    }
    const double* ep = e;
    int64_t le = lde;
    if (e && dev) {
      ep = e + (int64_t)done * lde;
    } else if (e) {
      if (lde != 0 && (r = copy_vectors_to_device(estage, e + (int64_t)done * lde, lde, nv, "constrain e H2D", (int64_t)k)))
        return r;
      ep = estage;
      le = lde ? (int64_t)k : 0;
    }
    double* lp = !lambda ? nullptr : dev ? lambda + (int64_t)done * ldl : lstage;
    cn_pass(xd, ld, nv, ep, le, lp, dev ? ldl : (int64_t)k);
    if (!dev) {
      HIPCHK(hipGetLastError(), "constrain launch");
      if ((r = copy_vectors(false, d_smstage_, x + (int64_t)done * ldx, ldx, nv, "constrain D2H"))) return r;
      if (lambda && (r = copy_vectors(false, lstage, lambda + (int64_t)done * ldl, ldl, nv, "constrain lambda D2H", (int64_t)k)))
        return r;
      if ((r = sync_stream(stream_, "constrain sync"))) return r;
    }
    return 0;
  });
  if (rc) return rc;
  HIPCHK(hipGetLastError(), "constrain launch");
  return sync_stream(stream_, "constrain sync");
}

int Engine::inverse_diag_constrained(double* out, int n, int64_t serial) {
  int rc;
  if (!enter(z_valid_ && out && n == S_->n && cn_.k > 0, false, &rc)) return rc;
  cn_.launches = 0;
  if (cn_.serial != serial && (rc = build_constraints(serial))) {
    const std::string why = feature_err_;
    if (!poisoned_) drop_constraints();
    feature_err_ = why;
    return rc;
  }
  launch_selinv_diag_gather(stream_, d_Z_, d_sidiag_, d_order_, n, d_siout_);
  launch_cn_var(stream_, d_siout_, cn_.U, (int64_t)n, n, cn_.k, d_siout_);
  ++cn_.launches;
  HIPCHK(hipGetLastError(), "constrained diag launch");
  HIPCHK(hipMemcpyAsync(out, d_siout_, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, stream_), "constrained diag D2H");
  return sync_stream(stream_, "constrained diag sync");
}

// ---- hard linear constraints C x = e for the members of a batch ---------------------------------------------
namespace {
// build_constraints_batch to its callers: a dependent row (reported as -20 once the constraints are dropped), as
// opposed to the -20 of a member that is not positive definite (the constraints stay)
constexpr int kErrDependent = -2000;
}  // namespace

BcnView Engine::bcn_view() const {
  return BcnView{bt_.flag, bt_.nbatch, S_->n, bcn_.k, bcn_.C, bcn_.U, bcn_.G,
                 bcn_.G + (size_t)bcn_.capacity * kCnMaxRows * kCnMaxRows, bcn_.part, bcn_.T,
                 (int64_t)cn_nchunks(S_->n) * kCnMaxRows * kCnMaxRows};
}

void Engine::drop_constraints_batch() {
  give_back(bcn_.C, bcn_.U, bcn_.G, bcn_.part, bcn_.T);
  const int64_t rebuilds = bcn_.rebuilds;
  bcn_ = BcnState{};
  bcn_.rebuilds = rebuilds;
}

int Engine::release_constraints_batch() {
  int rc;
  if (!enter_release(bcn_.C != nullptr, "constraints_batch release", &rc)) return rc;
  drop_constraints_batch();
  return 0;
}

void Engine::constraints_batch_info(int64_t out[4], double* stat, int64_t ldstat) const {
  out[0] = bcn_.k;
  out[1] = bcn_.rebuilds;
  out[2] = (int64_t)bcn_.bytes;
  out[3] = bcn_.launches;
  if (!stat || bcn_.k <= 0) return;
  // (numbers of an old batch are never returned: NaN until the first call that rebuilds)
  const bool current = bcn_.generation == bt_.generation && bcn_.stat.size() == 2 * (size_t)bt_.nbatch;
  for (int b = 0; b < bt_.nbatch; ++b)
    for (int i = 0; i < 2; ++i)
      stat[(int64_t)b * ldstat + i] = current ? bcn_.stat[2 * (size_t)b + i] : std::numeric_limits<double>::quiet_NaN();
}

// C (kept from the storage held when keep_c), U, G and the scalars, the partials and T for `members` members: one
// transaction; a failure keeps what was held before
int Engine::take_constraints_batch(int k, int members, bool keep_c) {
  const size_t n = (size_t)S_->n, m = (size_t)members;
  const size_t kn = sizeof(double) * (size_t)k * n;
  BcnState fresh;
  {
    auto t = take();
    t.block(&fresh.C, kn);
    t.block(&fresh.U, kn * m);
    t.block(&fresh.G, sizeof(double) * m * (kCnMaxRows * kCnMaxRows + kBcnStat));
    t.block(&fresh.part, sizeof(double) * m * (size_t)cn_nchunks(S_->n) * kCnMaxRows * kCnMaxRows);
    t.block(&fresh.T, sizeof(double) * m * 3 * kCnPass * kCnMaxRows);
    if (t.ok() && keep_c) {
      t.check(hipMemcpyAsync(fresh.C, bcn_.C, kn, hipMemcpyDeviceToDevice, stream_));
      if (t.ok()) t.check(hipStreamSynchronize(stream_));
    }
    if (!t.ok()) {
      feature_err_ = "set_constraints_batch: not enough device memory for C, U and the partial sums of " +
                     std::to_string(members) + " members (" + std::to_string(t.bytes() >> 20) +
                     " MiB): " + hipGetErrorString(t.error());
      return alloc_code(t.error());
    }
    t.commit();
    fresh.bytes = t.bytes();
  }
  fresh.rebuilds = bcn_.rebuilds;
  fresh.launches = bcn_.launches;
  drop_constraints_batch();
  bcn_ = fresh;
  bcn_.k = k;
  bcn_.capacity = members;
  return 0;
}

// U_b, G_b, log det S_b and the smallest relative pivot of every factorized member from the stored C: the copy of C
// into every member's slot, the blocked batch solve, three launches.  0, -20 with the constraints still held (a
// member is not positive definite: the others are built), or an error after which the caller drops the constraints.
int Engine::build_constraints_batch() {
  const int n = S_->n, k = bcn_.k, nbatch = bt_.nbatch;
  bcn_.generation = -1;
  const BcnView v = bcn_view();
  bool fits = launch_bcn_bcast(stream_, v) >= 0;
  HIPCHK(hipGetLastError(), "constraints_batch launch");
  int rc = fits ? solve_many_batch(bcn_.U, true, k, (int64_t)n, 0, false) : 0;
  if (rc && rc != kErrNotPosDef) return rc;
  int nl = 0;
  auto count = [&](int l) { if (l < 0) fits = false; else nl += l; };
  if (fits) count(launch_bcn_dot(stream_, v, bcn_.U, (int64_t)k * n, (int64_t)n, k, kCnMaxRows, true));
  if (fits) count(launch_bcn_chol(stream_, v));
  if (fits) count(launch_bcn_scale(stream_, v));
  bcn_.launches += nl;
  HIPCHK(hipGetLastError(), "constraints_batch launch");
  std::vector<double> stat((size_t)nbatch * kBcnStat, 0.0);
  HIPCHK(hipMemcpyAsync(stat.data(), v.stat, sizeof(double) * stat.size(), hipMemcpyDeviceToHost, stream_),
         "constraints_batch D2H");
  if ((rc = sync_stream(stream_, "constraints_batch sync"))) return rc;
  if (!fits) {
    feature_err_ = "set_constraints_batch: the batch has more members than a grid dimension holds";
    return -99;
  }
  // (U_b of a member with a dependent row was scaled by a G_b that is not a factor: the caller drops everything)
  bcn_.stat.assign(2 * (size_t)nbatch, std::numeric_limits<double>::quiet_NaN());
  for (int b = 0; b < nbatch; ++b) {
    if (bt_.hflag[(size_t)b] != INT_MAX) continue;   // (nothing of it was written: the scalars are not read)
    const double* sb = &stat[(size_t)b * kBcnStat];
    if (sb[2] != 0.0) {
      feature_err_ = "set_constraints_batch: member " + std::to_string(b) + ", row " + std::to_string((int)sb[2]) +
                     " of C depends on the rows before it (its pivot of S_b = C A_b^-1 C^T is <= 2^-26 S_jj or not "
                     "finite): the batch holds no constraints";
      return kErrDependent;
    }
    bcn_.stat[2 * (size_t)b] = sb[0];
    bcn_.stat[2 * (size_t)b + 1] = sb[1];
  }
  bcn_.generation = bt_.generation;
  ++bcn_.rebuilds;
  return batch_failed();
}

// before a call that needs U_b: the storage for the members of the current batch and their numbers
int Engine::refresh_constraints_batch() {
  if (bcn_.generation == bt_.generation && bt_.nbatch <= bcn_.capacity) return 0;
  int rc = 0;
  if (bt_.nbatch > bcn_.capacity) rc = take_constraints_batch(bcn_.k, bt_.nbatch, true);
  if (!rc) rc = build_constraints_batch();
  if (rc == kErrDependent || (rc && rc != kErrNotPosDef)) {
    const std::string why = feature_err_;
    if (!poisoned_) drop_constraints_batch();
    feature_err_ = why;
    return rc == kErrDependent ? kErrNotPosDef : rc;
  }
  return 0;   // (-20 of a member that is not positive definite: the caller reports it after serving the others)
}

int Engine::set_constraints_batch(int k, const double* c, int64_t ldc, bool dev) {
  if (k == 0) return release_constraints_batch();
  const int n = S_->n, nbatch = bt_.nbatch;
  int rc;
  if (!enter(k > 0 && k <= kCnMaxRows && c && ldc >= n && n > 0 && nbatch > 0, false, &rc)) return rc;
  // (a failure here leaves the batch and every other call usable: the engine's status is not touched)
  if ((bcn_.k != k || nbatch > bcn_.capacity) && (rc = take_constraints_batch(k, nbatch, false))) {
    const std::string why = feature_err_;
    drop_constraints_batch();
    feature_err_ = why;
    return rc;
  }
  bcn_.launches = 0;
  const hipError_t e = hipMemcpy2DAsync(bcn_.C, sizeof(double) * (size_t)n, c, sizeof(double) * (size_t)ldc,
                                        sizeof(double) * (size_t)n, (size_t)k,
                                        dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream_);
  if (e != hipSuccess) {
    drop_constraints_batch();
    return fail(kErrHip, "constraints_batch C copy", e);
  }
  rc = build_constraints_batch();
  if (rc && rc != kErrNotPosDef) {
    const std::string why = feature_err_;
    if (!poisoned_) drop_constraints_batch();
    feature_err_ = why;
    return rc == kErrDependent ? kErrNotPosDef : rc;
  }
  return rc;
}

int Engine::bcn_pass(double* xd, int64_t xs, int64_t ld, int nv, const double* e, int64_t es, int64_t lde, double* lambda,
                     int64_t ls, int64_t ldl) {
  const BcnView v = bcn_view();
  int nl = 0;
  for (int l : {launch_bcn_dot(stream_, v, xd, xs, ld, nv, kCnPass, false),
                launch_bcn_small(stream_, v, nv, e, es, lde, lambda, ls, ldl), launch_bcn_apply(stream_, v, xd, xs, ld, nv)}) {
    if (l < 0) return -1;
    nl += l;
  }
  return nl;
}

int Engine::constrain_batch(int op, int nvec, double* x, int64_t ldx, const double* e, int64_t lde, double* lambda,
                            int64_t ldl, bool dev, uint64_t seed, uint64_t first, uint32_t stream0, int stream_step,
                            const double* mean, int64_t ldmean) {
  const int n = S_->n, k = bcn_.k, nbatch = bt_.nbatch;
  int rc;
  if (!enter(op >= CN_CORRECT && op <= CN_SAMPLE && nvec >= 0 && x && ldx >= n && k > 0 && nbatch > 0 &&
                 (lde == 0 || lde >= k) && (!lambda || ldl >= k) && stream_step >= 0 && stream_step <= 1 &&
                 !(mean && ldmean != 0 && ldmean < n),
             nvec == 0 || n == 0, &rc))
    return rc;
  bcn_.launches = 0;
  if ((rc = refresh_constraints_batch())) return rc;
  if (op == CN_SOLVE && (rc = prepare_solve_many_batch())) return rc;
  const int cap = std::min(nvec, kCnPass);
  if (!dev && (rc = grow_batch_buffer(&bt_.stage, &bt_.stage_elems, (size_t)nbatch * (size_t)cap * (size_t)n,
                                      "the staged vectors")))
    return rc;
  // the mean of a host entry point, as sample_batch keeps it
  const double* dmean = mean;
  int64_t ldm = ldmean;
  if (op == CN_SAMPLE && mean && !dev) {
    const size_t nm = ldmean == 0 ? 1 : (size_t)nbatch;
    if ((rc = grow_batch_buffer(&d_bmmean_, &bm_mean_elems_, nm * (size_t)n, "the means"))) return rc;
    if ((rc = copy_vectors_to_device(d_bmmean_, mean, ldmean, (int64_t)nm, "mean H2D"))) return rc;
    dmean = d_bmmean_;
    ldm = ldmean == 0 ? 0 : n;
  }
  // device vectors: the samples of the whole call first (sample_batch lays member b's at x + b nsamp ldx)
  if (op == CN_SAMPLE && dev) {
    rc = sample_batch(x, nvec, ldx, 0, seed, first, stream0, stream_step, dmean, ldm, true);
    if (rc && rc != kErrNotPosDef) return rc;
  }
  double* estage = bcn_.T + (size_t)bcn_.capacity * kCnPass * kCnMaxRows;
  double* lstage = estage + (size_t)bcn_.capacity * kCnPass * kCnMaxRows;
  if (e && !dev && lde == 0 && (rc = copy_vectors_to_device(estage, e, (int64_t)k, 1, "constrain_batch e H2D", (int64_t)k)))
    return rc;
  bool fits = true;
  rc = walk_blocks({"constrain_batch", x, dev, nvec, ldx, nbatch, bt_.stage, kCnPass, false, op != CN_SAMPLE},
                   [&](int done, double* xd, int64_t xs, int64_t ld, int nv, int, bool) -> int {
                     int r = 0;
                     if (op == CN_SOLVE) {
                       // (blocks of the width the workspace of the blocked solve holds)
                       r = for_each_block(nv, bsm_rb_, [&](int at, int cur, int rb) {
                         return std::min(enqueue_solve_many_batch_block(xd + (int64_t)at * ld, xs, ld, cur, rb, 0, false), 0);
                       });
                       if (r) { fits = false; return -1; }
                     } else if (op == CN_SAMPLE && !dev) {
                       r = sample_batch(xd, nv, ld, 0, seed, first + (uint64_t)done, stream0, stream_step, dmean, ldm, true);
                       if (r && r != kErrNotPosDef) return r;
                     }
                     const double* ep = e;
                     int64_t es = lde == 0 ? 0 : (int64_t)nvec * lde, le = lde;
                     double* lp = lambda;
                     int64_t ls = (int64_t)nvec * ldl, ll = ldl;
                     if (dev) {
                       if (e) ep = e + (int64_t)done * lde;
                       if (lambda) lp = lambda + (int64_t)done * ldl;
                     } else {
                       if (e && lde != 0) {
                         for (int b = 0; b < nbatch; ++b)
                           if ((r = copy_vectors_to_device(estage + (int64_t)b * nv * k, e + ((int64_t)b * nvec + done) * lde, lde,
                                                           nv, "constrain_batch e H2D", (int64_t)k)))
                             return r;
                         es = (int64_t)nv * k;
                         le = k;
                       }
                       if (e) ep = estage;
                       if (lambda) {
                         lp = lstage;
                         ls = (int64_t)nv * k;
                         ll = k;
                       }
                     }
                     const int nl = bcn_pass(xd, xs, ld, nv, ep, es, le, lp, ls, ll);
                     if (nl < 0) { fits = false; return -1; }
                     bcn_.launches += nl;
                     if (!dev && lambda)
                       for (int b = 0; b < nbatch; ++b) {
                         if (bt_.hflag[(size_t)b] != INT_MAX) continue;   // (NaN below: nothing was written for it)
                         if ((r = copy_vectors(false, lstage + (int64_t)b * nv * k, lambda + ((int64_t)b * nvec + done) * ldl, ldl,
                                               nv, "constrain_batch lambda D2H", (int64_t)k)))
                           return r;
                       }
                     return 0;
                   });
  if (!fits) {
    feature_err_ = "constrain_batch: a launch has more work items for one member than a grid holds (the vectors are not "
                   "all served)";
    return -99;
  }
  if (rc) return rc;
  // a member that is not positive definite: its multipliers are NaN (its vectors stay as they were; its samples are
  // the NaN of sample_batch)
  if (lambda) {
    for (int b = 0; b < nbatch; ++b) {
      if (bt_.hflag[(size_t)b] == INT_MAX) continue;
      if (!dev) {
        for (int q = 0; q < nvec; ++q)
          std::fill_n(lambda + ((int64_t)b * nvec + q) * ldl, k, std::numeric_limits<double>::quiet_NaN());
      } else {
        const std::vector<double> nan((size_t)k * (size_t)nvec, std::numeric_limits<double>::quiet_NaN());
        HIPCHK(hipMemcpy2D(lambda + (int64_t)b * nvec * ldl, sizeof(double) * (size_t)ldl, nan.data(),
                           sizeof(double) * (size_t)k, sizeof(double) * (size_t)k, (size_t)nvec, hipMemcpyHostToDevice),
               "constrain_batch lambda NaN");
      }
    }
  }
  return batch_failed();
}

int Engine::inverse_diag_constrained_batch(double* out, int64_t ldout) {
  const int n = S_->n, nbatch = bt_.nbatch;
  int rc;
  if (!enter(bt_.z_valid && out && ldout >= n && nbatch > 0 && bcn_.k > 0, n == 0, &rc)) return rc;
  bcn_.launches = 0;
  if ((rc = refresh_constraints_batch())) return rc;
  if ((rc = grow_batch_buffer(&bt_.stage, &bt_.stage_elems, (size_t)nbatch * (size_t)n, "the gathered diagonals"))) return rc;
  // (the gather leaves NaN in the row of a member that is not positive definite; the kernel below skips that row)
  if (launch_batch_selinv_diag_gather(stream_, batch_selinv_view(), bt_.diag, d_order_, n, bt_.stage, n) < 0 ||
      launch_bcn_var(stream_, bcn_view(), bt_.stage, (int64_t)n, bt_.stage) < 0) {
    feature_err_ = "constrained batch diagonal: one member's entries are more work items than a grid holds";
    return -99;
  }
  ++bcn_.launches;
  HIPCHK(hipGetLastError(), "constrained batch diag launch");
  if ((rc = copy_vectors(false, bt_.stage, out, ldout, nbatch, "constrained batch diag D2H"))) return rc;
  if ((rc = sync_stream(stream_, "constrained batch diag sync"))) return rc;
  return batch_failed();
}

}  // namespace spx
