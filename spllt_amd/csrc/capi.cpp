// extern "C" boundary of libspllt_hip.so: the SpLLT C-ABI (include/spllt_iface.h)
// plus the extensions of include/spllt_hip.h.  Mirrors the behaviour of
// reference interfaces/C/spllt_data_ciface.F90: never aborts, messages on
// stderr, status in info->flag.
//
// Every extension that works on a handle goes through one ladder, enter(), whose order is fixed: every check
// that needs no device comes first, so a rejected call touches nothing.
//   1. handle and analysis      SPLLT_ERROR_PARAMETER, no message
//   2. the caller's own argument check (`bad`; "" refuses without a message)
//   3. partition                SPLLT_ERROR_UNIMPLEMENTED and a line on stderr (SINGLE, SINGLE_F)
//   4. dead                     SPLLT_ERROR_HIP: a submission of this handle never returned
//   5. wait                     for a pending factorization (WAIT returns its failure, WAIT_IGNORE does not)
//   6. engine                   created when there is none (ENGINE); its failure with its message
//   7. factor, batch or inverse SPLLT_ERROR_PARAMETER with a message saying what is missing
// ensure_engine() is the only place that constructs an Engine, leave() the one way out after the engine call.
#include <algorithm>
#include <cassert>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "engine.hpp"
#include "kernels.hpp"
#include "spllt_hip.h"
#include "spllt_hip_batch_mult.h"
#include "spllt_hip_batch_adjoint.h"
#include "spllt_hip_batch_solve_many.h"
#include "spllt_hip_batch_refine.h"
#include "spllt_hip_batch_repro.h"
#include "spllt_hip_constrain.h"
#include "spllt_hip_constrain_batch.h"
#include "spllt_hip_solve_sparse_batch.h"
#include "spllt_hip_updown_batch.h"
#include "symbolic.hpp"

using namespace spx;

namespace {

// a table of spllt_hip_program_get: rebuilt when the handle has been analysed again or the key differs
template <class T>
struct Cached {
  std::shared_ptr<const Symbolic> S;
  int key[2] = {-1, -1};
  int rc = 0;
  T value;
  template <class Build>
  const T* get(const std::shared_ptr<Symbolic>& s, int k0, int k1, Build build) {   // null: the build failed
    if (S != s || key[0] != k0 || key[1] != k1) {
      rc = build(value);
      S = s;
      key[0] = k0;
      key[1] = k1;
    }
    return rc ? nullptr : &value;
  }
};
struct MatvecTables {
  std::vector<int64_t> rowptr;
  std::vector<int> col, src;
};
struct PatternTables {
  std::vector<int> row, col;
};

struct Akeep {
  std::shared_ptr<Symbolic> S;
  SymOptions so;
};

struct Fkeep {
  std::shared_ptr<Symbolic> S;
  std::unique_ptr<Engine> eng;
  EngineOptions eo;
  std::vector<double> hostL;
  bool hostL_valid = false;
  int last_flag = 0;
  std::string last_error;
  // solve memory handed over by spllt_set_mem_solve (borrowed, unused by the host solve)
  double* y = nullptr;
  double* workspace = nullptr;
  long worksize = 0;
  double* xbuf = nullptr;  // multi-GPU exchange buffer (caller-owned device memory)
  bool dead = false;       // a submission never returned: the engine belongs to the stuck helper thread
  bool repro_solve = false;   // spllt_hip_set_reproducible_solve: handed to the engine before every solve
  bool batch_blocked = false;   // spllt_hip_set_batch_blocked_solve: handed to the engine before every sample_batch
  bool batch_repro = false;     // spllt_hip_set_batch_reproducible: handed to the engine by the setter and at its creation
  // what spllt_hip_program_get builds from the analysis alone, each once per pattern (and key):
  Cached<SelinvProgram> si;    // the selected-inversion program, keyed by panel width and chain block
  Cached<SelinvProgram> bsi;   // ... and the batch's (panel width 64 whatever the handle's)
  Cached<Program> bt;          // the batch program
  Cached<Program> btd;         // ... and its deterministic form ("batch_det_*")
  Cached<RsolveTables> brs;    // the tables of the batch's reproducible sweep ("batch_rsolve_*")
  Cached<MatvecTables> mv;     // the operator tables ("matvec_*")
  Cached<PatternTables> po;    // the (row, column) tables ("pattern_row" / "pattern_col")
  // spllt_hip_factor_serial: successful changes of the single factor [0] and of the batch [1]
  int64_t serial[2] = {0, 0};
};

std::mutex g_mu;
std::vector<Fkeep*> g_pending;  // factorizations submitted and not yet waited for

void clear_info(spllt_inform_t* info) {
  if (!info) return;
  std::memset(info, 0, sizeof(*info));
}

void fill_info(const Symbolic& S, spllt_inform_t* info) {
  if (!info) return;
  info->maxdepth = S.maxdepth;
  info->num_factor = (int)S.nnzL;  // truncated like the reference (ciface:77-78)
  info->num_flops = (int)S.flops;
  info->num_nodes = S.nnodes;
  info->stat = 0;
}

int do_wait(Fkeep* f) {
  if (f->dead) return SPLLT_ERROR_HIP;    // (its engine belongs to a submission that never returned)
  if (!f->eng) return f->last_flag;
  if (f->eng->pending()) {
    int rc = f->eng->wait();
    f->last_flag = rc;
    f->hostL_valid = false;
    if (rc == SPLLT_ERROR_NOT_POSDEF) {
      char buf[160];
      if (f->eng->not_posdef_column() < 0)
        std::snprintf(buf, sizeof buf, "matrix is not positive definite (reported by another rank of the partition)");
      else
        std::snprintf(buf, sizeof buf, "matrix is not positive definite (pivot column %d in elimination order)",
                      f->eng->not_posdef_column() + 1);
      f->last_error = buf;
      std::fprintf(stderr, "spllt-hip: %s\n", buf);
    } else if (rc) {
      f->last_error = f->eng->error();
    }
  }
  return f->last_flag;
}

// nothing factorized yet, or a failed downdate left the factor invalid (spllt_hip_updown)
bool no_factor(const Fkeep* f) { return !f->eng || !f->eng->factor_valid(); }

bool analysed(const Fkeep* f) { return f && f->S; }

void mark_pending(Fkeep* f) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (std::find(g_pending.begin(), g_pending.end(), f) == g_pending.end()) g_pending.push_back(f);
}

// a refusal with its message
int fail(Fkeep* f, const char* what, const std::string& msg, int rc = SPLLT_ERROR_PARAMETER) {
  f->last_error = std::string(what) + ": " + msg;
  return rc;
}

// the one way out after an engine call; the message of a failed one: the feature's own, else the engine's
int leave(Fkeep* f, int rc) {
  if (!rc) return 0;
  if (!f->eng->feature_error().empty()) f->last_error = f->eng->feature_error();
  else if (f->eng->status()) f->last_error = f->eng->error();
  return rc;
}

// the handle's engine, created when there is none: 0, SPLLT_ERROR_ALLOCATION, or the engine's status with its
// message in last_error (message = false: on the helper thread of factor_impl, which must not write the handle's
// strings -- after a deadline the caller owns them)
int ensure_engine(Fkeep* f, bool message = true) {
  if (!f->eng) {
    f->eng.reset(new (std::nothrow) Engine(f->S, f->eo));
    if (!f->eng) return SPLLT_ERROR_ALLOCATION;
    f->eng->set_exchange_buffer(f->xbuf);
    f->eng->set_batch_reproducible(f->batch_repro);   // (an engine that exists hears of the switch from its setter)
  }
  if (message && f->eng->status()) f->last_error = f->eng->error();
  return f->eng->status();
}

// what a call needs of its handle (the ladder at the top of the file)
enum Need : unsigned {
  SINGLE = 1u << 0,            // a single GPU: "... on a partitioned (multi-GPU) handle"
  SINGLE_F = 1u << 1,          // the same in the words of the older calls: "... on a partitioned (multi-GPU) factor"
  WAIT = 1u << 2,              // wait for a pending factorization and return its failure
  WAIT_IGNORE = 1u << 3,       // wait, whatever it reports (it shares the stream and the staging buffers)
  WAIT_NOT_POSDEF = 1u << 4,   // release() only: "not positive definite" is no reason not to release
  ENGINE = 1u << 5,            // create the engine
  FACTOR = 1u << 6,            // an engine whose factor no failed downdate has destroyed (the older calls: when
                               // nothing was factorized on it, the engine itself says so)
  FACTORED = 1u << 7,          // ... on which a factorization has been enqueued
  BATCH = 1u << 8,             // a batch
  INVERSE = 1u << 9,           // a selected inverse of the current factor
  BATCH_INVERSE = 1u << 10,    // a selected inverse of the current batch
  EMPTY = 1u << 11,            // the call has nothing to do: kEmpty once the checks that need no device are through
  EMPTY_FIRST = 1u << 12,      // ... even on a dead handle (spllt_hip_factor_batch)
  LENIENT = 1u << 13,          // release() only
};
// what enter() returns for EMPTY: no flag of the library; the caller hands its result on through done()
constexpr int kEmpty = INT_MAX;
int done(int rc) { return rc == kEmpty ? 0 : rc; }

// what == nullptr: the plain calls, which refuse without messages (and never ask for SINGLE: that refusal has one)
int enter(Fkeep* f, const char* what, const char* bad, unsigned need) {
  auto refuse = [&](const std::string& msg) { return what ? fail(f, what, msg) : SPLLT_ERROR_PARAMETER; };
  assert(what || !(need & (SINGLE | SINGLE_F)));
  if (!analysed(f)) return SPLLT_ERROR_PARAMETER;
  if (bad) return *bad ? refuse(bad) : SPLLT_ERROR_PARAMETER;
  if ((need & (SINGLE | SINGLE_F)) && f->eo.nranks > 1) {
    fail(f, what, std::string("not available on a partitioned (multi-GPU) ") + ((need & SINGLE_F) ? "factor" : "handle"));
    std::fprintf(stderr, "spllt-hip: %s\n", f->last_error.c_str());
    return SPLLT_ERROR_UNIMPLEMENTED;
  }
  if (need & EMPTY_FIRST) return kEmpty;
  if (f->dead) return SPLLT_ERROR_HIP;
  if (need & EMPTY) return kEmpty;
  if (need & (WAIT | WAIT_IGNORE)) {
    const int rc = do_wait(f);
    if (rc && (need & WAIT)) return rc;
  }
  if (need & ENGINE)
    if (int rc = ensure_engine(f)) return rc;
  if ((need & (FACTOR | FACTORED)) && (no_factor(f) || ((need & FACTORED) && !f->eng->factored())))
    return refuse("nothing has been factorized on this handle");
  if ((need & BATCH) && (!f->eng || f->eng->batch_count() <= 0)) return refuse("no batch has been factorized on this handle");
  if ((need & INVERSE) && !f->eng->inverse_valid())
    return refuse("no selected inverse of the current factor (call spllt_hip_selected_inverse after every factorization)");
  if ((need & BATCH_INVERSE) && !f->eng->batch_inverse_valid())
    return refuse("no selected inverse of the current batch (call spllt_hip_selected_inverse_batch after every "
                  "spllt_hip_factor_batch)");
  return 0;
}

// the SSIDS-style quintuple of spllt_hip_analyse_symbolic (1-based, as SSIDS delivers it)
struct SymbolicIn {
  int nnodes;
  const int* sptr;
  const int* sparent;
  const int64_t* rptr;
  const int* rlist;
};

void analyse_impl(void** akeep, void** fkeep, spllt_options_t* options, int n, const int* ptr,
                  const int* row, spllt_inform_t* info, int* order, const int* order_in,
                  const SymbolicIn* sym = nullptr) {
  clear_info(info);
  if (!akeep || !fkeep || !options || !ptr || !row || n < 0) {
    std::fprintf(stderr, "spllt-hip: spllt_analyse: invalid argument\n");
    if (info) info->flag = SPLLT_ERROR_PARAMETER;
    return;
  }
  if (options->nb > 1024) {
    // the substitution kernels keep one block column's worth of the right-hand side in LDS
    std::fprintf(stderr, "spllt-hip: spllt_analyse: nb = %d is not supported (nb <= 1024)\n", options->nb);
    if (info) info->flag = SPLLT_ERROR_UNIMPLEMENTED;
    return;
  }
  Akeep* a = static_cast<Akeep*>(*akeep);
  Fkeep* f = static_cast<Fkeep*>(*fkeep);
  if (!a) { a = new (std::nothrow) Akeep(); *akeep = a; }
  if (!f) {
    f = new (std::nothrow) Fkeep();
    *fkeep = f;
    // experiment knob: default chain block of every new handle (spllt_hip_set_chain_block overrides)
    if (f)
      if (const char* e = std::getenv("SPLLT_CHAIN_BLOCK")) f->eo.cb = std::max(1, std::atoi(e));
  }
  if (!a || !f) { if (info) info->flag = SPLLT_ERROR_ALLOCATION; return; }
  a->so.nb = options->nb;
  a->so.nemin = options->nemin;
  a->so.prune_tree = options->prune_tree != 0;
  a->so.ncpu = options->ncpu;
  if (const char* e = std::getenv("SPLLT_HIP_RELAX")) a->so.relax = std::atof(e);  // experiment knob
  // The reference hands ptr/row to SSIDS unchecked (ssids_analyse(check = .false.),
  // src/spllt_analyse_mod.F90:129): a malformed pattern is undefined behaviour there.
  // Here it is a parameter error: column pointers must start at 1 and not decrease,
  // rows must lie in the lower triangle (col <= row <= n) without duplicates.
  {
    bool ok = ptr[0] == 1;
    for (int j = 0; ok && j < n; ++j) ok = ptr[j + 1] >= ptr[j];
    std::vector<int> mark(ok ? (size_t)n : 0, -1);
    for (int j = 0; ok && j < n; ++j)
      for (int64_t e = (int64_t)ptr[j] - 1; ok && e < (int64_t)ptr[j + 1] - 1; ++e) {
        const int r = row[e] - 1;
        ok = r >= j && r < n && mark[r] != j;
        if (ok) mark[r] = j;
      }
    if (!ok) {
      std::fprintf(stderr, "spllt-hip: spllt_analyse: ptr/row is not a valid lower-triangular CSC pattern\n");
      if (info) info->flag = SPLLT_ERROR_PARAMETER;
      return;
    }
  }
  // 1-based int CSC -> 0-based
  std::vector<int64_t> p0((size_t)n + 1);
  for (int j = 0; j <= n; ++j) p0[j] = (int64_t)ptr[j] - 1;
  const int64_t nz = n > 0 ? p0[n] : 0;
  std::vector<int> r0((size_t)std::max<int64_t>(1, nz));
  for (int64_t e = 0; e < nz; ++e) r0[e] = row[e] - 1;
  std::vector<int> uo;
  if (order_in) {
    uo.resize(n);
    for (int i = 0; i < n; ++i) uo[i] = order_in[i] - 1;
  }
  auto S = std::make_shared<Symbolic>();
  int rc;
  try {
    if (sym) {
      // 1-based -> 0-based; the virtual root nnodes+1 becomes nnodes
      const int nn = sym->nnodes;
      if (nn < 1 || !order_in || !sym->sptr || !sym->sparent || !sym->rptr || !sym->rlist || sym->rptr[0] != 1 ||
          sym->rptr[nn] < 1) {
        rc = SPLLT_ERROR_PARAMETER;
      } else {
        std::vector<int> sp(nn + 1), spar(nn), rl((size_t)(sym->rptr[nn] - 1));
        std::vector<int64_t> rp(nn + 1);
        for (int s = 0; s <= nn; ++s) { sp[s] = sym->sptr[s] - 1; rp[s] = sym->rptr[s] - 1; }
        for (int s = 0; s < nn; ++s) spar[s] = sym->sparent[s] - 1;
        for (size_t k = 0; k < rl.size(); ++k) rl[k] = sym->rlist[k] - 1;
        rc = analyse_symbolic(n, p0.data(), r0.data(), nn, sp.data(), spar.data(), rp.data(), rl.data(),
                              uo.data(), a->so, *S);
      }
    } else {
      rc = analyse(n, p0.data(), r0.data(), order_in ? uo.data() : nullptr, a->so, *S);
    }
  } catch (const std::bad_alloc&) {
    rc = SPLLT_ERROR_ALLOCATION;
  }
  if (rc) {
    std::fprintf(stderr, "spllt-hip: spllt_analyse failed with flag %d\n", rc);
    if (info) info->flag = rc;
    return;
  }
  a->S = S;
  f->S = S;
  f->eng.reset();
  f->hostL_valid = false;
  f->last_flag = 0;
  if (order)
    for (int i = 0; i < n; ++i) order[i] = S->order[i] + 1;
  fill_info(*S, info);
}

void factor_impl(void* akeep, void* fkeep, int nnz, const double* val, bool dev, spllt_inform_t* info) {
  clear_info(info);
  Akeep* a = static_cast<Akeep*>(akeep);
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!a || !f || !f->S || !val) {
    std::fprintf(stderr, "spllt-hip: spllt_factor: akeep/fkeep/val provided by the user is empty\n");
    if (info) info->flag = SPLLT_ERROR_PARAMETER;
    return;
  }
  if ((int64_t)nnz != f->S->nnzA) {
    std::fprintf(stderr, "spllt-hip: spllt_factor: nnz = %d does not match the analysed pattern (%lld)\n", nnz,
                 (long long)f->S->nnzA);
    if (info) info->flag = SPLLT_ERROR_PARAMETER;
    return;
  }
  if (f->dead) {          // an earlier submission of this handle never returned (below)
    if (info) info->flag = SPLLT_ERROR_HIP;
    return;
  }
  if (f->eng && f->eng->pending()) do_wait(f);
  // engine creation and submission on the helper thread, under the deadline (engine.cpp)
  std::string why;
  int rc = run_with_deadline([f, dev, val, nnz]() -> int {
    if (int erc = ensure_engine(f, false)) return erc;   // (the message is copied below, on this thread)
    return dev ? f->eng->factor_async_dev(val, nnz) : f->eng->factor_async(val, nnz);
  }, &why);
  if (!why.empty()) {
    // the helper thread may still be inside the engine: the handle is dead, its engine is never
    // touched again (spllt_deallocate_fkeep leaks it)
    f->dead = true;
    f->last_flag = SPLLT_ERROR_HIP;
    f->last_error = why;
    if (info) info->flag = SPLLT_ERROR_HIP;
    return;
  }
  if (rc == SPLLT_ERROR_ALLOCATION && !f->eng) { if (info) info->flag = rc; return; }
  f->last_flag = rc;
  f->hostL_valid = false;
  if (rc == 0) {
    ++f->serial[0];
    mark_pending(f);
  } else {
    f->last_error = f->eng->error();
  }
  fill_info(*f->S, info);
  if (info) info->flag = rc;
}

// the one way out of the getters: what fits of the data into buf (when there is one), the full size returned
struct Out {
  void* buf;
  int64_t cap;   // in the unit of the size returned
  int64_t copy(const void* p, int64_t count, size_t unit) const {
    const int64_t k = std::min(cap, count);
    if (buf && k > 0) std::memcpy(buf, p, unit * (size_t)k);
    return count;
  }
  template <class Tp> int64_t elems(const std::vector<Tp>& v) const { return copy(v.data(), (int64_t)v.size(), sizeof(Tp)); }
  template <class Tp> int64_t bytes(const std::vector<Tp>& v) const { return bytes(v.data(), v.size() * sizeof(Tp)); }
  int64_t bytes(const void* p, size_t n) const { return copy(p, (int64_t)n, 1); }
};

}  // namespace

extern "C" {

void spllt_analyse(void** akeep, void** fkeep, spllt_options_t* options, int n, int* ptr, int* row,
                   spllt_inform_t* info, int* order) {
  analyse_impl(akeep, fkeep, options, n, ptr, row, info, order, nullptr);
}

void spllt_hip_analyse_ordered(void** akeep, void** fkeep, spllt_options_t* options, int n,
                               const int* ptr, const int* row, spllt_inform_t* info, int* order,
                               const int* order_in) {
  analyse_impl(akeep, fkeep, options, n, ptr, row, info, order, order_in);
}

void spllt_hip_analyse_symbolic(void** akeep, void** fkeep, spllt_options_t* options, int n,
                                const int* ptr, const int* row, spllt_inform_t* info, int nnodes,
                                const int* sptr, const int* sparent, const int64_t* rptr,
                                const int* rlist, const int* order_in) {
  SymbolicIn sym{nnodes, sptr, sparent, rptr, rlist};
  std::vector<int> order_out((size_t)std::max(n, 1));
  analyse_impl(akeep, fkeep, options, n, ptr, row, info, order_out.data(), order_in, &sym);
}

void spllt_factor(void* akeep, void* fkeep, spllt_options_t* options, int nnz, double* val,
                  spllt_inform_t* info) {
  (void)options;
  factor_impl(akeep, fkeep, nnz, val, false, info);
}

void spllt_hip_factor_dev(void* akeep, void* fkeep, spllt_options_t* options, int nnz,
                          const double* val_dev, spllt_inform_t* info) {
  (void)options;
  factor_impl(akeep, fkeep, nnz, val_dev, true, info);
}

void spllt_wait(void) {
  std::vector<Fkeep*> todo;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    todo.swap(g_pending);
  }
  for (Fkeep* f : todo) do_wait(f);
}

int spllt_hip_wait(void* fkeep) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!f) return SPLLT_ERROR_PARAMETER;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    g_pending.erase(std::remove(g_pending.begin(), g_pending.end(), f), g_pending.end());
  }
  return do_wait(f);
}

void spllt_solve_workspace_size(void* fkeep, int nworker, int nrhs, long* size) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!size) return;
  *size = 0;
  if (!f || !f->S) return;
  if (nworker < 1) nworker = 1;
  // reference formula, src/spllt_data_mod.F90:655
  *size = (long)f->S->n * nrhs + ((long)f->S->maxmn + f->S->n) * nrhs * nworker;
}

void spllt_prepare_solve(void* akeep, void* fkeep, int nb, int nrhs, long* worksize,
                         spllt_inform_t* info) {
  (void)akeep; (void)nb;
  clear_info(info);
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!f || !f->S) {
    std::fprintf(stderr, "spllt-hip: Error, fkeep provided by the user is empty\n");
    if (info) info->flag = SPLLT_ERROR_PARAMETER;
    return;
  }
  spllt_solve_workspace_size(fkeep, 1, nrhs, worksize);
  fill_info(*f->S, info);
}

void spllt_set_mem_solve(void* akeep, void* fkeep, int nb, int nrhs, long worksize, double* y,
                         double* workspace, spllt_inform_t* info) {
  (void)akeep; (void)nb; (void)nrhs;
  clear_info(info);
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!f || !f->S) {
    std::fprintf(stderr, "spllt-hip: Error, fkeep provided by the user is empty\n");
    if (info) info->flag = SPLLT_ERROR_PARAMETER;
    return;
  }
  if (!y) std::fprintf(stderr, "spllt-hip: Error, y provided by the user is empty\n");
  if (!workspace) std::fprintf(stderr, "spllt-hip: Error, workspace provided by the user is empty\n");
  f->y = y;
  f->workspace = workspace;
  f->worksize = worksize;
  fill_info(*f->S, info);
}

void spllt_solve(void* fkeep, spllt_options_t* options, int* order, int nrhs, double* x,
                 spllt_inform_t* info, int job) {
  (void)options; (void)order;  // `order` is ignored by the reference too (ciface:404-419)
  clear_info(info);
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!f || !f->S || !x) {
    std::fprintf(stderr, "spllt-hip: Error, fkeep/x provided by the user is empty\n");
    if (info) info->flag = SPLLT_ERROR_PARAMETER;
    return;
  }
  if (job < 0 || job > 2) {
    // reference src/spllt_solve_mod.F90:216-220
    std::fprintf(stderr, "Unknown requested job = %2d returned code : %4d\n", job, SPLLT_ERROR_PARAMETER);
    if (info) info->flag = SPLLT_ERROR_PARAMETER;
    return;
  }
  // Solve on the device-resident factor (no D2H of L).
  int rc = do_wait(f);
  if (rc == 0 && no_factor(f)) rc = SPLLT_ERROR_PARAMETER;  // nothing factorized yet
  if (rc) { if (info) info->flag = rc; return; }
  if (f->eo.nranks > 1 && !f->eng->has_communicator()) {
    // (with spllt_hip_set_communicator the engine runs the two all-reduces itself, below)
    // A partitioned factor is spread over the ranks (own subtrees + replicated top
    // tree); this process holds only its part, so a local substitution would be
    // wrong.  The partitioned solve is spllt_hip_solve_dev in three phases with the
    // caller's all-reduce in between (spllt_amd/multigpu.py, DistributedFactorization.solve).
    std::fprintf(stderr, "spllt-hip: spllt_solve on a partitioned (multi-GPU) factor needs the caller's "
                         "exchange: use spllt_hip_solve_dev (phases 0, 1, 2)\n");
    if (info) info->flag = SPLLT_ERROR_UNIMPLEMENTED;
    return;
  }
  f->eng->set_reproducible_solve(f->repro_solve);
  rc = f->eng->solve(x, nrhs, job);
  if (rc) { if (info) info->flag = rc; return; }
  fill_info(*f->S, info);
}

int spllt_hip_solve_dev(void* fkeep, void* y_dev, int nrhs, int job, int phase) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (int rc = enter(f, nullptr, y_dev ? nullptr : "", WAIT | FACTOR)) return rc;
  f->eng->set_reproducible_solve(f->repro_solve);
  return f->eng->solve_dev(static_cast<double*>(y_dev), nrhs, job, phase);
}

void spllt_solve_worker(void* fkeep, spllt_options_t* options, int* order, int nrhs, double* x,
                        spllt_inform_t* info, int job, double* workspace, long worksize, void* tm) {
  (void)workspace; (void)worksize; (void)tm;
  spllt_solve(fkeep, options, order, nrhs, x, info, job);
}

// reference src/utils_mod.F90:432-478 (check_backward_error_multi): scaled
// backward error ||b - A x||_2 / (||b||_2 + max|a_ij| ||x||_2), pass <= 1e-14.
void spllt_chkerr(int n, int* ptr, int* row, double* val, int nrhs, double* x, double* rhs) {
  if (!ptr || !row || !val || !x || !rhs) {
    std::fprintf(stderr, "spllt-hip: Error, an array provided by the user is empty\n");
    return;
  }
  double amax = 0;
  for (int e = 0; e < ptr[n] - 1; ++e) amax = std::max(amax, std::fabs(val[e]));
  int ok = 0;
  std::vector<double> res(n);
  for (int r = 0; r < nrhs; ++r) {
    const double* xr = x + (int64_t)r * n;
    const double* br = rhs + (int64_t)r * n;
    for (int i = 0; i < n; ++i) res[i] = br[i];
    for (int j = 0; j < n; ++j)
      for (int e = ptr[j] - 1; e < ptr[j + 1] - 1; ++e) {
        int i = row[e] - 1;
        res[i] -= val[e] * xr[j];
        if (i != j) res[j] -= val[e] * xr[i];
      }
    double nr = 0, nb = 0, nx = 0;
    for (int i = 0; i < n; ++i) { nr += res[i] * res[i]; nb += br[i] * br[i]; nx += xr[i] * xr[i]; }
    double err = std::sqrt(nr) / (std::sqrt(nb) + amax * std::sqrt(nx));
    if (err != err) {
      std::printf("Backward error of rhs %3d is equal to a NAN\n", r + 1);
    } else if (err > 1e-14) {
      std::fprintf(stderr, "Wrong Bwd error for %4d/%4d : %10.2e\n", r + 1, nrhs, err);
    } else {
      std::fprintf(stderr, "Bwd error for %4d/%4d : %10.2e\n", r + 1, nrhs, err);
      ok++;
    }
  }
  std::fprintf(stderr, "Backward error... ok for %3d/%3d\n", ok, nrhs);
}

void spllt_deallocate_fkeep(void** fkeep, int* stat) {
  if (stat) *stat = 0;
  if (!fkeep || !*fkeep) return;
  Fkeep* f = static_cast<Fkeep*>(*fkeep);
  {
    std::lock_guard<std::mutex> lk(g_mu);
    g_pending.erase(std::remove(g_pending.begin(), g_pending.end(), f), g_pending.end());
  }
  if (f->dead) {
    // a submission of this handle never returned: the helper thread may still be inside the
    // engine, and if it was merely slow it goes on to write f->eng and to read the symbolic
    // structure and the staged values through f -- the whole handle is leaked, not just its parts
    // (and `val` of the spllt_factor call that failed must stay valid: spllt_iface.h)
    *fkeep = nullptr;
    return;
  }
  delete f;
  *fkeep = nullptr;
}

void spllt_deallocate_akeep(void** akeep, int* stat) {
  if (stat) *stat = 0;
  if (!akeep || !*akeep) return;
  delete static_cast<Akeep*>(*akeep);
  *akeep = nullptr;
}

// The reference's task manager drives the OpenMP solve tasks; the stream-DAG
// engine needs none.  A token object keeps init/deallocate pairs well-formed.
void spllt_task_manager_init(void** task_manager) {
  if (task_manager) *task_manager = new int(0);
}
void spllt_task_manager_deallocate(void** task_manager, int* stat) {
  if (stat) *stat = 0;
  if (!task_manager || !*task_manager) return;
  delete static_cast<int*>(*task_manager);
  *task_manager = nullptr;
}

void spllt_all(void** akeep, void** fkeep, spllt_options_t* options, int n, int nnz, int nrhs,
               int nb, int* ptr, int* row, double* val, double* x, double* rhs,
               spllt_inform_t* info) {
  if (options) options->nb = nb;
  std::vector<int> order((size_t)std::max(1, n));
  spllt_analyse(akeep, fkeep, options, n, ptr, row, info, order.data());
  if (info && info->flag < 0) return;
  spllt_factor(*akeep, *fkeep, options, nnz, val, info);
  if (info && info->flag < 0) return;
  int rc = spllt_hip_wait(*fkeep);
  if (rc) { if (info) info->flag = rc; return; }
  long ws = 0;
  spllt_prepare_solve(*akeep, *fkeep, nb, nrhs, &ws, info);
  if (x != rhs) std::memcpy(x, rhs, sizeof(double) * (size_t)n * nrhs);
  spllt_solve(*fkeep, options, order.data(), nrhs, x, info, 0);
  if (info && info->flag < 0) return;
  spllt_chkerr(n, ptr, row, val, nrhs, x, rhs);
}

// ---------------------------------------------------------------------------
// extensions
// ---------------------------------------------------------------------------
int spllt_hip_sym_info(const void* akeep, spllt_hip_sym_info_t* out) {
  const Akeep* a = static_cast<const Akeep*>(akeep);
  if (!a || !a->S || !out) return SPLLT_ERROR_PARAMETER;
  const Symbolic& S = *a->S;
  std::memset(out, 0, sizeof(*out));
  out->n = S.n; out->nnz_a = S.nnzA; out->nnodes = S.nnodes; out->nbcol = S.nbcol();
  out->nblk = S.nblk; out->arena = S.arena; out->nnz_l = S.nnzL; out->flops = S.flops;
  out->rlist_len = (int64_t)S.rlist.size();
  out->nb = S.nb; out->maxmn = S.maxmn; out->maxdepth = S.maxdepth;
  int nl = 0;
  for (int s = 0; s < S.nnodes; ++s) nl = std::max(nl, S.level[s] + 1);
  out->nlevels = nl;
  std::snprintf(out->ordering, sizeof out->ordering, "%s", S.ordering.c_str());
  return 0;
}

int64_t spllt_hip_sym_get(const void* akeep, const char* name, void* buf, int64_t cap) {
  const Akeep* a = static_cast<const Akeep*>(akeep);
  if (!a || !a->S || !name) return -1;
  const Symbolic& S = *a->S;
  std::string k(name);
  const Out o{buf, cap};
  if (k == "order") return o.elems(S.order);
  if (k == "sptr") return o.elems(S.sptr);
  if (k == "sparent") return o.elems(S.sparent);
  if (k == "rlist") return o.elems(S.rlist);
  if (k == "small") return o.elems(S.small);
  if (k == "level") return o.elems(S.level);
  if (k == "rptr") return o.elems(S.rptr);
  if (k == "map_dst") return o.elems(S.map_dst);
  if (k == "map_src") return o.elems(S.map_src);
  if (k == "lmap_ptr") return o.elems(S.lmap_ptr);
  if (k == "weight") return o.elems(S.weight);
  if (k == "node_bcol0") return o.elems(S.node_bcol0);
  if (k.rfind("bcol_", 0) == 0) {
    const int nb = S.nbcol();
    if (k == "bcol_off") {
      std::vector<int64_t> v(nb);
      for (int b = 0; b < nb; ++b) v[b] = S.bcols[b].off;
      return o.elems(v);
    }
    std::vector<int> v(nb);
    for (int b = 0; b < nb; ++b) {
      const BlockCol& B = S.bcols[b];
      v[b] = k == "bcol_node" ? B.node : k == "bcol_width" ? B.width : k == "bcol_r0" ? B.r0 : k == "bcol_nrow" ? B.nrow : -1;
    }
    return o.elems(v);
  }
  return -1;
}

int spllt_hip_set_engine(void* fkeep, int panel_width, int tile, int flags) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!f) return SPLLT_ERROR_PARAMETER;
  if (f->eng) return SPLLT_ERROR_PARAMETER;  // too late
  if (panel_width > 0) f->eo.pw = std::min(panel_width, kPanelMax);
  if (tile > 0) f->eo.tile = tile;
  f->eo.lookahead = (flags & 2) == 0;       // bit 1 set: single-stream program
  f->eo.slice_between = (flags & 64) == 0;  // bit 6 set: inter-node updates only at the end of a level
  f->eo.poison_lds = (flags & 128) != 0;    // bit 7 set: debug, LDS poisoned before every launch
  if (flags & 256) f->eo.reserve_cus = 0;   // bit 8 set: no CU reservation for the chain
  if (flags & 1024) f->eo.zones = 1;        // bit 10 / 11: force the zone pipeline (and the atomic
  if (flags & 2048) f->eo.zones = 0;        // trailing updates that go with it) on / off
  f->eo.fused_panel = (flags & 512) == 0;   // bit 9 set: no fused panel launches (POTRF, TRSM, update apart)
  f->eo.deterministic = (flags & 4096) != 0;
  if (flags & 8192) f->eo.dist_top = 1;     // bit 13 / 14: top tree of a partitioned factorization
  if (flags & 16384) f->eo.dist_top = 0;    // distributed over the ranks / replicated on every rank  // bit 12: no atomics (buffer + ordered gather)
  if (flags & 32768) f->eo.graph = 1;       // bit 15 / 16: HIP-graph replay, one chain in program order /
  if (flags & 65536) f->eo.graph = 2;       // the DAG of the multi-stream program
  if (flags & 131072) f->eo.graph = 0;      // bit 17: eager launches
  if (flags & 262144) f->eo.subtrees = 1;   // bit 18 / 19: small subtrees as single device tasks (L_SUBTREE)
  if (flags & 524288) f->eo.subtrees = 0;   // on / off
  return 0;
}

// test hooks of the process-wide "runtime is wedged" state (engine.cpp): "wedge" sets it, "wedged"
// reads it, "teardown" runs the atexit handler of the pools now; then the "name=value" switches:
//   batch_grid_limit=N      the grid size from which on a batched launch is split by member range (N <= 0: the
//                           hardware limit again)
//   fmult_alloc_fail=N      the next N allocations of the products' second workspace and scratch fail (those of
//                           the batched products and the workspace of the batched blocked solve included)
//   alloc_fail_at=K         the K-th allocation of feature memory from now on fails once with "out of memory" and the
//                           hook disarms itself (0 disarms it); "alloc_fail_armed" reads whether it still waits
//   batch_selinv_fused=0|1  0 forces the three-launch form of every step of the batched selected inversion
//   batch_fadj_fused=0|1    1 runs the eligible steps of the factor adjoint of a batch as one fused launch each (default 0)
//   rsolve_poison=0|1       1 fills the scratch of the reproducible solve with NaN before every sweep
//   batch_repro_poison=0|1  1 fills the scratch of the deterministic batch factorization and that of the reproducible
//                           batch sweep with NaN before every factorization and every sweep
//   solve_sparse_poison=0|1 1 fills the workspace of a sparse solve with NaN before its touched rows are zeroed
//   solve_sparse_batch_poison=0|1 1 fills the whole workspace of the batch with NaN before a sparse solve of the batch
//                           zeroes its touched rows
//   fmult_poison=0|1        1 fills the scratch of the factor products (the batched ones too) with NaN before every
//                           direction
int spllt_hip_debug(const char* what) {
  if (!what) return -1;
  const std::string w(what);
  if (w == "wedge") { mark_runtime_wedged(); return 0; }
  if (w == "wedged") return runtime_wedged() ? 1 : 0;
  if (w == "teardown") { run_pools_teardown_for_test(); return 0; }
  if (w == "alloc_fail_armed") return alloc_fail_armed() ? 1 : 0;
  const size_t eq = w.find('=');
  if (eq == std::string::npos) return -1;
  const std::string name = w.substr(0, eq), value = w.substr(eq + 1);
  if (name == "batch_grid_limit") { set_batch_grid_limit(std::atoll(value.c_str())); return 0; }
  if (name == "fmult_alloc_fail") { set_fmult_alloc_fail(std::atoi(value.c_str())); return 0; }
  if (name == "alloc_fail_at") { set_alloc_fail_at(std::atoi(value.c_str())); return 0; }
  static const struct { const char* name; void (*set)(bool); } kSwitches[] = {
      {"batch_selinv_fused", set_batch_selinv_fused}, {"batch_fadj_fused", set_batch_fadj_fused},
      {"rsolve_poison", set_rsolve_poison}, {"batch_repro_poison", set_batch_repro_poison},
      {"solve_sparse_poison", set_solve_sparse_poison}, {"fmult_poison", set_fmult_poison},
      {"solve_sparse_batch_poison", set_solve_sparse_batch_poison}};
  for (const auto& s : kSwitches)
    if (name == s.name && (value == "0" || value == "1")) { s.set(value == "1"); return 0; }
  return -1;
}

int spllt_hip_set_chain_block(void* fkeep, int chain_block) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!f || chain_block < 1) return SPLLT_ERROR_PARAMETER;
  if (f->eng) return SPLLT_ERROR_PARAMETER;  // too late
  f->eo.cb = chain_block;
  return 0;
}

// The program of a handle that has no engine (yet): built on the host, no GPU needed.
static void build_local_program(Fkeep* f, Program& local) {
  EngineOptions eo = f->eo;                 // (the handle's options stay unresolved)
  ScheduleOptions so = schedule_options(*f->S, eo);
  std::vector<int> owner, top_owner;
  partition_options(*f->S, f->eo, owner, top_owner, so);
  build_program(*f->S, so, local);
}

// ---- multi-GPU partition ---------------------------------------------------
// Works without a GPU (tests inspect the partition and the two-phase program):
// the owners are recomputed from the symbolic structure when no engine exists.
static void partition_tables(Fkeep* f, std::vector<int>& owner, std::vector<int>& top,
                             std::vector<char>& keep, int64_t& elems) {
  const Symbolic& S = *f->S;
  assign_owners(S, f->eo.nranks, owner);
  top.clear();
  elems = 0;
  for (int b = 0; b < S.nbcol(); ++b)
    if (owner[S.bcols[b].node] < 0) {
      top.push_back(b);
      elems += (int64_t)S.bcols[b].nrow * S.bcols[b].width;
    }
  keep.assign(S.map_dst.size(), 0);
  for (int b = 0; b < S.nbcol(); ++b) {
    const int own = owner[S.bcols[b].node];
    if ((own == f->eo.rank) || (own < 0 && f->eo.rank == 0))
      for (int64_t i = S.lmap_ptr[b]; i < S.lmap_ptr[b + 1]; ++i) keep[i] = 1;
  }
}

int spllt_hip_set_partition(void* fkeep, int rank, int nranks, int64_t* exchange_elems) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!f || !f->S || nranks < 1 || rank < 0 || rank >= nranks) return SPLLT_ERROR_PARAMETER;
  if (f->eng) return SPLLT_ERROR_PARAMETER;  // too late
  f->eo.rank = rank;
  f->eo.nranks = nranks;
  if (exchange_elems) {
    *exchange_elems = 0;
    if (nranks > 1) {   // the largest exchange of this rank's program
      Program local;
      build_local_program(f, local);
      *exchange_elems = local.xbuf_elems;
    }
  }
  return 0;
}

void* spllt_hip_engine_stream(void* fkeep) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!f || !f->S) return nullptr;
  // (created here so that the caller can order its collective on it before the first factor)
  if (ensure_engine(f)) return nullptr;
  return (void*)f->eng->stream();
}

void* spllt_hip_exchange_stream(void* fkeep) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!f || !f->S || !f->eng) return spllt_hip_engine_stream(fkeep);
  return (void*)f->eng->pending_exchange_stream();
}

int spllt_hip_set_communicator(void* fkeep, void* nccl_comm) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (int rc = enter(f, nullptr, nullptr, ENGINE)) return rc;
  int rc = f->eng->set_communicator(nccl_comm);
  if (rc) f->last_error = f->eng->error();
  return rc;
}

int spllt_hip_set_exchange_buffer(void* fkeep, void* dev_ptr) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!f || !f->S) return SPLLT_ERROR_PARAMETER;
  f->xbuf = static_cast<double*>(dev_ptr);
  if (f->eng) f->eng->set_exchange_buffer(f->xbuf);
  return 0;
}

int spllt_hip_pending_exchange(void* fkeep) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!f || !f->eng) return -1;
  return f->eng->pending_exchange();
}

int spllt_hip_continue(void* fkeep) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!f || !f->eng) return SPLLT_ERROR_PARAMETER;
  int rc = f->eng->continue_after_exchange();
  f->last_flag = rc;
  if (rc == 0) mark_pending(f);
  return rc;
}

int64_t spllt_hip_partition_get(void* fkeep, const char* name, void* buf, int64_t cap) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!f || !f->S || !name) return -1;
  std::vector<int> owner, top;
  std::vector<char> keep;
  int64_t elems = 0;
  partition_tables(f, owner, top, keep, elems);
  const std::string k(name);
  const Out o{buf, cap};
  if (k == "arena_elems") {   // int64 x 2: doubles of the factor arena held on this rank's device, of the whole arena
    int64_t v[2] = {f->eng ? f->eng->arena_elems() : f->S->arena, f->S->arena};
    return o.bytes(v, sizeof v);
  }
  if (k == "owner") return o.bytes(owner);
  if (k == "top_bcol_owner") {   // empty: the top tree is replicated
    ScheduleOptions so;
    std::vector<int> o2, top_owner;
    partition_options(*f->S, f->eo, o2, top_owner, so);
    return o.bytes(top_owner);
  }
  if (k == "top_bcols") return o.bytes(top);
  if (k == "map_keep") return o.bytes(keep);
  return -1;
}

int spllt_hip_get_factor(void* fkeep, double* out, int64_t count) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (int rc = enter(f, nullptr, out ? nullptr : "", WAIT | FACTOR)) return rc;
  if (!f->hostL_valid) {
    f->hostL.resize((size_t)f->S->arena);
    if (int rc = f->eng->download(f->hostL.data(), f->S->arena)) return rc;
    f->hostL_valid = true;
  }
  std::memcpy(out, f->hostL.data(), sizeof(double) * (size_t)std::min<int64_t>(count, f->S->arena));
  return 0;
}

double* spllt_hip_device_factor(void* fkeep) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  return (f && f->eng) ? f->eng->device_L() : nullptr;
}

// ---- blocked, reproducible and product sweeps over many vectors --------------
// what the argument checks of the vector calls name; nrhs also stands for nvec and nsamp
static const char* vectors_bad(const Fkeep* f, int nrhs, const void* x, int64_t ldx, int job) {
  if (!x) return "the array of right-hand sides is null";
  if (nrhs < 0) return "nrhs < 0";
  if (ldx < f->S->n) return "ldx < n";
  if (job < 0 || job > 2) return "job is not 0, 1 or 2";
  return nullptr;
}

static int vectors_impl(const char* what, void* fkeep, int nrhs, double* x, int64_t ldx, int job,
                        int (Engine::*host)(double*, int, int64_t, int), int (Engine::*dev)(double*, int, int64_t, int, bool),
                        bool pivot_order) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!analysed(f)) return SPLLT_ERROR_PARAMETER;
  if (int rc = enter(f, what, vectors_bad(f, nrhs, x, ldx, job), SINGLE_F | WAIT | FACTOR)) return rc;
  Engine& e = *f->eng;
  return leave(f, host ? (e.*host)(x, nrhs, ldx, job) : (e.*dev)(x, nrhs, ldx, job, pivot_order));
}

int spllt_hip_solve_many(void* fkeep, int nrhs, double* x_host, int64_t ldx, int job) {
  return vectors_impl("spllt_hip_solve_many", fkeep, nrhs, x_host, ldx, job, &Engine::solve_many, nullptr, false);
}

int spllt_hip_solve_many_dev(void* fkeep, int nrhs, double* x_dev, int64_t ldx, int job, int pivot_order) {
  return vectors_impl("spllt_hip_solve_many_dev", fkeep, nrhs, x_dev, ldx, job, nullptr, &Engine::solve_many_dev,
                      pivot_order != 0);
}

int spllt_hip_solve_repro(void* fkeep, int nrhs, double* x_host, int64_t ldx, int job) {
  return vectors_impl("spllt_hip_solve_repro", fkeep, nrhs, x_host, ldx, job, &Engine::solve_repro, nullptr, false);
}

int spllt_hip_solve_repro_dev(void* fkeep, int nrhs, double* x_dev, int64_t ldx, int job, int pivot_order) {
  return vectors_impl("spllt_hip_solve_repro_dev", fkeep, nrhs, x_dev, ldx, job, nullptr, &Engine::solve_repro_dev,
                      pivot_order != 0);
}

int spllt_hip_factor_mult(void* fkeep, int nvec, double* x_host, int64_t ldx, int job) {
  return vectors_impl("spllt_hip_factor_mult", fkeep, nvec, x_host, ldx, job, &Engine::factor_mult, nullptr, false);
}

int spllt_hip_factor_mult_dev(void* fkeep, int nvec, double* x_dev, int64_t ldx, int job, int pivot_order) {
  return vectors_impl("spllt_hip_factor_mult_dev", fkeep, nvec, x_dev, ldx, job, nullptr, &Engine::factor_mult_dev,
                      pivot_order != 0);
}

int spllt_hip_set_reproducible_solve(void* fkeep, int on) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!f || !f->S) return SPLLT_ERROR_PARAMETER;
  if (on && f->eo.nranks > 1) {   // (a plain setter: refused without the stderr line of the guard)
    f->last_error = "spllt_hip_set_reproducible_solve: not available on a partitioned (multi-GPU) handle";
    return SPLLT_ERROR_UNIMPLEMENTED;
  }
  const int before = f->repro_solve ? 1 : 0;
  f->repro_solve = on != 0;
  return before;
}

// ---- Gaussian sampling ---------------------------------------------------------
static int sample_impl(const char* what, void* fkeep, int nsamp, double* x, int64_t ldx, int kind, uint64_t seed,
                       uint64_t first_sample, const double* mean, bool dev) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!analysed(f)) return SPLLT_ERROR_PARAMETER;
  const char* bad = vectors_bad(f, nsamp, x, ldx, 0);
  if (!bad && (kind < 0 || kind > 1)) bad = "kind is not 0 (precision) or 1 (covariance)";
  if (int rc = enter(f, what, bad, SINGLE_F | WAIT | FACTOR)) return rc;
  f->eng->set_reproducible_solve(f->repro_solve);
  return leave(f, f->eng->sample(x, nsamp, ldx, kind, seed, first_sample, mean, dev));
}

int spllt_hip_sample_dev(void* fkeep, int nsamp, double* x_dev, int64_t ldx, int kind, uint64_t seed,
                         uint64_t first_sample, const double* mean_dev) {
  return sample_impl("spllt_hip_sample_dev", fkeep, nsamp, x_dev, ldx, kind, seed, first_sample, mean_dev, true);
}

int spllt_hip_sample(void* fkeep, int nsamp, double* x_host, int64_t ldx, int kind, uint64_t seed,
                     uint64_t first_sample, const double* mean_host) {
  return sample_impl("spllt_hip_sample", fkeep, nsamp, x_host, ldx, kind, seed, first_sample, mean_host, false);
}

int spllt_hip_white_noise_dev(void* fkeep, int nsamp, double* z_dev, int64_t ldz, uint64_t seed, uint64_t first_sample) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!analysed(f)) return SPLLT_ERROR_PARAMETER;
  if (int rc = enter(f, "spllt_hip_white_noise_dev", vectors_bad(f, nsamp, z_dev, ldz, 0), SINGLE_F | WAIT | FACTOR))
    return rc;
  return leave(f, f->eng->white_noise_dev(z_dev, nsamp, ldz, seed, first_sample));
}

// ---- hard linear constraints C x = e (spllt_hip_constrain.h) ----------------------------------------
static int set_constraints_impl(const char* what, void* fkeep, int k, const double* c, int64_t ldc, bool dev) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!analysed(f)) return SPLLT_ERROR_PARAMETER;
  const char* bad = nullptr;
  if (k != 0 && !c) bad = "the array of constraint rows is null";
  else if (k < 0) bad = "k < 0";
  else if (k > 64) bad = "k > 64";
  else if (k > 0 && ldc < f->S->n) bad = "ldc < n";
  // (FACTORED, as the refined solves: on an engine that has never factorized, W would be numbers of an empty arena)
  if (int rc = enter(f, what, bad, SINGLE | WAIT | FACTORED)) return rc;
  f->eng->set_reproducible_solve(f->repro_solve);
  return leave(f, f->eng->set_constraints(k, c, ldc, dev, f->serial[0]));
}

int spllt_hip_set_constraints(void* fkeep, int k, const double* c_host, int64_t ldc) {
  return set_constraints_impl("spllt_hip_set_constraints", fkeep, k, c_host, ldc, false);
}

int spllt_hip_set_constraints_dev(void* fkeep, int k, const double* c_dev, int64_t ldc) {
  return set_constraints_impl("spllt_hip_set_constraints_dev", fkeep, k, c_dev, ldc, true);
}

// the correction behind nothing (op 0), the blocked solve (1) or the kind-0 sample (2): Engine::CnOp
static int constrain_impl(const char* what, int op, void* fkeep, int nvec, double* x, int64_t ldx, const double* e,
                          int64_t lde, double* lambda, int64_t ldl, bool dev, uint64_t seed, uint64_t first,
                          const double* mean) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!analysed(f)) return SPLLT_ERROR_PARAMETER;
  const char* bad = vectors_bad(f, nvec, x, ldx, 0);
  const int k = f->eng ? f->eng->constraints_k() : 0;   // (0: refused below, once the ladder is through)
  if (!bad && k > 0 && e && lde != 0 && lde < k) bad = "lde is neither 0 nor >= k";
  if (!bad && k > 0 && lambda && ldl < k) bad = "ldl < k";
  if (int rc = enter(f, what, bad, SINGLE | WAIT | FACTORED)) return rc;
  if (f->eng->constraints_k() <= 0) return fail(f, what, "no constraints are set on this handle (spllt_hip_set_constraints)");
  f->eng->set_reproducible_solve(f->repro_solve);
  return leave(f, f->eng->constrain(op, nvec, x, ldx, e, e ? lde : 0, lambda, ldl, dev, f->serial[0], seed, first, mean));
}

int spllt_hip_constrain(void* fkeep, int nvec, double* x_host, int64_t ldx, const double* e_host, int64_t lde,
                        double* lambda_host, int64_t ldl) {
  return constrain_impl("spllt_hip_constrain", Engine::CN_CORRECT, fkeep, nvec, x_host, ldx, e_host, lde, lambda_host, ldl,
                        false, 0, 0, nullptr);
}

int spllt_hip_constrain_dev(void* fkeep, int nvec, double* x_dev, int64_t ldx, const double* e_dev, int64_t lde,
                            double* lambda_dev, int64_t ldl) {
  return constrain_impl("spllt_hip_constrain_dev", Engine::CN_CORRECT, fkeep, nvec, x_dev, ldx, e_dev, lde, lambda_dev, ldl,
                        true, 0, 0, nullptr);
}

int spllt_hip_solve_constrained(void* fkeep, int nrhs, double* x_host, int64_t ldx, const double* e_host, int64_t lde,
                                double* lambda_host, int64_t ldl) {
  return constrain_impl("spllt_hip_solve_constrained", Engine::CN_SOLVE, fkeep, nrhs, x_host, ldx, e_host, lde, lambda_host,
                        ldl, false, 0, 0, nullptr);
}

int spllt_hip_solve_constrained_dev(void* fkeep, int nrhs, double* x_dev, int64_t ldx, const double* e_dev, int64_t lde,
                                    double* lambda_dev, int64_t ldl) {
  return constrain_impl("spllt_hip_solve_constrained_dev", Engine::CN_SOLVE, fkeep, nrhs, x_dev, ldx, e_dev, lde, lambda_dev,
                        ldl, true, 0, 0, nullptr);
}

int spllt_hip_sample_constrained(void* fkeep, int nsamp, double* x_host, int64_t ldx, uint64_t seed, uint64_t first_sample,
                                 const double* mean_host, const double* e_host) {
  return constrain_impl("spllt_hip_sample_constrained", Engine::CN_SAMPLE, fkeep, nsamp, x_host, ldx, e_host, 0, nullptr, 0,
                        false, seed, first_sample, mean_host);
}

int spllt_hip_sample_constrained_dev(void* fkeep, int nsamp, double* x_dev, int64_t ldx, uint64_t seed,
                                     uint64_t first_sample, const double* mean_dev, const double* e_dev) {
  return constrain_impl("spllt_hip_sample_constrained_dev", Engine::CN_SAMPLE, fkeep, nsamp, x_dev, ldx, e_dev, 0, nullptr, 0,
                        true, seed, first_sample, mean_dev);
}

int spllt_hip_inverse_diag_constrained(void* fkeep, double* out, int n) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  const char* what = "spllt_hip_inverse_diag_constrained";
  if (int rc = enter(f, what, out ? nullptr : "", SINGLE_F | WAIT | FACTOR | INVERSE)) return rc;
  if (n != f->S->n)
    return fail(f, what, "n = " + std::to_string(n) + " does not match the analysed order " + std::to_string(f->S->n));
  if (f->eng->constraints_k() <= 0) return fail(f, what, "no constraints are set on this handle (spllt_hip_set_constraints)");
  f->eng->set_reproducible_solve(f->repro_solve);
  return leave(f, f->eng->inverse_diag_constrained(out, n, f->serial[0]));
}

int spllt_hip_constraints_info(void* fkeep, int64_t out[4], double stat[2]) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!f || !f->S || !out || !stat) return SPLLT_ERROR_PARAMETER;
  for (int i = 0; i < 4; ++i) out[i] = 0;
  stat[0] = stat[1] = 0.0;
  if (f->eng && !f->dead) f->eng->constraints_info(out, stat);
  return 0;
}

// ---- batched factorization --------------------------------------------------
static int factor_batch_impl(void* akeep, void* fkeep, int nbatch, int nnz, const double* val, int64_t ldval, bool dev,
                             const char* what) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!akeep || !analysed(f)) return SPLLT_ERROR_PARAMETER;
  const char* bad = nullptr;
  if (!val) bad = "the array of values is null";
  else if (nbatch < 0) bad = "nbatch < 0";
  else if ((int64_t)nnz != f->S->nnzA) bad = "nnz does not match the analysed pattern";
  else if (ldval < nnz) bad = "ldval < nnz";
  // (EMPTY_FIRST: an empty batch is accepted on a dead handle)
  if (int rc = enter(f, what, bad, SINGLE | WAIT_IGNORE | ENGINE | (nbatch == 0 ? EMPTY | EMPTY_FIRST : 0)))
    return done(rc);
  int rc = f->eng->factor_batch(val, dev, nbatch, ldval);
  if (rc == 0 || rc == SPLLT_ERROR_NOT_POSDEF) ++f->serial[1];   // (the members that are positive definite were factorized)
  if (rc == SPLLT_ERROR_NOT_POSDEF) {   // -20 of the batch calls: the batch stands, the message says which members failed
    const std::vector<int>& fl = f->eng->batch_flags();
    int nbad = 0, first = -1;
    for (size_t b = 0; b < fl.size(); ++b)
      if (fl[b] != INT_MAX) { if (first < 0) first = (int)b; ++nbad; }
    return fail(f, what, std::to_string(nbad) + " of " + std::to_string(nbatch) +
                             " members are not positive definite (first: member " + std::to_string(first) +
                             ", pivot column " + std::to_string(first >= 0 ? fl[(size_t)first] : 0) + " in elimination order)",
                rc);
  }
  return leave(f, rc);
}

int spllt_hip_factor_batch(void* akeep, void* fkeep, int nbatch, int nnz, const double* val_host, int64_t ldval) {
  return factor_batch_impl(akeep, fkeep, nbatch, nnz, val_host, ldval, false, "spllt_hip_factor_batch");
}

int spllt_hip_factor_batch_dev(void* akeep, void* fkeep, int nbatch, int nnz, const double* val_dev, int64_t ldval) {
  return factor_batch_impl(akeep, fkeep, nbatch, nnz, val_dev, ldval, true, "spllt_hip_factor_batch_dev");
}

int spllt_hip_batch_status(void* fkeep, int* flag, int* column, int capacity) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!f) return SPLLT_ERROR_PARAMETER;
  if (!f->eng || f->dead) return 0;
  const std::vector<int>& fl = f->eng->batch_flags();
  const int nb = f->eng->batch_count();
  for (int b = 0; b < nb && b < capacity; ++b) {
    const bool bad = fl[(size_t)b] != INT_MAX;
    if (flag) flag[b] = bad ? SPLLT_ERROR_NOT_POSDEF : 0;
    if (column) column[b] = bad ? fl[(size_t)b] : 0;
  }
  return nb;
}

static int solve_batch_impl(void* fkeep, int nrhs, double* x, int64_t ldx, int job, bool dev, bool pivot_order,
                            const char* what) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!analysed(f)) return SPLLT_ERROR_PARAMETER;
  if (int rc = enter(f, what, vectors_bad(f, nrhs, x, ldx, job), SINGLE | WAIT_IGNORE | BATCH)) return rc;
  if (nrhs == 0) return 0;
  int rc = f->eng->solve_batch(x, dev, nrhs, ldx, job, pivot_order);
  if (rc == SPLLT_ERROR_NOT_POSDEF)   // -20 of the batch calls
    return fail(f, what, "the vectors of the members that are not positive definite were left unchanged "
                         "(spllt_hip_batch_status)", rc);
  return leave(f, rc);
}

int spllt_hip_solve_batch(void* fkeep, int nrhs, double* x_host, int64_t ldx, int job) {
  return solve_batch_impl(fkeep, nrhs, x_host, ldx, job, false, false, "spllt_hip_solve_batch");
}

int spllt_hip_solve_batch_dev(void* fkeep, int nrhs, double* x_dev, int64_t ldx, int job, int pivot_order) {
  return solve_batch_impl(fkeep, nrhs, x_dev, ldx, job, true, pivot_order != 0, "spllt_hip_solve_batch_dev");
}

// ---- factor products and sampling for the members of a batch (spllt_hip_batch_mult.h) -------------
// the rungs of solve_batch_impl, in its order; -20 of the batch calls with the message of the family
static int batch_mult_leave(Fkeep* f, const char* what, int rc, const char* failed) {
  if (rc == SPLLT_ERROR_NOT_POSDEF) return fail(f, what, std::string(failed) + " (spllt_hip_batch_status)", rc);
  return leave(f, rc);
}

static int factor_mult_batch_impl(void* fkeep, int nvec, double* x, int64_t ldx, int job, bool dev, bool pivot_order,
                                  const char* what) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!analysed(f)) return SPLLT_ERROR_PARAMETER;
  if (int rc = enter(f, what, vectors_bad(f, nvec, x, ldx, job), SINGLE | WAIT_IGNORE | BATCH)) return rc;
  if (nvec == 0) return 0;
  Engine& e = *f->eng;
  return batch_mult_leave(f, what, dev ? e.factor_mult_batch_dev(x, nvec, ldx, job, pivot_order) : e.factor_mult_batch(x, nvec, ldx, job),
                          "the vectors of the members that are not positive definite were left unchanged");
}

int spllt_hip_factor_mult_batch(void* fkeep, int nvec, double* x_host, int64_t ldx, int job) {
  return factor_mult_batch_impl(fkeep, nvec, x_host, ldx, job, false, false, "spllt_hip_factor_mult_batch");
}

int spllt_hip_factor_mult_batch_dev(void* fkeep, int nvec, double* x_dev, int64_t ldx, int job, int pivot_order) {
  return factor_mult_batch_impl(fkeep, nvec, x_dev, ldx, job, true, pivot_order != 0, "spllt_hip_factor_mult_batch_dev");
}

int spllt_hip_white_noise_batch_dev(void* fkeep, int nsamp, double* z_dev, int64_t ldz, uint64_t seed,
                                    uint64_t first_sample, uint32_t stream0, int stream_step) {
  const char* what = "spllt_hip_white_noise_batch_dev";
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!analysed(f)) return SPLLT_ERROR_PARAMETER;
  const char* bad = vectors_bad(f, nsamp, z_dev, ldz, 0);
  if (!bad && (stream_step < 0 || stream_step > 1)) bad = "stream_step is not 0 (common noise) or 1 (a stream per member)";
  if (int rc = enter(f, what, bad, SINGLE | WAIT_IGNORE | BATCH)) return rc;
  if (nsamp == 0) return 0;
  return batch_mult_leave(f, what, f->eng->white_noise_batch_dev(z_dev, nsamp, ldz, seed, first_sample, stream0, stream_step),
                          "the noise of the members that are not positive definite is NaN");
}

static int sample_batch_impl(const char* what, void* fkeep, int nsamp, double* x, int64_t ldx, int kind, uint64_t seed,
                             uint64_t first_sample, uint32_t stream0, int stream_step, const double* mean, int64_t ldmean,
                             bool dev) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!analysed(f)) return SPLLT_ERROR_PARAMETER;
  const char* bad = vectors_bad(f, nsamp, x, ldx, 0);
  if (!bad && (kind < 0 || kind > 1)) bad = "kind is not 0 (precision) or 1 (covariance)";
  if (!bad && (stream_step < 0 || stream_step > 1)) bad = "stream_step is not 0 (common noise) or 1 (a stream per member)";
  if (!bad && mean && ldmean != 0 && ldmean < f->S->n) bad = "ldmean is neither 0 (one mean for all members) nor >= n";
  if (int rc = enter(f, what, bad, SINGLE | WAIT_IGNORE | BATCH)) return rc;
  if (nsamp == 0) return 0;
  f->eng->set_batch_blocked_solve(f->batch_blocked);
  return batch_mult_leave(f, what,
                          f->eng->sample_batch(x, nsamp, ldx, kind, seed, first_sample, stream0, stream_step, mean, ldmean, dev),
                          "the samples of the members that are not positive definite are NaN");
}

int spllt_hip_sample_batch(void* fkeep, int nsamp, double* x_host, int64_t ldx, int kind, uint64_t seed,
                           uint64_t first_sample, uint32_t stream0, int stream_step, const double* mean_host,
                           int64_t ldmean) {
  return sample_batch_impl("spllt_hip_sample_batch", fkeep, nsamp, x_host, ldx, kind, seed, first_sample, stream0,
                           stream_step, mean_host, ldmean, false);
}

int spllt_hip_sample_batch_dev(void* fkeep, int nsamp, double* x_dev, int64_t ldx, int kind, uint64_t seed,
                               uint64_t first_sample, uint32_t stream0, int stream_step, const double* mean_dev,
                               int64_t ldmean) {
  return sample_batch_impl("spllt_hip_sample_batch_dev", fkeep, nsamp, x_dev, ldx, kind, seed, first_sample, stream0,
                           stream_step, mean_dev, ldmean, true);
}

// ---- blocked solve for the members of a batch (spllt_hip_batch_solve_many.h) -----------------------
// the rungs of solve_batch_impl, in its order
static int solve_many_batch_impl(void* fkeep, int nrhs, double* x, int64_t ldx, int job, bool dev, bool pivot_order,
                                 const char* what) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!analysed(f)) return SPLLT_ERROR_PARAMETER;
  if (int rc = enter(f, what, vectors_bad(f, nrhs, x, ldx, job), SINGLE | WAIT_IGNORE | BATCH)) return rc;
  if (nrhs == 0) return 0;
  return batch_mult_leave(f, what, f->eng->solve_many_batch(x, dev, nrhs, ldx, job, pivot_order),
                          "the vectors of the members that are not positive definite were left unchanged");
}

int spllt_hip_solve_many_batch(void* fkeep, int nrhs, double* x_host, int64_t ldx, int job) {
  return solve_many_batch_impl(fkeep, nrhs, x_host, ldx, job, false, false, "spllt_hip_solve_many_batch");
}

int spllt_hip_solve_many_batch_dev(void* fkeep, int nrhs, double* x_dev, int64_t ldx, int job, int pivot_order) {
  return solve_many_batch_impl(fkeep, nrhs, x_dev, ldx, job, true, pivot_order != 0, "spllt_hip_solve_many_batch_dev");
}

int spllt_hip_set_batch_blocked_solve(void* fkeep, int on) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!f || !f->S) return SPLLT_ERROR_PARAMETER;
  if (on && f->eo.nranks > 1) {   // (a plain setter: refused without the stderr line of the guard)
    f->last_error = "spllt_hip_set_batch_blocked_solve: not available on a partitioned (multi-GPU) handle";
    return SPLLT_ERROR_UNIMPLEMENTED;
  }
  const int before = f->batch_blocked ? 1 : 0;
  f->batch_blocked = on != 0;
  return before;
}

int spllt_hip_solve_many_batch_info(void* fkeep, int64_t out[4]) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!f || !f->S || !out) return SPLLT_ERROR_PARAMETER;
  for (int i = 0; i < 4; ++i) out[i] = f->eng ? f->eng->solve_many_batch_info()[i] : 0;
  return 0;
}

// ---- the bit-reproducible batch (spllt_hip_batch_repro.h) -------------------------------------------
int spllt_hip_set_batch_reproducible(void* fkeep, int on) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!f || !f->S) return SPLLT_ERROR_PARAMETER;
  if (on && f->eo.nranks > 1) {   // (a plain setter: refused without the stderr line of the guard)
    f->last_error = "spllt_hip_set_batch_reproducible: not available on a partitioned (multi-GPU) handle";
    return SPLLT_ERROR_UNIMPLEMENTED;
  }
  const int before = f->batch_repro ? 1 : 0;
  f->batch_repro = on != 0;
  if (f->eng && !f->dead) f->eng->set_batch_reproducible(f->batch_repro);
  return before;
}

// the rungs of solve_many_batch_impl, in its order
static int solve_repro_batch_impl(void* fkeep, int nrhs, double* x, int64_t ldx, int job, bool dev, bool pivot_order,
                                  const char* what) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!analysed(f)) return SPLLT_ERROR_PARAMETER;
  if (int rc = enter(f, what, vectors_bad(f, nrhs, x, ldx, job), SINGLE | WAIT_IGNORE | BATCH)) return rc;
  if (nrhs == 0) return 0;
  return batch_mult_leave(f, what, f->eng->solve_repro_batch(x, dev, nrhs, ldx, job, pivot_order),
                          "the vectors of the members that are not positive definite were left unchanged");
}

int spllt_hip_solve_repro_batch(void* fkeep, int nrhs, double* x_host, int64_t ldx, int job) {
  return solve_repro_batch_impl(fkeep, nrhs, x_host, ldx, job, false, false, "spllt_hip_solve_repro_batch");
}

int spllt_hip_solve_repro_batch_dev(void* fkeep, int nrhs, double* x_dev, int64_t ldx, int job, int pivot_order) {
  return solve_repro_batch_impl(fkeep, nrhs, x_dev, ldx, job, true, pivot_order != 0, "spllt_hip_solve_repro_batch_dev");
}

int spllt_hip_batch_repro_info(void* fkeep, int64_t out[6]) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!f || !f->S || !out) return SPLLT_ERROR_PARAMETER;
  for (int i = 0; i < 6; ++i) out[i] = 0;
  if (f->eng && !f->dead) f->eng->batch_repro_info(out);
  out[0] = f->batch_repro ? 1 : 0;
  return 0;
}

// ---- refined solves ---------------------------------------------------------
static int matvec_impl(void* fkeep, int nnz, const double* val, int nvec, const double* x, int64_t ldx, double* y,
                       int64_t ldy, bool dev, bool pivot_order, const char* what) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!analysed(f)) return SPLLT_ERROR_PARAMETER;
  const char* bad = nullptr;
  if (!val) bad = "the array of values is null";
  else if (!x || !y) bad = "a vector array is null";
  else if (nvec < 0) bad = "nvec < 0";
  else if (ldx < f->S->n) bad = "ldx < n";
  else if (ldy < f->S->n) bad = "ldy < n";
  else if ((int64_t)nnz != f->S->nnzA) bad = "nnz does not match the analysed pattern";
  if (int rc = enter(f, what, bad, SINGLE | WAIT_IGNORE | ENGINE | (nvec == 0 ? EMPTY : 0))) return done(rc);
  return leave(f, f->eng->matvec(val, nvec, x, ldx, y, ldy, dev, pivot_order));
}

int spllt_hip_matvec(void* fkeep, int nnz, const double* val_host, int nvec, const double* x_host, int64_t ldx,
                     double* y_host, int64_t ldy) {
  return matvec_impl(fkeep, nnz, val_host, nvec, x_host, ldx, y_host, ldy, false, false, "spllt_hip_matvec");
}

int spllt_hip_matvec_dev(void* fkeep, int nnz, const double* val_dev, int nvec, const double* x_dev, int64_t ldx,
                         double* y_dev, int64_t ldy, int pivot_order) {
  return matvec_impl(fkeep, nnz, val_dev, nvec, x_dev, ldx, y_dev, ldy, true, pivot_order != 0, "spllt_hip_matvec_dev");
}

static int solve_refined_impl(void* fkeep, int nnz, const double* val, int nrhs, double* x, int64_t ldx, int method,
                              double tol, int max_iter, int* iterations, double* error, bool dev, const char* what) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!analysed(f)) return SPLLT_ERROR_PARAMETER;
  const char* bad = nullptr;
  if (!val) bad = "the array of values is null";
  else if (!x) bad = "the array of right-hand sides is null";
  else if (nrhs < 0) bad = "nrhs < 0";
  else if (ldx < f->S->n) bad = "ldx < n";
  else if (method != 0 && method != 1) bad = "method is not 0 (refinement) or 1 (PCG)";
  else if (!(tol > 0.0)) bad = "tol is not positive";
  else if (max_iter < 0) bad = "max_iter < 0";
  else if ((int64_t)nnz != f->S->nnzA) bad = "nnz does not match the analysed pattern";
  if (int rc = enter(f, what, bad, SINGLE | WAIT | FACTORED | (nrhs == 0 ? EMPTY : 0))) return done(rc);
  f->eng->set_reproducible_solve(f->repro_solve);
  int rc = f->eng->solve_refined(val, nrhs, x, ldx, dev, method, tol, max_iter, iterations, error);
  if (rc == 1)   // rc 1 of the refined solve: not an error, the vectors hold their best iterates
    return fail(f, what, "at least one vector did not reach tol (error[] says which)", 1);
  return leave(f, rc);
}

int spllt_hip_solve_refined(void* fkeep, int nnz, const double* val_host, int nrhs, double* x_host, int64_t ldx,
                            int method, double tol, int max_iter, int* iterations, double* error) {
  return solve_refined_impl(fkeep, nnz, val_host, nrhs, x_host, ldx, method, tol, max_iter, iterations, error, false,
                            "spllt_hip_solve_refined");
}

int spllt_hip_solve_refined_dev(void* fkeep, int nnz, const double* val_dev, int nrhs, double* x_dev, int64_t ldx,
                                int method, double tol, int max_iter, int* iterations, double* error) {
  return solve_refined_impl(fkeep, nnz, val_dev, nrhs, x_dev, ldx, method, tol, max_iter, iterations, error, true,
                            "spllt_hip_solve_refined_dev");
}

// ---- the product and the refined solves for the members of a batch (spllt_hip_batch_refine.h) --------
// what is wrong with the values of a batch call, or null
static const char* batch_values_bad(const Fkeep* f, int nnz, const double* val, int64_t ldval) {
  if (!val) return "the array of values is null";
  if ((int64_t)nnz != f->S->nnzA) return "nnz does not match the analysed pattern";
  if (ldval < nnz) return "ldval < nnz";
  return nullptr;
}

static int matvec_batch_impl(void* fkeep, int nbatch, int nnz, const double* val, int64_t ldval, int nvec, const double* x,
                             int64_t ldx, double* y, int64_t ldy, bool dev, bool pivot_order, const char* what) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!analysed(f)) return SPLLT_ERROR_PARAMETER;
  const char* bad = nullptr;
  if (!val) bad = "the array of values is null";
  else if (!x || !y) bad = "a vector array is null";
  else if (nbatch < 0) bad = "nbatch < 0";
  else if (nvec < 0) bad = "nvec < 0";
  else if ((bad = batch_values_bad(f, nnz, val, ldval))) {}
  else if (ldx < f->S->n) bad = "ldx < n";
  else if (ldy < f->S->n) bad = "ldy < n";
  if (int rc = enter(f, what, bad, SINGLE | WAIT_IGNORE | ENGINE | (nvec == 0 || nbatch == 0 ? EMPTY : 0))) return done(rc);
  return leave(f, f->eng->matvec_batch(val, ldval, nbatch, nvec, x, ldx, y, ldy, dev, pivot_order));
}

int spllt_hip_matvec_batch(void* fkeep, int nbatch, int nnz, const double* val_host, int64_t ldval, int nvec,
                           const double* x_host, int64_t ldx, double* y_host, int64_t ldy) {
  return matvec_batch_impl(fkeep, nbatch, nnz, val_host, ldval, nvec, x_host, ldx, y_host, ldy, false, false,
                           "spllt_hip_matvec_batch");
}

int spllt_hip_matvec_batch_dev(void* fkeep, int nbatch, int nnz, const double* val_dev, int64_t ldval, int nvec,
                               const double* x_dev, int64_t ldx, double* y_dev, int64_t ldy, int pivot_order) {
  return matvec_batch_impl(fkeep, nbatch, nnz, val_dev, ldval, nvec, x_dev, ldx, y_dev, ldy, true, pivot_order != 0,
                           "spllt_hip_matvec_batch_dev");
}

// the rungs of solve_batch_impl and of solve_refined_impl
static int solve_refined_batch_impl(void* fkeep, int nnz, const double* val, int64_t ldval, int nrhs, double* x, int64_t ldx,
                                    int method, double tol, int max_iter, int* iterations, double* error, bool dev,
                                    const char* what) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!analysed(f)) return SPLLT_ERROR_PARAMETER;
  const char* bad = nullptr;
  if (!val) bad = "the array of values is null";
  else if (!x) bad = "the array of right-hand sides is null";
  else if (nrhs < 0) bad = "nrhs < 0";
  else if ((bad = batch_values_bad(f, nnz, val, ldval))) {}
  else if (ldx < f->S->n) bad = "ldx < n";
  else if (method != 0 && method != 1) bad = "method is not 0 (refinement) or 1 (PCG)";
  else if (!(tol > 0.0)) bad = "tol is not positive";
  else if (max_iter < 0) bad = "max_iter < 0";
  if (int rc = enter(f, what, bad, SINGLE | WAIT_IGNORE | BATCH)) return rc;
  if (nrhs == 0) return 0;
  int rc = f->eng->solve_refined_batch(val, ldval, nrhs, x, ldx, dev, method, tol, max_iter, iterations, error);
  if (rc == 1)   // rc 1 of the refined solve: not an error, the vectors hold their best iterates
    return fail(f, what, "at least one vector did not reach tol (error[] says which)", 1);
  return batch_mult_leave(f, what, rc, "the vectors of the members that are not positive definite were left unchanged");
}

int spllt_hip_solve_refined_batch(void* fkeep, int nnz, const double* val_host, int64_t ldval, int nrhs, double* x_host,
                                  int64_t ldx, int method, double tol, int max_iter, int* iterations, double* error) {
  return solve_refined_batch_impl(fkeep, nnz, val_host, ldval, nrhs, x_host, ldx, method, tol, max_iter, iterations, error,
                                  false, "spllt_hip_solve_refined_batch");
}

int spllt_hip_solve_refined_batch_dev(void* fkeep, int nnz, const double* val_dev, int64_t ldval, int nrhs, double* x_dev,
                                      int64_t ldx, int method, double tol, int max_iter, int* iterations, double* error) {
  return solve_refined_batch_impl(fkeep, nnz, val_dev, ldval, nrhs, x_dev, ldx, method, tol, max_iter, iterations, error,
                                  true, "spllt_hip_solve_refined_batch_dev");
}

int spllt_hip_solve_refined_batch_info(void* fkeep, int64_t out[4]) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!f || !f->S || !out) return SPLLT_ERROR_PARAMETER;
  for (int i = 0; i < 4; ++i) out[i] = f->eng ? f->eng->solve_refined_batch_info()[i] : 0;
  return 0;
}

// ---- hard linear constraints for the members of a batch (spllt_hip_constrain_batch.h) ---------------
// the argument rungs of set_constraints_impl, then the handle rungs of solve_many_batch_impl
static int set_constraints_batch_impl(const char* what, void* fkeep, int k, const double* c, int64_t ldc, bool dev) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!analysed(f)) return SPLLT_ERROR_PARAMETER;
  const char* bad = nullptr;
  if (k != 0 && !c) bad = "the array of constraint rows is null";
  else if (k < 0) bad = "k < 0";
  else if (k > 64) bad = "k > 64";
  else if (k > 0 && ldc < f->S->n) bad = "ldc < n";
  if (int rc = enter(f, what, bad, SINGLE | WAIT_IGNORE | BATCH)) return rc;
  const int rc = f->eng->set_constraints_batch(k, c, ldc, dev);
  // (-20 with the constraints still held: a member is not positive definite; without: a dependent row, the engine's
  // message names it)
  if (rc == SPLLT_ERROR_NOT_POSDEF && f->eng->constraints_batch_k() > 0)
    return batch_mult_leave(f, what, rc, "the members that are not positive definite hold no constraints, the others do");
  return leave(f, rc);
}

int spllt_hip_set_constraints_batch(void* fkeep, int k, const double* c_host, int64_t ldc) {
  return set_constraints_batch_impl("spllt_hip_set_constraints_batch", fkeep, k, c_host, ldc, false);
}

int spllt_hip_set_constraints_batch_dev(void* fkeep, int k, const double* c_dev, int64_t ldc) {
  return set_constraints_batch_impl("spllt_hip_set_constraints_batch_dev", fkeep, k, c_dev, ldc, true);
}

static const char* const kNoBatchConstraints = "no constraints are set on this batch (spllt_hip_set_constraints_batch)";

// the rungs of constrain_impl for the arguments, of solve_many_batch_impl / sample_batch_impl for the handle
static int constrain_batch_impl(const char* what, int op, void* fkeep, int nvec, double* x, int64_t ldx, const double* e,
                                int64_t lde, double* lambda, int64_t ldl, bool dev, uint64_t seed, uint64_t first,
                                uint32_t stream0, int stream_step, const double* mean, int64_t ldmean) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!analysed(f)) return SPLLT_ERROR_PARAMETER;
  const char* bad = vectors_bad(f, nvec, x, ldx, 0);
  const int k = f->eng ? f->eng->constraints_batch_k() : 0;   // (0: refused below, once the ladder is through)
  if (!bad && k > 0 && e && lde != 0 && lde < k) bad = "lde is neither 0 nor >= k";
  if (!bad && k > 0 && lambda && ldl < k) bad = "ldl < k";
  if (!bad && (stream_step < 0 || stream_step > 1)) bad = "stream_step is not 0 (common noise) or 1 (a stream per member)";
  if (!bad && mean && ldmean != 0 && ldmean < f->S->n) bad = "ldmean is neither 0 (one mean for all members) nor >= n";
  if (int rc = enter(f, what, bad, SINGLE | WAIT_IGNORE | BATCH)) return rc;
  if (nvec == 0) return 0;
  if (f->eng->constraints_batch_k() <= 0) return fail(f, what, kNoBatchConstraints);
  f->eng->set_batch_blocked_solve(f->batch_blocked);
  const int rc = f->eng->constrain_batch(op, nvec, x, ldx, e, e ? lde : 0, lambda, ldl, dev, seed, first, stream0, stream_step,
                                         mean, ldmean);
  // (-20 with the constraints gone: the rebuild for a later batch met a dependent row, the engine's message names it)
  if (rc == SPLLT_ERROR_NOT_POSDEF && f->eng->constraints_batch_k() <= 0) return leave(f, rc);
  return batch_mult_leave(f, what, rc,
                          op == Engine::CN_SAMPLE ? "the samples of the members that are not positive definite are NaN"
                                                  : "the vectors of the members that are not positive definite were left "
                                                    "unchanged");
}

int spllt_hip_constrain_batch(void* fkeep, int nvec, double* x_host, int64_t ldx, const double* e_host, int64_t lde,
                              double* lambda_host, int64_t ldl) {
  return constrain_batch_impl("spllt_hip_constrain_batch", Engine::CN_CORRECT, fkeep, nvec, x_host, ldx, e_host, lde,
                              lambda_host, ldl, false, 0, 0, 0, 1, nullptr, 0);
}

int spllt_hip_constrain_batch_dev(void* fkeep, int nvec, double* x_dev, int64_t ldx, const double* e_dev, int64_t lde,
                                  double* lambda_dev, int64_t ldl) {
  return constrain_batch_impl("spllt_hip_constrain_batch_dev", Engine::CN_CORRECT, fkeep, nvec, x_dev, ldx, e_dev, lde,
                              lambda_dev, ldl, true, 0, 0, 0, 1, nullptr, 0);
}

int spllt_hip_solve_constrained_batch(void* fkeep, int nrhs, double* x_host, int64_t ldx, const double* e_host, int64_t lde,
                                      double* lambda_host, int64_t ldl) {
  return constrain_batch_impl("spllt_hip_solve_constrained_batch", Engine::CN_SOLVE, fkeep, nrhs, x_host, ldx, e_host, lde,
                              lambda_host, ldl, false, 0, 0, 0, 1, nullptr, 0);
}

int spllt_hip_solve_constrained_batch_dev(void* fkeep, int nrhs, double* x_dev, int64_t ldx, const double* e_dev,
                                          int64_t lde, double* lambda_dev, int64_t ldl) {
  return constrain_batch_impl("spllt_hip_solve_constrained_batch_dev", Engine::CN_SOLVE, fkeep, nrhs, x_dev, ldx, e_dev, lde,
                              lambda_dev, ldl, true, 0, 0, 0, 1, nullptr, 0);
}

int spllt_hip_sample_constrained_batch(void* fkeep, int nsamp, double* x_host, int64_t ldx, uint64_t seed,
                                       uint64_t first_sample, uint32_t stream0, int stream_step, const double* mean_host,
                                       int64_t ldmean, const double* e_host) {
  return constrain_batch_impl("spllt_hip_sample_constrained_batch", Engine::CN_SAMPLE, fkeep, nsamp, x_host, ldx, e_host, 0,
                              nullptr, 0, false, seed, first_sample, stream0, stream_step, mean_host, ldmean);
}

int spllt_hip_sample_constrained_batch_dev(void* fkeep, int nsamp, double* x_dev, int64_t ldx, uint64_t seed,
                                           uint64_t first_sample, uint32_t stream0, int stream_step, const double* mean_dev,
                                           int64_t ldmean, const double* e_dev) {
  return constrain_batch_impl("spllt_hip_sample_constrained_batch_dev", Engine::CN_SAMPLE, fkeep, nsamp, x_dev, ldx, e_dev,
                              0, nullptr, 0, true, seed, first_sample, stream0, stream_step, mean_dev, ldmean);
}

// the rungs of spllt_hip_inverse_diag_batch, then "no constraints"
int spllt_hip_inverse_diag_constrained_batch(void* fkeep, double* out, int64_t ldout) {
  const char* what = "spllt_hip_inverse_diag_constrained_batch";
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!analysed(f)) return SPLLT_ERROR_PARAMETER;
  const char* bad = !out ? "the output array is null" : ldout < f->S->n ? "ldout < n" : nullptr;
  if (int rc = enter(f, what, bad, SINGLE | WAIT_IGNORE | BATCH | BATCH_INVERSE)) return rc;
  if (f->eng->constraints_batch_k() <= 0) return fail(f, what, kNoBatchConstraints);
  const int rc = f->eng->inverse_diag_constrained_batch(out, ldout);
  if (rc == SPLLT_ERROR_NOT_POSDEF && f->eng->constraints_batch_k() <= 0) return leave(f, rc);
  return batch_mult_leave(f, what, rc, "the rows of the members that are not positive definite are NaN");
}

int spllt_hip_constraints_batch_info(void* fkeep, int64_t out[4], double* stat, int64_t ldstat) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!f || !f->S || !out || (stat && ldstat < 2)) return SPLLT_ERROR_PARAMETER;
  for (int i = 0; i < 4; ++i) out[i] = 0;
  if (!f->eng || f->dead) return 0;
  if (stat)
    for (int b = 0; b < f->eng->batch_count(); ++b) stat[(int64_t)b * ldstat] = stat[(int64_t)b * ldstat + 1] = 0.0;
  f->eng->constraints_batch_info(out, stat, ldstat);
  return 0;
}

// ---- low-rank update / downdate of the factor ------------------------------------------------------
int64_t spllt_hip_updown_plan(void* fkeep, int k, const int* wptr, const int* wrow, int32_t* bcols, int64_t capacity) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!analysed(f)) return SPLLT_ERROR_PARAMETER;
  std::vector<int> plan;
  std::string why;
  if (build_updown_plan(*f->S, k, wptr, wrow, plan, nullptr, &why)) return fail(f, "spllt_hip_updown_plan", why);
  return Out{bcols, capacity}.elems(plan);
}

int spllt_hip_updown(void* fkeep, int k, const int* wptr, const int* wrow, const double* wval, int sign) {
  const char* what = "spllt_hip_updown";
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!analysed(f)) return SPLLT_ERROR_PARAMETER;
  std::vector<int> plan, first;
  std::string why;
  const char* bad = nullptr;
  if (sign != 1 && sign != -1) bad = "sign is not +1 or -1";
  else if (k > 0 && !wval) bad = "the array of values is null";
  else if (build_updown_plan(*f->S, k, wptr, wrow, plan, &first, &why)) bad = why.c_str();
  for (int e = 0; !bad && k > 0 && e < wptr[k] - 1; ++e)
    if (!std::isfinite(wval[e])) bad = "a value of W is not finite";
  // (without a factorization the engine is created only to tell "no device" from "nothing factorized")
  if (int rc = enter(f, what, bad, SINGLE | WAIT | ENGINE | FACTORED)) return rc;
  const int rc = f->eng->updown(k, wptr, wrow, wval, sign, plan, first);
  f->hostL_valid = false;
  ++f->serial[0];   // (a failed downdate has changed the factor as well: it is invalid now)
  leave(f, rc);
  if (rc == SPLLT_ERROR_NOT_POSDEF) std::fprintf(stderr, "spllt-hip: %s\n", f->last_error.c_str());
  return rc;
}

int spllt_hip_updown_time(void* fkeep, double* device_ms) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!f || !f->S || !device_ms) return SPLLT_ERROR_PARAMETER;
  *device_ms = f->eng ? f->eng->updown_device_ms() : 0.0;
  return 0;
}

int spllt_hip_updown_info(void* fkeep, int64_t out[4]) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!f || !f->S || !out) return SPLLT_ERROR_PARAMETER;
  for (int i = 0; i < 4; ++i) out[i] = f->eng ? f->eng->updown_info()[i] : 0;
  return 0;
}

// ---- low-rank update / downdate of the factors of a batch (spllt_hip_updown_batch.h) ----------------
static int updown_batch_impl(void* fkeep, int k, const int* wptr, const int* wrow, const double* wval, int64_t ldw,
                             int sign, bool dev, const char* what) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!analysed(f)) return SPLLT_ERROR_PARAMETER;
  std::vector<int> plan, first;
  std::string why;
  const char* bad = nullptr;
  // (the argument checks of spllt_hip_updown, in its order, then the member stride)
  if (sign != 1 && sign != -1) bad = "sign is not +1 or -1";
  else if (k > 0 && !wval) bad = "the array of values is null";
  else if (build_updown_plan(*f->S, k, wptr, wrow, plan, &first, &why)) bad = why.c_str();
  else if (k > 0 && ldw < (int64_t)wptr[k] - 1) bad = "ldw < wptr[k] - 1";
  const int nb = (f->eng && !f->dead) ? f->eng->batch_count() : 0;
  for (int b = 0; !bad && !dev && k > 0 && b < nb; ++b)
    for (int e = wptr[0] - 1; !bad && e < wptr[k] - 1; ++e)
      if (!std::isfinite(wval[(int64_t)b * ldw + e])) bad = "a value of W is not finite";
  if (int rc = enter(f, what, bad, SINGLE | WAIT_IGNORE | BATCH)) return rc;
  const int rc = f->eng->updown_batch(k, wptr, wrow, wval, ldw, dev, sign, plan, first);
  if (!plan.empty() && rc != SPLLT_ERROR_ALLOCATION && rc != SPLLT_ERROR_PARAMETER && rc != SPLLT_ERROR_UNIMPLEMENTED)
    ++f->serial[1];   // (the call reached the device: the members' factors have changed, a failed one included)
  if (rc == SPLLT_ERROR_NOT_POSDEF) {   // -20 of the batch calls
    const bool fresh = f->eng->updown_batch_info()[5] > 0;   // (a downdate of THIS call failed: said aloud, as spllt_hip_updown does)
    fail(f, what, fresh ? f->eng->feature_error()
                        : std::string("the members that are not positive definite were skipped, the others are "
                                      "modified (spllt_hip_batch_status)"), rc);
    if (fresh) std::fprintf(stderr, "spllt-hip: %s\n", f->last_error.c_str());
    return rc;
  }
  return leave(f, rc);
}

int spllt_hip_updown_batch(void* fkeep, int k, const int* wptr, const int* wrow, const double* wval_host, int64_t ldw,
                           int sign) {
  return updown_batch_impl(fkeep, k, wptr, wrow, wval_host, ldw, sign, false, "spllt_hip_updown_batch");
}

int spllt_hip_updown_batch_dev(void* fkeep, int k, const int* wptr, const int* wrow, const double* wval_dev, int64_t ldw,
                               int sign) {
  return updown_batch_impl(fkeep, k, wptr, wrow, wval_dev, ldw, sign, true, "spllt_hip_updown_batch_dev");
}

int spllt_hip_updown_batch_info(void* fkeep, int64_t out[6]) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!f || !f->S || !out) return SPLLT_ERROR_PARAMETER;
  for (int i = 0; i < 6; ++i) out[i] = (f->eng && !f->dead) ? f->eng->updown_batch_info()[i] : 0;
  return 0;
}

int spllt_hip_updown_batch_time(void* fkeep, double* device_ms) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!f || !f->S || !device_ms) return SPLLT_ERROR_PARAMETER;
  *device_ms = (f->eng && !f->dead) ? f->eng->updown_batch_device_ms() : 0.0;
  return 0;
}

// ---- sparse right-hand sides and selected outputs --------------------------------------------------
// the argument rungs of the sparse solves of handle and batch: the first that fails (*why holds its text when it is
// check_sparse_columns'), or null.  out: the output array, ld against the number of wanted entries (gram: against k)
static const char* sparse_args_bad(const Fkeep* f, int k, const int* bptr, const int* brow, const double* bval, int nsel,
                                   const int* sel, const void* out, int64_t ld, int64_t ld_min, int job, std::string* why) {
  if (!out) return "the output array is null";
  if (job < 0 || job > 2) return "job is not 0, 1 or 2";
  if (check_sparse_columns(*f->S, k, bptr, brow, nsel, sel, why)) return why->c_str();
  if (k > 0 && bptr[k] > bptr[0] && !bval) return "the array of values is null";
  if (ld < ld_min) return "the leading dimension of the output is too small";
  return nullptr;
}

static int solve_sparse_enter(Fkeep* f, const char* what, int k, const int* bptr, const int* brow, const double* bval,
                              int nsel, const int* sel, const void* out, int64_t ld, int64_t ld_min, int job) {
  if (!analysed(f)) return SPLLT_ERROR_PARAMETER;
  std::string why;
  const char* bad = sparse_args_bad(f, k, bptr, brow, bval, nsel, sel, out, ld, ld_min, job, &why);
  // (without a factorization the engine is created only to tell "no device" from "nothing factorized")
  return enter(f, what, bad, SINGLE | WAIT | ENGINE | FACTORED);
}

static int solve_sparse_impl(const char* what, void* fkeep, int k, const int* bptr, const int* brow, const double* bval,
                             int nsel, const int* sel, double* x, int64_t ldx, int job, bool dev) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!sel || nsel < 0) { sel = nullptr; nsel = -1; }
  const int64_t nout = !analysed(f) ? 0 : (sel ? nsel : f->S->n);
  if (int rc = solve_sparse_enter(f, what, k, bptr, brow, bval, nsel, sel, x, ldx, nout, job)) return rc;
  return leave(f, f->eng->solve_sparse(k, bptr, brow, bval, nsel, sel, x, ldx, job, dev));
}

int spllt_hip_solve_sparse(void* fkeep, int k, const int* bptr, const int* brow, const double* bval, int nsel,
                           const int* sel, double* x_host, int64_t ldx, int job) {
  return solve_sparse_impl("spllt_hip_solve_sparse", fkeep, k, bptr, brow, bval, nsel, sel, x_host, ldx, job, false);
}

int spllt_hip_solve_sparse_dev(void* fkeep, int k, const int* bptr, const int* brow, const double* bval, int nsel,
                               const int* sel, double* x_dev, int64_t ldx, int job) {
  return solve_sparse_impl("spllt_hip_solve_sparse_dev", fkeep, k, bptr, brow, bval, nsel, sel, x_dev, ldx, job, true);
}

int spllt_hip_gram_sparse(void* fkeep, int k, const int* bptr, const int* brow, const double* bval, double* g_host,
                          int64_t ldg) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (int rc = solve_sparse_enter(f, "spllt_hip_gram_sparse", k, bptr, brow, bval, -1, nullptr, g_host, ldg, k, 0))
    return rc;
  return leave(f, f->eng->gram_sparse(k, bptr, brow, bval, g_host, ldg));
}

int spllt_hip_solve_sparse_plan(void* fkeep, int k, const int* bptr, const int* brow, int nsel, const int* sel, int job,
                                int32_t* fwd_bcols, int64_t fwd_cap, int32_t* bwd_bcols, int64_t bwd_cap,
                                int64_t counts[2]) {
  const char* what = "spllt_hip_solve_sparse_plan";
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!analysed(f)) return SPLLT_ERROR_PARAMETER;
  if (!counts) return fail(f, what, "counts is null");
  if (job < 0 || job > 2) return fail(f, what, "job is not 0, 1 or 2");
  if (!sel || nsel < 0) { sel = nullptr; nsel = -1; }
  std::string why;
  if (check_sparse_columns(*f->S, k, bptr, brow, nsel, sel, &why)) return fail(f, what, why);
  SolveSparsePlan P;
  build_solve_sparse_plan(*f->S, 0, k, bptr, brow, nsel, sel, job, P);
  counts[0] = Out{fwd_bcols, fwd_cap}.elems(P.fwd);
  counts[1] = Out{bwd_bcols, bwd_cap}.elems(P.bwd);
  return 0;
}

int spllt_hip_solve_sparse_info(void* fkeep, int64_t out[6]) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!f || !f->S || !out) return SPLLT_ERROR_PARAMETER;
  for (int i = 0; i < 6; ++i) out[i] = f->eng ? f->eng->solve_sparse_info()[i] : 0;
  return 0;
}

// ---- sparse right-hand sides for the members of a batch (spllt_hip_solve_sparse_batch.h) ------------
// the argument rungs of sparse_args_bad, then the member stride; the handle rungs of solve_many_batch_impl, then
// the reproducible switch
static int solve_sparse_batch_enter(Fkeep* f, const char* what, int k, const int* bptr, const int* brow,
                                    const double* bval, int64_t ldb, int nsel, const int* sel, const void* out, int64_t ld,
                                    int64_t ld_min, int job) {
  if (!analysed(f)) return SPLLT_ERROR_PARAMETER;
  std::string why;
  const char* bad = sparse_args_bad(f, k, bptr, brow, bval, nsel, sel, out, ld, ld_min, job, &why);
  if (!bad && k > 0 && ldb != 0 && ldb < (int64_t)bptr[k] - 1)
    bad = "ldb is neither 0 (one set of values for all members) nor >= bptr[k] - 1";
  if (int rc = enter(f, what, bad, SINGLE | WAIT_IGNORE | BATCH)) return rc;
  if (f->eng->batch_reproducible())
    return fail(f, what, "not available while the reproducible batch is switched on (spllt_hip_set_batch_reproducible): "
                         "the filtered sweeps run the kernels that add with atomics", SPLLT_ERROR_UNIMPLEMENTED);
  return 0;
}

static int solve_sparse_batch_impl(const char* what, void* fkeep, int k, const int* bptr, const int* brow,
                                   const double* bval, int64_t ldb, int nsel, const int* sel, double* x, int64_t ldx, int job,
                                   bool dev) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!sel || nsel < 0) { sel = nullptr; nsel = -1; }
  const int64_t nout = !analysed(f) ? 0 : (sel ? nsel : f->S->n);
  if (int rc = solve_sparse_batch_enter(f, what, k, bptr, brow, bval, ldb, nsel, sel, x, ldx, nout, job)) return rc;
  return batch_mult_leave(f, what, f->eng->solve_sparse_batch(k, bptr, brow, bval, ldb, nsel, sel, x, ldx, job, dev),
                          "the outputs of the members that are not positive definite are NaN");
}

int spllt_hip_solve_sparse_batch(void* fkeep, int k, const int* bptr, const int* brow, const double* bval, int64_t ldb,
                                 int nsel, const int* sel, double* x_host, int64_t ldx, int job) {
  return solve_sparse_batch_impl("spllt_hip_solve_sparse_batch", fkeep, k, bptr, brow, bval, ldb, nsel, sel, x_host, ldx,
                                 job, false);
}

int spllt_hip_solve_sparse_batch_dev(void* fkeep, int k, const int* bptr, const int* brow, const double* bval, int64_t ldb,
                                     int nsel, const int* sel, double* x_dev, int64_t ldx, int job) {
  return solve_sparse_batch_impl("spllt_hip_solve_sparse_batch_dev", fkeep, k, bptr, brow, bval, ldb, nsel, sel, x_dev, ldx,
                                 job, true);
}

static int gram_sparse_batch_impl(const char* what, void* fkeep, int k, const int* bptr, const int* brow, const double* bval,
                                  int64_t ldb, double* g, int64_t ldg, bool dev) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (int rc = solve_sparse_batch_enter(f, what, k, bptr, brow, bval, ldb, -1, nullptr, g, ldg, k, 0)) return rc;
  return batch_mult_leave(f, what, f->eng->gram_sparse_batch(k, bptr, brow, bval, ldb, g, ldg, dev),
                          "the outputs of the members that are not positive definite are NaN");
}

int spllt_hip_gram_sparse_batch(void* fkeep, int k, const int* bptr, const int* brow, const double* bval, int64_t ldb,
                                double* g_host, int64_t ldg) {
  return gram_sparse_batch_impl("spllt_hip_gram_sparse_batch", fkeep, k, bptr, brow, bval, ldb, g_host, ldg, false);
}

int spllt_hip_gram_sparse_batch_dev(void* fkeep, int k, const int* bptr, const int* brow, const double* bval, int64_t ldb,
                                    double* g_dev, int64_t ldg) {
  return gram_sparse_batch_impl("spllt_hip_gram_sparse_batch_dev", fkeep, k, bptr, brow, bval, ldb, g_dev, ldg, true);
}

int spllt_hip_solve_sparse_batch_info(void* fkeep, int64_t out[8]) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!f || !f->S || !out) return SPLLT_ERROR_PARAMETER;
  for (int i = 0; i < 8; ++i) out[i] = (f->eng && !f->dead) ? f->eng->solve_sparse_batch_info()[i] : 0;
  return 0;
}

// ---- readers of the batch ------------------------------------------------------
int spllt_hip_get_factor_batch(void* fkeep, int member, double* out, int64_t count) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  const char* what = "spllt_hip_get_factor_batch";
  const char* bad = !out ? "the output array is null" : count < 0 ? "count < 0" : nullptr;
  if (int rc = enter(f, what, bad, SINGLE | WAIT_IGNORE | BATCH)) return rc;
  if (member < 0 || member >= f->eng->batch_count()) return fail(f, what, "member is not in [0, nbatch)");
  return leave(f, f->eng->download_batch(member, out, count));
}

double* spllt_hip_device_factor_batch(void* fkeep, int64_t* member_stride) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (member_stride) *member_stride = 0;
  if (!f || !f->eng || f->dead) return nullptr;
  return f->eng->device_batch(member_stride);
}

int spllt_hip_log_det_batch(void* fkeep, double* out) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (int rc = enter(f, "spllt_hip_log_det_batch", out ? nullptr : "the output array is null", SINGLE | WAIT_IGNORE | BATCH))
    return rc;
  return leave(f, f->eng->log_det_batch(out));
}

int spllt_hip_batch_launches(void* fkeep) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!f) return SPLLT_ERROR_PARAMETER;
  return (f->eng && !f->dead) ? f->eng->batch_launches() : 0;
}

// ---- batched selected inversion ------------------------------------------------
int spllt_hip_selected_inverse_batch(void* fkeep) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  const char* what = "spllt_hip_selected_inverse_batch";
  if (int rc = enter(f, what, nullptr, SINGLE | WAIT_IGNORE | BATCH)) return rc;
  int rc = f->eng->selected_inverse_batch();
  if (rc == SPLLT_ERROR_NOT_POSDEF)   // -20 of the batch calls
    return fail(f, what, "the members that are not positive definite were skipped, the others are inverted "
                         "(spllt_hip_batch_status)", rc);
  return leave(f, rc);
}

int spllt_hip_get_inverse_batch(void* fkeep, int member, double* out, int64_t count) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  const char* what = "spllt_hip_get_inverse_batch";
  const char* bad = !out ? "the output array is null" : count < 0 ? "count < 0" : nullptr;
  if (int rc = enter(f, what, bad, SINGLE | WAIT_IGNORE | BATCH | BATCH_INVERSE)) return rc;
  if (member < 0 || member >= f->eng->batch_count()) return fail(f, what, "member is not in [0, nbatch)");
  if (f->eng->batch_flags()[(size_t)member] != INT_MAX)
    return fail(f, what, "member " + std::to_string(member) + " is not positive definite: it has no inverse "
                         "(spllt_hip_batch_status)", SPLLT_ERROR_NOT_POSDEF);
  return leave(f, f->eng->download_inverse_batch(member, out, count));
}

double* spllt_hip_device_inverse_batch(void* fkeep, int64_t* member_stride) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (member_stride) *member_stride = 0;
  if (!f || !f->eng || f->dead) return nullptr;
  return f->eng->device_inverse_batch(member_stride);
}

// one row of `width` values per member; ld_name: what a short leading dimension is called
static int batch_rows_impl(const char* what, void* fkeep, double* out, int64_t ldout, bool nnz_wide, const char* ld_name,
                           int (Engine::*fn)(double*, int64_t)) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!analysed(f)) return SPLLT_ERROR_PARAMETER;
  const char* bad = !out ? "the output array is null" : ldout < (nnz_wide ? f->S->nnzA : f->S->n) ? ld_name : nullptr;
  if (int rc = enter(f, what, bad, SINGLE | WAIT_IGNORE | BATCH | BATCH_INVERSE)) return rc;
  return leave(f, (f->eng.get()->*fn)(out, ldout));
}

int spllt_hip_inverse_diag_batch(void* fkeep, double* out, int64_t ldout) {
  return batch_rows_impl("spllt_hip_inverse_diag_batch", fkeep, out, ldout, false, "ldout < n", &Engine::inverse_diag_batch);
}

int spllt_hip_inverse_on_pattern_batch(void* fkeep, double* out, int64_t ldout) {
  return batch_rows_impl("spllt_hip_inverse_on_pattern_batch", fkeep, out, ldout, true, "ldout < nnz",
                         &Engine::inverse_on_pattern_batch);
}

int spllt_hip_inverse_on_pattern_batch_dev(void* fkeep, double* out_dev, int64_t ldout) {
  return batch_rows_impl("spllt_hip_inverse_on_pattern_batch_dev", fkeep, out_dev, ldout, true, "ldout < nnz",
                         &Engine::inverse_on_pattern_batch_dev);
}

int spllt_hip_batch_selinv_launches(void* fkeep) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!f) return SPLLT_ERROR_PARAMETER;
  return (f->eng && !f->dead) ? f->eng->batch_selinv_launches() : 0;
}

// ---- selected inversion ---------------------------------------------------
// (a null output array of these older calls is refused without a message: bad = "")
int spllt_hip_selected_inverse(void* fkeep) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (int rc = enter(f, "spllt_hip_selected_inverse", nullptr, SINGLE_F | WAIT | FACTOR)) return rc;
  return leave(f, f->eng->selected_inverse());
}

int spllt_hip_get_inverse(void* fkeep, double* out, int64_t count) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (int rc = enter(f, "spllt_hip_get_inverse", out ? nullptr : "", SINGLE_F | WAIT | FACTOR | INVERSE)) return rc;
  return leave(f, f->eng->download_inverse(out, count));
}

double* spllt_hip_device_inverse(void* fkeep) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  return (f && f->eng && !f->eng->pending()) ? f->eng->device_Z() : nullptr;
}

int spllt_hip_inverse_diag(void* fkeep, double* out, int n) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (int rc = enter(f, "spllt_hip_inverse_diag", out ? nullptr : "", SINGLE_F | WAIT | FACTOR | INVERSE)) return rc;
  if (n != f->S->n)
    return fail(f, "spllt_hip_inverse_diag", "n = " + std::to_string(n) + " does not match the analysed order " +
                                             std::to_string(f->S->n));
  return leave(f, f->eng->inverse_diag(out, n));
}

static int inverse_on_pattern_impl(const char* what, void* fkeep, double* out, int (Engine::*fn)(double*)) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (int rc = enter(f, what, out ? nullptr : "", SINGLE_F | WAIT | FACTOR | INVERSE)) return rc;
  return leave(f, (f->eng.get()->*fn)(out));
}

int spllt_hip_inverse_on_pattern(void* fkeep, double* out) {
  return inverse_on_pattern_impl("spllt_hip_inverse_on_pattern", fkeep, out, &Engine::inverse_on_pattern);
}

int spllt_hip_inverse_on_pattern_dev(void* fkeep, double* out_dev) {
  return inverse_on_pattern_impl("spllt_hip_inverse_on_pattern_dev", fkeep, out_dev, &Engine::inverse_on_pattern_dev);
}

int spllt_hip_log_det(void* fkeep, double* out) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (int rc = enter(f, "spllt_hip_log_det", out ? nullptr : "", SINGLE_F | WAIT | FACTOR)) return rc;
  return leave(f, f->eng->log_det(out));
}

int64_t spllt_hip_factor_serial(const void* fkeep, int which) {
  const Fkeep* f = static_cast<const Fkeep*>(fkeep);
  if (!f || which < 0 || which > 1) return SPLLT_ERROR_PARAMETER;
  return f->serial[which];
}

// ---- sampled outer product on the analysed pattern ---------------------------------------------------
// the operation needs the analysis only, so an engine is created when the handle has none yet
static int pattern_outer_impl(const char* what, void* fkeep, int nbatch, int nvec, const double* u, int64_t ldu,
                              const double* v, int64_t ldv, double alpha, double* out, int64_t ldout, bool dev) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!analysed(f)) return SPLLT_ERROR_PARAMETER;
  const char* bad = nullptr;
  if (!u || !v) bad = "a vector array is null";
  else if (!out) bad = "the output array is null";
  else if (nbatch < 0) bad = "nbatch < 0";
  else if (nvec < 0) bad = "nvec < 0";
  else if (ldu < f->S->n) bad = "ldu < n";
  else if (ldv < f->S->n) bad = "ldv < n";
  else if (ldout < f->S->nnzA) bad = "ldout < nnz";
  if (int rc = enter(f, what, bad, SINGLE | WAIT_IGNORE | ENGINE | (nbatch == 0 ? EMPTY : 0))) return done(rc);
  return leave(f, f->eng->pattern_outer(nbatch, nvec, u, ldu, v, ldv, alpha, out, ldout, dev));
}

int spllt_hip_pattern_outer(void* fkeep, int nvec, const double* u_host, int64_t ldu, const double* v_host, int64_t ldv,
                            double alpha, double* out_host) {
  const Fkeep* f = static_cast<const Fkeep*>(fkeep);
  return pattern_outer_impl("spllt_hip_pattern_outer", fkeep, 1, nvec, u_host, ldu, v_host, ldv, alpha, out_host,
                            analysed(f) ? f->S->nnzA : 0, false);
}

int spllt_hip_pattern_outer_dev(void* fkeep, int nvec, const double* u_dev, int64_t ldu, const double* v_dev, int64_t ldv,
                                double alpha, double* out_dev) {
  const Fkeep* f = static_cast<const Fkeep*>(fkeep);
  return pattern_outer_impl("spllt_hip_pattern_outer_dev", fkeep, 1, nvec, u_dev, ldu, v_dev, ldv, alpha, out_dev,
                            analysed(f) ? f->S->nnzA : 0, true);
}

int spllt_hip_pattern_outer_batch_dev(void* fkeep, int nbatch, int nvec, const double* u_dev, int64_t ldu,
                                      const double* v_dev, int64_t ldv, double alpha, double* out_dev, int64_t ldout) {
  return pattern_outer_impl("spllt_hip_pattern_outer_batch_dev", fkeep, nbatch, nvec, u_dev, ldu, v_dev, ldv, alpha,
                            out_dev, ldout, true);
}

// ---- reverse-mode derivative of the factor --------------------------------------------------------
constexpr unsigned kAdjoint = SINGLE | WAIT | FACTOR;

static int fadj_seed_impl(const char* what, void* fkeep, int nvec, const double* a, const double* b, int64_t ld,
                          double alpha, int accumulate, int order_flags, bool dev) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!analysed(f)) return SPLLT_ERROR_PARAMETER;
  const char* bad = nullptr;
  if (!a || !b) bad = "a vector array is null";
  else if (nvec < 0) bad = "nvec < 0";
  else if (ld < f->S->n) bad = "ld < n";
  else if (accumulate < 0 || accumulate > 1) bad = "accumulate is not 0 or 1";
  else if (order_flags < 0 || order_flags > 3) bad = "order_flags is not 0 .. 3";
  if (int rc = enter(f, what, bad, kAdjoint)) return rc;
  const int rc = f->eng->fadj_seed(nvec, a, b, ld, alpha, accumulate != 0, order_flags, dev);
  if (rc == SPLLT_ERROR_PARAMETER && f->eng->feature_error().empty())
    f->last_error = std::string(what) + ": the factor is not available";
  return leave(f, rc);
}

int spllt_hip_factor_adjoint_seed_dev(void* fkeep, int nvec, const double* a_dev, const double* b_dev, int64_t ld,
                                      double alpha, int accumulate, int order_flags) {
  return fadj_seed_impl("spllt_hip_factor_adjoint_seed_dev", fkeep, nvec, a_dev, b_dev, ld, alpha, accumulate,
                        order_flags, true);
}

int spllt_hip_factor_adjoint_seed(void* fkeep, int nvec, const double* a_host, const double* b_host, int64_t ld,
                                  double alpha, int accumulate, int order_flags) {
  return fadj_seed_impl("spllt_hip_factor_adjoint_seed", fkeep, nvec, a_host, b_host, ld, alpha, accumulate,
                        order_flags, false);
}

int spllt_hip_set_factor_adjoint(void* fkeep, const double* host_arena, int64_t count) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!analysed(f)) return SPLLT_ERROR_PARAMETER;
  const char* bad = !host_arena ? "the arena is null" : count < f->S->arena ? "count is smaller than the factor arena" : nullptr;
  if (int rc = enter(f, "spllt_hip_set_factor_adjoint", bad, kAdjoint)) return rc;
  return leave(f, f->eng->fadj_upload(host_arena, count));
}

int spllt_hip_get_factor_adjoint(void* fkeep, double* out, int64_t count) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  const char* what = "spllt_hip_get_factor_adjoint";
  if (int rc = enter(f, what, out ? nullptr : "the output array is null", kAdjoint)) return rc;
  if (f->eng->fadj_state() == Engine::FADJ_UNSEEDED)
    return fail(f, what, "no factor adjoint of the current factor (seed it after every factorization)");
  return leave(f, f->eng->fadj_download(out, count));
}

double* spllt_hip_device_factor_adjoint(void* fkeep) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  return (f && f->eng && !f->eng->pending()) ? f->eng->device_G() : nullptr;
}

static int fadj_sweep_impl(const char* what, void* fkeep, double* gval, bool dev) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (int rc = enter(f, what, gval ? nullptr : "the gradient array is null", kAdjoint)) return rc;
  return leave(f, f->eng->fadj_sweep(gval, dev));
}

int spllt_hip_factor_adjoint_dev(void* fkeep, double* gval_dev) {
  return fadj_sweep_impl("spllt_hip_factor_adjoint_dev", fkeep, gval_dev, true);
}

int spllt_hip_factor_adjoint(void* fkeep, double* gval_host) {
  return fadj_sweep_impl("spllt_hip_factor_adjoint", fkeep, gval_host, false);
}

// ---- reverse-mode derivative of the factors of a batch (spllt_hip_batch_adjoint.h) ------------------
constexpr unsigned kBatchAdjoint = SINGLE | WAIT_IGNORE | BATCH;

static int bfadj_seed_impl(const char* what, void* fkeep, int nvec, const double* a, const double* b, int64_t ld,
                           double alpha, int accumulate, int order_flags, bool dev) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!analysed(f)) return SPLLT_ERROR_PARAMETER;
  const char* bad = nullptr;
  if (!a || !b) bad = "a vector array is null";
  else if (nvec < 0) bad = "nvec < 0";
  else if (ld < f->S->n) bad = "ld < n";
  else if (accumulate < 0 || accumulate > 1) bad = "accumulate is not 0 or 1";
  else if (order_flags < 0 || order_flags > 3) bad = "order_flags is not 0 .. 3";
  if (int rc = enter(f, what, bad, kBatchAdjoint)) return rc;
  return leave(f, f->eng->fadj_seed_batch(nvec, a, b, ld, alpha, accumulate != 0, order_flags, dev));
}

int spllt_hip_factor_adjoint_seed_batch_dev(void* fkeep, int nvec, const double* a_dev, const double* b_dev, int64_t ld,
                                            double alpha, int accumulate, int order_flags) {
  return bfadj_seed_impl("spllt_hip_factor_adjoint_seed_batch_dev", fkeep, nvec, a_dev, b_dev, ld, alpha, accumulate,
                         order_flags, true);
}

int spllt_hip_factor_adjoint_seed_batch(void* fkeep, int nvec, const double* a_host, const double* b_host, int64_t ld,
                                        double alpha, int accumulate, int order_flags) {
  return bfadj_seed_impl("spllt_hip_factor_adjoint_seed_batch", fkeep, nvec, a_host, b_host, ld, alpha, accumulate,
                         order_flags, false);
}

int spllt_hip_set_factor_adjoint_batch(void* fkeep, const double* host_arenas, int64_t ldarena) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!analysed(f)) return SPLLT_ERROR_PARAMETER;
  const char* bad = !host_arenas ? "the arenas are null" : ldarena < f->S->arena ? "ldarena is smaller than the factor arena" : nullptr;
  if (int rc = enter(f, "spllt_hip_set_factor_adjoint_batch", bad, kBatchAdjoint)) return rc;
  return leave(f, f->eng->fadj_upload_batch(host_arenas, ldarena));
}

int spllt_hip_get_factor_adjoint_batch(void* fkeep, int member, double* out, int64_t count) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  const char* what = "spllt_hip_get_factor_adjoint_batch";
  const char* bad = !out ? "the output array is null" : count < 0 ? "count < 0" : nullptr;
  if (int rc = enter(f, what, bad, kBatchAdjoint)) return rc;
  if (f->eng->fadj_batch_state() == Engine::FADJ_UNSEEDED)
    return fail(f, what, "no factor adjoint of the current batch (seed it after every spllt_hip_factor_batch)");
  if (member < 0 || member >= f->eng->batch_count()) return fail(f, what, "member is not in [0, nbatch)");
  return leave(f, f->eng->fadj_download_batch(member, out, count));
}

double* spllt_hip_device_factor_adjoint_batch(void* fkeep, int64_t* member_stride) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (member_stride) *member_stride = 0;
  if (!f || !f->eng || f->dead || f->eng->pending()) return nullptr;
  return f->eng->device_G_batch(member_stride);
}

static int bfadj_sweep_impl(const char* what, void* fkeep, double* gval, int64_t ldout, bool dev) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!analysed(f)) return SPLLT_ERROR_PARAMETER;
  const char* bad = !gval ? "the gradient array is null" : ldout < f->S->nnzA ? "ldout < nnz" : nullptr;
  if (int rc = enter(f, what, bad, kBatchAdjoint)) return rc;
  const int rc = f->eng->fadj_sweep_batch(gval, ldout, dev);
  if (rc == SPLLT_ERROR_NOT_POSDEF)   // -20 of the batch calls
    return fail(f, what, "the members that are not positive definite were skipped (their rows are NaN), the others are "
                         "served (spllt_hip_batch_status)", rc);
  return leave(f, rc);
}

int spllt_hip_factor_adjoint_batch_dev(void* fkeep, double* gval_dev, int64_t ldout) {
  return bfadj_sweep_impl("spllt_hip_factor_adjoint_batch_dev", fkeep, gval_dev, ldout, true);
}

int spllt_hip_factor_adjoint_batch(void* fkeep, double* gval_host, int64_t ldout) {
  return bfadj_sweep_impl("spllt_hip_factor_adjoint_batch", fkeep, gval_host, ldout, false);
}

int spllt_hip_batch_adjoint_launches(void* fkeep) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!f) return SPLLT_ERROR_PARAMETER;
  return (f->eng && !f->dead) ? f->eng->batch_adjoint_launches() : 0;
}

// ---- giving a feature's device memory back ---------------------------------------------------------
// Three shapes have grown, and they differ observably; the differences stay, as flags:
//   WAIT_NOT_POSDEF  a pending failure other than "not positive definite" is returned, nothing released
//   WAIT_IGNORE      whatever the pending factorization reports, the memory is released
//   LENIENT          a handle without an analysis or a dead one has nothing to release: 0 (else -10 / -30)
static int release(void* fkeep, int (Engine::*fn)(), unsigned need) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  const bool lenient = (need & LENIENT) != 0;
  if (!f || (!lenient && !f->S)) return SPLLT_ERROR_PARAMETER;
  if (f->dead) return lenient ? 0 : SPLLT_ERROR_HIP;
  if (!f->eng) return 0;
  const int rc = do_wait(f);
  if ((need & WAIT_NOT_POSDEF) && rc && rc != SPLLT_ERROR_NOT_POSDEF) return rc;
  return leave(f, (f->eng.get()->*fn)());
}

int spllt_hip_release_solve_repro(void* fkeep) { return release(fkeep, &Engine::release_solve_repro, WAIT_NOT_POSDEF); }
int spllt_hip_release_constraints(void* fkeep) { return release(fkeep, &Engine::release_constraints, WAIT_NOT_POSDEF); }
int spllt_hip_release_factor_mult(void* fkeep) { return release(fkeep, &Engine::release_factor_mult, WAIT_NOT_POSDEF); }
int spllt_hip_release_solve_sparse(void* fkeep) { return release(fkeep, &Engine::release_solve_sparse, WAIT_NOT_POSDEF); }
int spllt_hip_release_refine(void* fkeep) { return release(fkeep, &Engine::release_refine, WAIT_IGNORE); }
int spllt_hip_release_batch(void* fkeep) { return release(fkeep, &Engine::release_batch, WAIT_IGNORE | LENIENT); }
int spllt_hip_release_factor_mult_batch(void* fkeep) { return release(fkeep, &Engine::release_factor_mult_batch, WAIT_IGNORE | LENIENT); }
int spllt_hip_release_solve_many_batch(void* fkeep) { return release(fkeep, &Engine::release_solve_many_batch, WAIT_IGNORE | LENIENT); }
int spllt_hip_release_solve_sparse_batch(void* fkeep) { return release(fkeep, &Engine::release_solve_sparse_batch, WAIT_IGNORE | LENIENT); }
int spllt_hip_release_updown_batch(void* fkeep) { return release(fkeep, &Engine::release_updown_batch, WAIT_IGNORE | LENIENT); }
int spllt_hip_release_batch_repro(void* fkeep) { return release(fkeep, &Engine::release_batch_repro, WAIT_IGNORE | LENIENT); }
int spllt_hip_release_refine_batch(void* fkeep) { return release(fkeep, &Engine::release_refine_batch, WAIT_IGNORE | LENIENT); }
int spllt_hip_release_constraints_batch(void* fkeep) { return release(fkeep, &Engine::release_constraints_batch, WAIT_IGNORE | LENIENT); }
int spllt_hip_release_inverse_batch(void* fkeep) { return release(fkeep, &Engine::release_inverse_batch, WAIT_IGNORE | LENIENT); }
int spllt_hip_release_factor_adjoint_batch(void* fkeep) { return release(fkeep, &Engine::release_factor_adjoint_batch, WAIT_IGNORE | LENIENT); }
int spllt_hip_release_inverse(void* fkeep) { return release(fkeep, &Engine::release_inverse, WAIT_IGNORE | LENIENT); }
int spllt_hip_release_factor_adjoint(void* fkeep) { return release(fkeep, &Engine::release_factor_adjoint, WAIT_IGNORE | LENIENT); }

int spllt_hip_factor_times(void* fkeep, double* submit_ms, double* device_ms, double* h2d_ms, int* launches) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!f || !f->eng) return SPLLT_ERROR_PARAMETER;
  const FactorStats& st = f->eng->stats();
  if (submit_ms) *submit_ms = st.submit_ms;
  if (device_ms) *device_ms = st.device_ms;
  if (h2d_ms) *h2d_ms = st.h2d_ms;
  if (launches) *launches = st.launches;
  return 0;
}

// ---- spllt_hip_program_get: one function per family of names ---------------------------------------
// "pattern_*": the index stream of the sampled outer product, from the analysed pattern alone
static int64_t get_pattern(Fkeep* f, const std::string& k, const Out& o) {
  const PatternTables* t = f->po.get(f->S, 0, 0, [&](PatternTables& v) { build_pattern_tables(*f->S, v.row, v.col); return 0; });
  if (k == "pattern_row") return o.bytes(t->row);
  if (k == "pattern_col") return o.bytes(t->col);
  return -1;
}

// "matvec_*": the operator of the refined solves, from the analysed pattern and the pivot order alone
static int64_t get_matvec(Fkeep* f, const std::string& k, const Out& o) {
  const MatvecTables* t = f->mv.get(f->S, 0, 0, [&](MatvecTables& v) {
    build_matvec_tables(*f->S, v.rowptr, v.col, v.src);
    return 0;
  });
  if (k == "matvec_rowptr") return o.bytes(t->rowptr);
  if (k == "matvec_col") return o.bytes(t->col);
  if (k == "matvec_src") return o.bytes(t->src);
  return -1;
}

// (the rows of the tables that go out as int64 columns)
static void put(std::vector<int64_t>& v, std::initializer_list<int64_t> row) {
  for (int64_t x : row) v.push_back(x);
}

// "selinv_*" of a selected-inversion program (the handle's, or the batch's under "batch_selinv_*")
static int64_t get_selinv(const SelinvProgram* sp, const std::string& q, const Out& o) {
  if (!sp) return -1;
  if (q == "selinv_units") return o.bytes(sp->units);
  if (q == "selinv_tiles") return o.bytes(sp->tiles);
  if (q == "selinv_rows") return o.bytes(sp->rows);
  if (q == "selinv_relpos") return o.bytes(sp->relpos);
  if (q == "selinv_diag") return o.bytes(sp->diag_pos);
  if (q == "selinv_scratch") return o.bytes(&sp->scratch_size, sizeof(int64_t));
  if (q == "selinv_flops") return o.bytes(&sp->flops, sizeof(double));
  if (q == "selinv_launches") {   // int64 x 5 per launch: kind, level, first, count, flops
    std::vector<int64_t> v;
    for (const SelinvLaunch& l : sp->launches)
      put(v, {(int64_t)l.kind, (int64_t)l.level, (int64_t)l.first, (int64_t)l.count, (int64_t)l.flops});
    return o.bytes(v);
  }
  return -1;
}

// the tables of a substitution program under their "solve_*" names; -1: not one of them
static int64_t get_solve_tables(const SolveProgram& sp, const std::string& k, const Out& o) {
  if (k == "solve_units") return o.bytes(sp.units);
  if (k == "solve_list") return o.bytes(sp.diag_list);
  if (k == "solve_tiles") return o.bytes(sp.tiles);
  if (k == "solve_fwd" || k == "solve_bwd") {
    std::vector<int64_t> v;
    for (const SolveLaunch& l : (k == "solve_fwd" ? sp.fwd : sp.bwd))
      put(v, {(int64_t)l.kind, (int64_t)l.level, (int64_t)l.first, (int64_t)l.count});
    return o.bytes(v);
  }
  return -1;
}

// "solve_*" and "rsolve_*": the substitution program (partition-aware like the factor program) and the tables of
// the reproducible solve, which follow from it and the symbolic structure alone
static int64_t get_solve(Fkeep* f, int cb, const std::string& k, const Out& o) {
  SolveProgram sp;
  std::vector<int> owner;
  if (f->eo.nranks > 1) assign_owners(*f->S, f->eo.nranks, owner);
  build_solve_program(*f->S, f->eo.pw > 0 ? f->eo.pw : kPanelMax, cb, sp, f->eo.nranks > 1 ? owner.data() : nullptr,
                      f->eo.rank);
  const int64_t got = get_solve_tables(sp, k, o);
  if (got != -1) return got;
  if (k == "solve_split") {
    int64_t v[2] = {(int64_t)sp.fwd_nsub, (int64_t)sp.bwd_ntop};
    return o.bytes(v, sizeof v);
  }
  if (k.rfind("rsolve_", 0) != 0) return -1;
  RsolveTables R;
  build_rsolve_tables(*f->S, sp, R);
  if (k == "rsolve_fslot") return o.bytes(R.fslot);
  if (k == "rsolve_bfirst") return o.bytes(R.bfirst);
  if (k == "rsolve_gptr") return o.bytes(R.gptr);
  if (k == "rsolve_gsrc") return o.bytes(R.gsrc);
  if (k == "rsolve_bslot") return o.bytes(R.bslot);
  if (k == "rsolve_frows") return o.bytes(&R.frows, sizeof(int64_t));
  if (k == "rsolve_bsize") return o.bytes(&R.bsize, sizeof(int64_t));
  return -1;
}

// the plain names: the tables of a factor program (the handle's, or the batch's under "batch_*")
static int64_t get_plain(const Program* P, const std::string& k, const Out& o) {
  auto scalar = [&](int64_t v) { return o.bytes(&v, sizeof v); };
  if (k == "launches") {
    std::vector<int64_t> v;
    for (const Launch& l : P->launches) {
      put(v, {(int64_t)l.kind, (int64_t)l.level, (int64_t)l.first, (int64_t)l.count, (int64_t)l.tile,
                         (int64_t)l.flops, (int64_t)l.stream, (int64_t)l.record});
      for (int w : l.wait) v.push_back(w);
    }
    return o.bytes(v);
  }
  if (k == "potrf") return o.bytes(P->potrf_units);
  if (k == "units") return o.bytes(P->units);
  if (k == "tiles") return o.bytes(P->tiles);
  if (k == "relpos") return o.bytes(P->relpos);
  if (k == "exchanges") {   // int64 x 5 per exchange: kind, first_item, nitems, elems, chunk
    std::vector<int64_t> t;
    for (const Exchange& e : P->exchanges)
      put(t, {(int64_t)e.kind, (int64_t)e.first_item, (int64_t)e.nitems, (int64_t)e.elems, (int64_t)e.chunk});
    return o.bytes(t);
  }
  if (k == "xitems") {      // int64 x 6 per item: block column, root, offset in the buffer, count,
    std::vector<int64_t> t; // offset in the arena / dinv scratch, space (0 arena, 1 dinv)
    for (const ExchangeItem& e : P->xitems)
      put(t, {(int64_t)e.bcol, (int64_t)e.root, (int64_t)e.xoff, (int64_t)e.count, (int64_t)e.off,
                         (int64_t)e.space});
    return o.bytes(t);
  }
  if (k == "xbuf_elems") return scalar(P->xbuf_elems);
  if (k == "panels") return o.bytes(P->panel_units);
  if (k == "sub_tasks") return o.bytes(P->sub_tasks);
  if (k == "sub_nodes") return o.bytes(P->sub_nodes);
  if (k == "gen_size") return scalar(P->gen_size);
  if (k == "chains") return o.bytes(P->chain_units);
  if (k == "chain_block") return scalar(P->cb);
  if (k == "panel_width") return scalar(P->pw);
  if (k == "gather_tiles") return o.bytes(P->gather_tiles);
  if (k == "gather_items") return o.bytes(P->gather_items);
  if (k == "scratch_size") return scalar(P->scratch_size);
  if (k == "dinv_size") return scalar(P->dinv_size);
  return -1;
}

// "batch_*": the program of the batched factorization (fixed options, independent of the handle's engine flags)
static int64_t get_batch(Fkeep* f, const std::string& q, const Out& o) {   // q: the unprefixed name
  const Program* P = f->bt.get(f->S, 0, 0, [&](Program& v) { return build_batch_program(*f->S, v, &f->last_error); });
  if (!P) return -1;
  // ("potrf" and "scratch_size" -- empty and 0 in this program -- because tests/emulate.py asks for them)
  static const char* const kNames[] = {"launches", "units", "tiles", "chains", "relpos", "dinv_size", "potrf", "scratch_size"};
  for (const char* n : kNames)
    if (q == n) return get_plain(P, q, o);
  return -1;
}

// "batch_det_*": the deterministic program of the batched factorization (batch_repro.hip), the same fixed options
static int64_t get_batch_det(Fkeep* f, const std::string& q, const Out& o) {
  const Program* P = f->btd.get(f->S, 1, 0, [&](Program& v) { return build_batch_program(*f->S, v, &f->last_error, true); });
  if (!P) return -1;
  static const char* const kNames[] = {"launches", "units", "tiles", "chains", "relpos", "dinv_size", "potrf", "scratch_size",
                                       "gather_tiles", "gather_items"};
  for (const char* n : kNames)
    if (q == n) return get_plain(P, q, o);
  return -1;
}

// "batch_rsolve_*": the tables of the reproducible sweep of the batch, from the batch's own solve program (pw = cb = 64)
static int64_t get_batch_rsolve(Fkeep* f, const std::string& q, const Out& o) {
  const RsolveTables* R = f->brs.get(f->S, 64, 64, [&](RsolveTables& v) {
    SolveProgram sp;
    build_solve_program(*f->S, 64, 64, sp);
    v = RsolveTables();
    build_rsolve_tables(*f->S, sp, v);
    return 0;
  });
  if (q == "fslot") return o.bytes(R->fslot);
  if (q == "bfirst") return o.bytes(R->bfirst);
  if (q == "gptr") return o.bytes(R->gptr);
  if (q == "gsrc") return o.bytes(R->gsrc);
  if (q == "bslot") return o.bytes(R->bslot);
  if (q == "frows") return o.bytes(&R->frows, sizeof(int64_t));
  if (q == "bsize") return o.bytes(&R->bsize, sizeof(int64_t));
  return -1;
}

int64_t spllt_hip_program_get(void* fkeep, const char* name, void* buf, int64_t cap) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  if (!f || !f->S || !name) return -1;
  const std::string k(name);
  auto is = [&](const char* prefix) { return k.rfind(prefix, 0) == 0; };
  if (k == "solve_sparse_host_us") {   // (of this handle's last sparse solve or gram; written whole or not at all)
    const int64_t v = f->eng ? f->eng->solve_sparse_host_us() : 0;
    return Out{cap >= (int64_t)sizeof v ? buf : nullptr, cap}.bytes(&v, sizeof v);
  }
  if (k == "solve_sparse_batch_host_us") {   // (... of the last sparse solve or gram of the batch)
    const int64_t v = (f->eng && !f->dead) ? f->eng->solve_sparse_batch_host_us() : 0;
    return Out{cap >= (int64_t)sizeof v ? buf : nullptr, cap}.bytes(&v, sizeof v);
  }
  const Out o{buf, cap};
  if (k == "owned") {   // (entries of the engine's ledger of device buffers and their bytes: host state only)
    int64_t v[2] = {0, 0};
    if (f->eng) f->eng->owned_info(v);
    return o.bytes(v, sizeof v);
  }
  if (is("pattern_")) return get_pattern(f, k, o);
  if (is("matvec_")) return get_matvec(f, k, o);
  // The program can be inspected without a GPU: build it on demand.
  Program local;
  const Program* P;
  if (f->eng && !f->eng->status()) {
    P = &f->eng->program();
  } else {
    build_local_program(f, local);
    P = &local;
  }
  if (is("batch_selinv_"))   // panels of 64 columns whatever the handle's, from the symbolic structure alone
    return get_selinv(f->bsi.get(f->S, 64, 64, [&](SelinvProgram& v) { return build_selinv_program(*f->S, 64, 64, v); }),
                      k.substr(6), o);
  if (is("batch_det_")) return get_batch_det(f, k.substr(10), o);
  if (is("batch_rsolve_")) return get_batch_rsolve(f, k.substr(13), o);
  if (is("bsolve_")) {   // "bsolve_*": the "solve_*" tables of the batch's own substitution program (pw = cb = 64, no partition)
    SolveProgram sp;
    build_solve_program(*f->S, 64, 64, sp);
    return get_solve_tables(sp, k.substr(1), o);
  }
  if (is("batch_")) return get_batch(f, k.substr(6), o);
  if (is("selinv_"))         // (single GPU; built from the symbolic structure alone)
    return get_selinv(f->si.get(f->S, P->pw, P->cb, [&](SelinvProgram& v) { return build_selinv_program(*f->S, P->pw, P->cb, v); }),
                      k, o);
  if (is("solve_") || is("rsolve_")) return get_solve(f, P->cb, k, o);
  return get_plain(P, k, o);
}

// ---- timing runs -------------------------------------------------------------------------------------
// one factorization for its per-launch times; an engine that cannot be had is a device error here
enum Timing { PROFILE_SERIAL, PROFILE_IN_PROGRAM, TIMELINE };

static int timing_impl(void* fkeep, const double* val, int nnz, float* ms, int capacity, Timing how) {
  Fkeep* f = static_cast<Fkeep*>(fkeep);
  // (WAIT_IGNORE: a factorization still in flight owns the streams and the events)
  if (int rc = enter(f, nullptr, val ? nullptr : "", WAIT_IGNORE)) return rc;
  if (ensure_engine(f)) return SPLLT_ERROR_HIP;
  std::vector<float> v;
  if (int rc = how == TIMELINE ? f->eng->timeline(val, nnz, v) : f->eng->profile_launches(val, nnz, v, how == PROFILE_SERIAL))
    return rc;
  for (int i = 0; i < (int)v.size() && i < capacity; ++i) ms[i] = v[i];
  f->hostL_valid = false;
  ++f->serial[0];
  return (int)v.size();
}

int spllt_hip_profile(void* fkeep, const double* val, int nnz, float* ms, int capacity) {
  return timing_impl(fkeep, val, nnz, ms, capacity, PROFILE_SERIAL);
}
int spllt_hip_profile_in_program(void* fkeep, const double* val, int nnz, float* ms, int capacity) {
  return timing_impl(fkeep, val, nnz, ms, capacity, PROFILE_IN_PROGRAM);
}
int spllt_hip_timeline(void* fkeep, const double* val, int nnz, float* t_ms, int capacity) {
  return timing_impl(fkeep, val, nnz, t_ms, capacity, TIMELINE);
}

int spllt_hip_last_flag(const void* fkeep) {
  const Fkeep* f = static_cast<const Fkeep*>(fkeep);
  return f ? (f->dead ? SPLLT_ERROR_HIP : f->last_flag) : SPLLT_ERROR_PARAMETER;
}

const char* spllt_hip_last_error(const void* fkeep) {
  const Fkeep* f = static_cast<const Fkeep*>(fkeep);
  if (!f) return "";
  // (a handle whose communicator is a one-rank stand-in says so for as long as it lives)
  if (f->last_error.empty() && f->eng && f->eng->comm_rehearsal())
    return "rehearsal: a one-rank communicator stands in for the partition's ranks (SPLLT_HIP_COMM_REHEARSAL); "
           "the factor of this handle is not the factor of the matrix";
  return f->last_error.c_str();
}

const char* spllt_hip_version(void) { return "spllt-hip 0.1 (gfx950)"; }

}  // extern "C"
