// Device-side factorization engine: owns the L arena in HBM, the uploaded
// work tables of the stream-DAG program, and the HIP stream(s) it runs on.
// This is what replaces spllt_stf_factorize + the task runtimes
// (reference src/spllt_stf_mod.F90:18-192).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <functional>
#include <initializer_list>
#include <memory>
#include <string>
#include <vector>

#include "engine_detail.hpp"
#include "kernels.hpp"
#include "schedule.hpp"
#include "ss_driver.hpp"
#include "ss_filter.hpp"
#include "symbolic.hpp"

namespace spx {

struct RfOperator;   // (refine.hpp)
struct BrfView;

// deadline of every blocking wait, seconds (SPLLT_HIP_TIMEOUT_S, default 180; 0: none)
double hip_deadline_s();
// runs fn on the process's submission thread and waits for it with that deadline; a job that
// does not come back makes this call and every later one return SPLLT_ERROR_HIP (-30) with *why
// naming the last step the library reached (engine.cpp)
int run_with_deadline(std::function<int()> fn, std::string* why);
// process-wide "the HIP runtime did not come back from a call" flag (set by the wait / submission
// deadlines): the atexit teardown of the pools then touches nothing
void mark_runtime_wedged();
bool runtime_wedged();
void run_pools_teardown_for_test();
const char* last_crumb();

struct EngineOptions {
  int pw = 64;
  int tile = 128;
  int cb = 64;             // ignored (see ScheduleOptions)
  bool lookahead = true;   // multi-stream program (panel chain overlaps trailing updates)
  bool slice_between = true;  // inter-node updates in K slices beside the panel chains
  bool deterministic = false;  // see ScheduleOptions
  bool fused_panel = true;     // see ScheduleOptions
  int dist_top = -1;           // multi-GPU top tree: 1 distributed over the ranks, 0 replicated on every
                               // rank, -1 by distribute_top_tree() (env SPLLT_DIST_TOP overrides)
  bool poison_lds = false; // debug: poison the LDS of every CU before every launch
  int reserve_cus = -1;    // CUs the bulk / far streams are masked off (0: no mask; -1: 32 when the
                           // problem is latency-bound (schedule.hpp), else 0)
  int zones = -1;          // zone pipeline of the inter-node updates (1 / 0; -1: when latency-bound)
  int rank = 0, nranks = 1;  // multi-GPU subtree partition (nranks > 1: two-phase program)
  int subtrees = -1;       // small subtrees as single device tasks (L_SUBTREE): 1 / 0; -1: the default (off)
  int graph = -1;          // HIP-graph replay of the factorization (single GPU): 0 eager launches, 1 one
                           // chain of kernel nodes in program order, 2 the DAG of the multi-stream
                           // program, -1 by problem size (env SPLLT_HIP_GRAPH overrides)
};

// debug hook (spllt_hip_debug "batch_selinv_fused=0|1"): 0 forces the three-launch form of every step of the
// batched selected inversion; process-wide, read when an inversion is enqueued
void set_batch_selinv_fused(bool on);
// switch (spllt_hip_debug "batch_fadj_fused=0|1"): 1 runs every eligible step of the factor adjoint of a batch as
// ONE fused launch, 0 (the default: DESIGN.md section 23) all steps in their three-launch form; process-wide, read
// when a sweep is enqueued
void set_batch_fadj_fused(bool on);
// debug: the scratch of the reproducible solve is filled with NaN before every sweep
void set_rsolve_poison(bool on);
// debug hook (spllt_hip_debug "batch_repro_poison=0|1"): 1 fills the scratch of the deterministic batch
// factorization and that of the reproducible batch sweep with NaN before every factorization and every sweep
void set_batch_repro_poison(bool on);
bool batch_repro_poison();
// debug: the scratch of the factor products is filled with NaN before every direction
void set_fmult_poison(bool on);
// debug: the next n allocations of the factor products' workspace and scratch fail (the fall-back to blocks of 16)
void set_fmult_alloc_fail(int n);
// debug: the k-th allocation of feature memory from now on (a Take or a grow; 1: the next) fails once with "out of
// memory", then the hook is disarmed; 0 disarms it
void set_alloc_fail_at(int k);
bool alloc_fail_armed();
// debug: the workspace of a sparse solve is filled with NaN before its touched rows are zeroed
void set_solve_sparse_poison(bool on);
// ... and the whole workspace of the batch before a sparse solve of the batch clears its touched rows
void set_solve_sparse_batch_poison(bool on);
bool batch_selinv_fused();
bool batch_fadj_fused();

struct FactorStats {
  double submit_ms = 0;   // host time spent in factor_async
  double device_ms = 0;   // HIP-event time from first to last enqueued operation
  double h2d_ms = 0;
  int launches = 0;
};

// EngineOptions -> ScheduleOptions (the one place); resolves the "decide by the problem" options of opt
ScheduleOptions schedule_options(const Symbolic& S, EngineOptions& opt);
// HIP-graph replay of a factorization of S: 0 eager launches, 1 one chain of kernel nodes, 2 the DAG of the
// multi-stream program (opt.graph, env SPLLT_HIP_GRAPH, or by problem size)
int resolve_graph_mode(const Symbolic& S, const EngineOptions& opt);

// Partition of the tree for opt.nranks ranks: node owners, and (distributed top tree) the owners of
// the top-tree block columns; fills the partition fields of so (the vectors must outlive it).
void partition_options(const Symbolic& S, const EngineOptions& opt, std::vector<int>& owner,
                       std::vector<int>& top_owner, ScheduleOptions& so);

// the two callables through which a Take, a grow and a give_back work on an engine's ledger of device buffers
class Engine;
struct EngineAlloc { Engine* eng; inline hipError_t operator()(void** p, size_t bytes) const; };
struct EngineRelease { Engine* eng; inline void operator()(void* p) const; };
using FeatureTake = Take<EngineAlloc, EngineRelease>;

class Engine {
 public:
  Engine(std::shared_ptr<const Symbolic> S, const EngineOptions& opt);
  ~Engine();
  Engine(const Engine&) = delete;
  Engine& operator=(const Engine&) = delete;

  int status() const { return status_; }  // 0 or SPLLT error flag from construction
  bool poisoned() const { return poisoned_; }
  bool comm_rehearsal() const { return comm_rehearsal_; }
  void poison(const std::string& why) { poisoned_ = true; status_ = -30; err_ = why; }
  const std::string& error() const { return err_; }
  // what the last call of a feature below (blocked / reproducible / refined solve, update, selected inversion,
  // batch) has to say about its failure; empty: see error().  Every such call clears it on entry.
  const std::string& feature_error() const { return feature_err_; }

  // spllt_factor: enqueue H2D of val, value scatter and the whole program.
  int factor_async(const double* val_host, int64_t nnz);
  // Same with val already resident in HBM (device pointer, same device).
  int factor_async_dev(const double* val_dev, int64_t nnz);
  // spllt_wait for this engine: drain the stream, surface "not positive definite".
  int wait();
  bool pending() const { return pending_; }
  // ---- multi-GPU (nranks > 1): factor_async* stops after the rank's own
  // subtrees with the top-tree block columns packed into the exchange buffer;
  // the caller reduces that buffer across ranks (RCCL all-reduce), then calls
  // continue_after_exchange() and finally wait().
  // doubles the exchange buffer must hold (the largest exchange of the program)
  int64_t exchange_elems() const { return prog_.xbuf_elems; }
  int set_exchange_buffer(double* dev_ptr) { xbuf_ = dev_ptr; return 0; }
  bool awaiting_exchange() const { return awaiting_exchange_; }
  // index (into program().exchanges) of the exchange the engine is waiting for, -1: none
  int pending_exchange() const { return awaiting_exchange_ ? (int)prog_.launches[cur_x_].first : -1; }
  // ---- the collectives inside the library (RCCL over xGMI): with a communicator set,
  // factor_async* does not stop at the exchange points -- every exchange of the program
  // (all-reduce of the top tree / reduce-scatter to the owners + one broadcast per block-column
  // step / the flag) is enqueued on the engine's stream between its pack and its unpack, and
  // the solve adds its two all-reduces of the right-hand sides.  What the reference's
  // distributed build has inside the library too (src/PaRSEC/spllt_parsec_blk_data.c:33-64,
  // factorize.jdf).  comm: the caller's ncclComm_t, one rank per GPU.
  int set_communicator(void* nccl_comm);
  bool has_communicator() const { return comm_ != nullptr; }
  int run_exchanges();              // all pending exchanges, enqueue only
  int sync_phase();                 // drain the streams at the exchange point
  int continue_after_exchange();
  const std::vector<int>& owners() const { return owner_; }
  const std::vector<int>& top_bcols() const { return top_bcols_; }
  const std::vector<char>& map_keep() const { return map_keep_; }
  int not_posdef_column() const { return npd_col_; }
  // doubles of the factor arena held on this device (a rank of a partition: own branches + top tree)
  int64_t arena_elems() const { return arena_elems_; }

  int download(double* out, int64_t count);  // D2H of the arena
  // spllt_solve on the device-resident factor (x: n x nrhs column-major, original
  // variable order, overwritten).  job 0 = both sweeps, 1 = forward, 2 = backward.
  int solve(double* x_host, int nrhs, int job);
  // substitution on device vectors in pivot order; phase -1 = all, 0/1/2 = partitioned phases
  int solve_dev(double* y_dev, int nrhs, int job, int phase);
  int prepare_solve();
  // ---- blocked solve for many right-hand sides (solve_many.hip, single GPU): the same substitution
  // program on blocks of 32 right-hand sides (a tail of at most 16: one block of 16), fp64 MFMA kernels,
  // L read once per block.  x: vector q at x[q * ldx .. q * ldx + n), ldx >= n, overwritten; nothing
  // outside those ranges is read or written.  The strips add with fp64 atomics: reproducible to rounding.
  int solve_many_dev(double* x_dev, int nrhs, int64_t ldx, int job, bool pivot_order);
  int solve_many(double* x_host, int nrhs, int64_t ldx, int job);   // host vectors, user order
  // ---- reproducible solve (solve_repro.hip, single GPU): the substitution program of solve_dev without an
  // atomic add -- strips store their products, the diagonal launches subtract them in the order of the
  // RsolveTables.  Same factor bits + same right-hand-side bits = same solution bits, whatever the group
  // size, the entry point or the handle.  Layout of x as solve_many; sweeps of 4, 2 or 1 vectors.
  // prepare_solve_repro: tables uploaded once, 4 x max(frows, bsize) doubles of scratch and a staging block
  // of 4 n doubles for the host entry point, all or nothing (-1: no memory; the factor and every other solve
  // stay usable).
  int prepare_solve_repro();
  int solve_repro_dev(double* x_dev, int nrhs, int64_t ldx, int job, bool pivot_order);
  int solve_repro(double* x_host, int nrhs, int64_t ldx, int job);   // host vectors, user order
  int release_solve_repro();                                          // tables and scratch back to the pool
  // ---- products with the factor and Gaussian sampling (factor_mult.hip, single GPU): x <- P^T L L^T P x (job 0),
  // P^T L x (job 1), L^T P x (job 2) on blocks of 32 vectors (a tail of at most 16: one block of 16), out of
  // place between the workspace of solve_many and a second one, two launches per direction, no atomic add:
  // the same factor bits and vector bits give the same result bits whatever the block, the place in it or the
  // entry point.  Layout of x as solve_many.  prepare_factor_mult: the RsolveTables (shared with the
  // reproducible solve when resident), the second workspace (rb n doubles) and a scratch of rb * max(frows,
  // bsize) doubles, rb = 32, or 16 when that does not fit (-1: no memory either way; the factor and every
  // solve stay usable).
  int factor_mult_dev(double* x_dev, int nvec, int64_t ldx, int job, bool pivot_order);
  int factor_mult(double* x_host, int nvec, int64_t ldx, int job);   // host vectors, user order
  // z[q * ldz + p] = N(0, 1) of (seed, pivot position p, sample first + q): Philox4x32-10 + Box-Muller
  int white_noise_dev(double* z_dev, int nsamp, int64_t ldz, uint64_t seed, uint64_t first);
  // x[q * ldx ..] = mean + P^T L z_q (kind 1) or mean + P^T L^-T z_q (kind 0: the backward sweep of solve_repro
  // when set_reproducible_solve is on, else of solve_many); mean: n doubles in user order or null; user order
  int sample(double* x, int nsamp, int64_t ldx, int kind, uint64_t seed, uint64_t first, const double* mean, bool dev);
  int release_factor_mult();                                          // workspace, scratch and tables back to the pool
  // ---- the same for every member of the last batch (batch_mult.hip): vector q of member b at x[(b nvec + q) ldx ..],
  // the layout of solve_batch; every launch carries all members (two per direction, plus pack and unpack, per
  // block of 32 vectors per member).  The tables are those of prepare_factor_mult, applied to the members'
  // arenas; taken on first use: two workspaces of nbatch rb n doubles and a scratch of nbatch rb max(frows,
  // bsize), rb = 32, or 16 when that does not fit (-1: no memory either way, nothing kept; the batch, its solve
  // and the single factorization stay usable).  Kept until release_factor_mult_batch / release_batch, re-taken
  // when a later batch has more members.  A member that is not positive definite: its vectors stay as they
  // were, its noise and samples are NaN, the call returns -20.
  int factor_mult_batch_dev(double* x_dev, int nvec, int64_t ldx, int job, bool pivot_order);
  int factor_mult_batch(double* x_host, int nvec, int64_t ldx, int job);   // host vectors, user order
  // z[(b nsamp + q) ldz + p] = N(0, 1) of (seed, pivot position p, stream stream0 + b stream_step, sample first + q)
  int white_noise_batch_dev(double* z_dev, int nsamp, int64_t ldz, uint64_t seed, uint64_t first, uint32_t stream0,
                            int stream_step);
  // x[(b nsamp + q) ldx ..] = mean_b + P^T L_b z_bq (kind 1) or mean_b + P^T L_b^-T z_bq (kind 0: the backward sweep
  // of solve_batch); mean: null, n doubles for all members (ldmean = 0) or member b's at mean + b ldmean
  int sample_batch(double* x, int nsamp, int64_t ldx, int kind, uint64_t seed, uint64_t first, uint32_t stream0,
                   int stream_step, const double* mean, int64_t ldmean, bool dev);
  int release_factor_mult_batch();
  // ---- blocked solve for every member of the last batch (batch_solve_many.hip): the kernels of solve_many with
  // member offsets, on the batch's own solve program.  Vector q of member b at x[(b nrhs + q) ldx ..], the layout
  // of solve_batch; job 0 / 1 / 2 as there.  Each member's vectors go in blocks of 32 (a tail of at most 16: a
  // block of 16); per block: pack, the launches of the sweeps, unpack -- every launch carries all members.
  // Storage on first use: nbatch 32 n doubles, or nbatch 16 n with blocks of 16 only when that does not fit (-1:
  // no memory either way, nothing kept; the batch, solve_batch and the single factorization stay usable).  Kept
  // until release_solve_many_batch / release_batch, re-taken when a later batch has more members.  A member that
  // is not positive definite: its vectors stay as they were, the call returns -20.
  int solve_many_batch(double* x, bool on_device, int nrhs, int64_t ldx, int job, bool pivot_order);
  // on: the backward sweep of sample_batch kind 0 runs through solve_many_batch instead of solve_batch
  void set_batch_blocked_solve(bool on) { bsm_on_ = on; }
  bool batch_blocked_solve() const { return bsm_on_; }
  // block width in use (32, 16 after the fallback, 0 before the first call), blocks per member and kernel launches
  // of the last solve_many_batch, bytes of the workspace
  const int64_t* solve_many_batch_info() const { return bsm_info_; }
  int release_solve_many_batch();
  // ---- bit-reproducible batch (batch_repro.hip; include/spllt_hip_batch_repro.h).  on: factor_batch runs the
  // deterministic batch program (MODE_BUFFER units + ordered gathers) and EVERY blocked sweep of the batch -- the
  // dispatch point enqueue_solve_many_batch_block, to which solve_batch is routed as well -- runs the kernels that
  // store the strip products and subtract them in table order.  The factor scratch (scratch_size doubles per member)
  // is taken with the batch; the sweep's tables and scratch (rb max(frows, bsize) doubles per member) on the first
  // reproducible sweep, all or nothing (-1: nothing kept, the batch and every other solve stay usable).  Flipping the
  // switch keeps the batch.
  void set_batch_reproducible(bool on) { brp_on_ = on; }
  bool batch_reproducible() const { return brp_on_; }
  // solve_many_batch through the reproducible kernels whatever the switch says
  int solve_repro_batch(double* x, bool on_device, int nrhs, int64_t ldx, int job, bool pivot_order);
  // the switch, whether the LAST batch was factorized by the deterministic program, the kernel launches of that
  // factorization, the block width of the last reproducible sweep's last block, bytes of the factor scratch, bytes
  // of the sweep scratch
  void batch_repro_info(int64_t out[6]) const;
  int release_batch_repro();   // the sweep's scratch and tables (the factor scratch goes with the batch)
  // ---- sparse right-hand sides and selected outputs (solve_sparse.hip, single GPU): B = k sparse columns (CSC,
  // 1-based, user order, validated by the caller: check_sparse_columns), sel = nsel wanted user variables (null:
  // all n).  Per group of 32 columns (a tail of at most 16: a block of 16) the substitution program is filtered
  // to the block columns of build_solve_sparse_plan and run by the kernels of solve_many on the shared
  // workspace; x[q * ldx + t] = the solution of column q at sel[t] (at variable t when all are wanted).
  // Everything a call needs on the device is taken before anything is enqueued (-1: no memory, nothing of
  // this feature stays allocated); the stream is drained on return.
  int solve_sparse(int k, const int* bptr, const int* brow, const double* bval, int nsel, const int* sel, double* x,
                   int64_t ldx, int job, bool dev);
  // G = B^T A^-1 B (k x k, column-major, both triangles, host): forward sweeps only, one workspace per group
  int gram_sparse(int k, const int* bptr, const int* brow, const double* bval, double* g_host, int64_t ldg);
  // of the last solve_sparse / gram_sparse: block columns of the forward / backward sweeps, doubles of L in
  // them, kernel launches, workgroups of the sweeps -- summed over the groups, from the uploaded lists
  const int64_t* solve_sparse_info() const { return ss_.info; }
  // host microseconds the last solve_sparse / gram_sparse of this engine spent, before its first device call, on
  // the plans of its groups, the filtered launches and the arrays to be uploaded (not the upload itself)
  int64_t solve_sparse_host_us() const { return ss_.host_us; }
  int release_solve_sparse();
  // on: solve(), solve_dev(phase -1) and the preconditioner of solve_refined go through the path above
  void set_reproducible_solve(bool on) { repro_on_ = on; }
  // ---- refined solves (refine.hip, single GPU): the operator A on the analysed pattern, gather-only, in
  // pivot order, and iterative refinement / conjugate gradients preconditioned by the CURRENT factor, to a
  // requested backward error.  Groups of 32 vectors; the preconditioner is solve_dev (up to 4 vectors) or
  // solve_many_dev in pivot order, unchanged.  val: nnz values on the analysed pattern (device when dev).
  // y = A x; dev: device pointers, then pivot_order says that x and y are in pivot order (x, y distinct)
  int matvec(const double* val, int nvec, const double* x, int64_t ldx, double* y, int64_t ldy, bool dev,
             bool pivot_order);
  // x: b on entry, the solution on exit (user order).  method 0 refinement, 1 PCG.  0: every vector reached
  // tol; 1: at least one did not (x then holds its best confirmed iterate); < 0: error flag
  int solve_refined(const double* val, int nrhs, double* x, int64_t ldx, bool dev, int method, double tol,
                    int max_iter, int* iterations, double* error);
  int release_refine();     // operator tables and work vectors back to the pool
  // ---- the same for the members of a batch (batch_refine.hip).  Vector q of member b at (b * nvec + q) * ld, the
  // layout of solve_batch; member b's values at val + b * ldval.  The product takes nbatch from the caller and
  // needs neither a factor nor a batch; the refined solve serves the members of the LAST batch with their
  // factors as M^-1 (solve_batch below BRF_BLOCKED_MIN vectors per member in a pass, solve_many_batch from there
  // on: measured, from 1).  Passes of at most 32 vectors per member (16 / 8 when the six work arrays do not fit; else -1 with
  // nothing kept).  iterations / error: nbatch * nrhs entries in the order of the vectors, either may be null.
  // A member without a factor: nothing of it is read or written, iterations 0, error NaN, -20 after the others
  // were served.  Else 0: every pair reached tol, 1: at least one did not.
  int matvec_batch(const double* val, int64_t ldval, int nbatch, int nvec, const double* x, int64_t ldx, double* y,
                   int64_t ldy, bool dev, bool pivot_order);
  int solve_refined_batch(const double* val, int64_t ldval, int nrhs, double* x, int64_t ldx, bool dev, int method,
                          double tol, int max_iter, int* iterations, double* error);
  // pass width the workspace holds (0: none held), passes and kernel launches of the last solve_refined_batch (its
  // own kernels and those of the sweeps, whichever route M^-1 took), bytes of the workspace
  const int64_t* solve_refined_batch_info() const { return brf_info_; }
  int release_refine_batch();
  // ---- hard linear constraints C x = e (constrain.hip, single GPU; include/spllt_hip_constrain.h has the
  // mathematics).  set_constraints stores C (k rows of n at c + i * ldc, user order; dev: a device pointer) and builds
  // W = A^-1 C^T (solve_repro_dev when set_reproducible_solve is on, else solve_many_dev), S = C W, S = G G^T, U = W G^-T
  // for the factor `serial` names (the caller's count of changes of the factor); k = 0 releases.  Every later call
  // passes the current serial: when it differs, U, G and the scalars are rebuilt from the stored C first.  Dependent
  // rows: -20, feature_error() names the row, nothing of the feature stays allocated.  Storage, all or nothing (-1: no
  // memory, nothing kept): C and U (k n doubles each), G, the partials of cn_nchunks(n) chunks, t, and the staged e /
  // lambda of a host entry point.
  int set_constraints(int k, const double* c, int64_t ldc, bool dev, int64_t serial);
  int constraints_k() const { return cn_.k; }
  // op 0: the correction of the nvec vectors in x (layout of solve_many); 1: solve_many_dev job 0 first; 2: x = the
  // kind-0 sample of (seed, first + q) + mean first (e then k shared targets: lde = 0).  Passes of at most 32 vectors
  // (for_each_block); host vectors go through the staging block of solve_many.  e: null, shared (lde = 0) or per
  // vector; lambda: null or k per vector.
  enum CnOp : int { CN_CORRECT = 0, CN_SOLVE = 1, CN_SAMPLE = 2 };
  int constrain(int op, int nvec, double* x, int64_t ldx, const double* e, int64_t lde, double* lambda, int64_t ldl,
                bool dev, int64_t serial, uint64_t seed = 0, uint64_t first = 0, const double* mean = nullptr);
  int inverse_diag_constrained(double* out, int n, int64_t serial);   // host, user order; needs inverse_valid()
  // out: k, rebuilds of U, device bytes held, kernel launches of this family in the last call; stat: log det S, the
  // smallest pivot_j / S_jj
  void constraints_info(int64_t out[4], double stat[2]) const;
  int release_constraints();
  // ---- the same for the members of the LAST batch (constrain_batch.hip; include/spllt_hip_constrain_batch.h has the
  // mathematics, the layout of e and lambda and the storage formula).  ONE C for all members; U_b, G_b and the scalars
  // belong to the batch generation they were built for (bt_.generation, bumped by every factor_batch): every call
  // compares and rebuilds from the stored C first, taking the storage again when the batch has grown.  Independent
  // of cn_: neither family reads or touches the other's state.  A member that is not positive definite is skipped
  // by every kernel; the calls return -20 after serving the others.  Dependent rows in ANY factorized member: -20,
  // feature_error() names the member and the row, nothing of the feature stays allocated.  W_b always by
  // solve_many_batch; host vectors through the batch's staging buffer.
  int set_constraints_batch(int k, const double* c, int64_t ldc, bool dev);
  int constraints_batch_k() const { return bcn_.k; }
  // op as CnOp: 0 the correction of the nvec vectors per member in x (layout of solve_batch), 1 solve_many_batch job 0
  // first, 2 the kind-0 samples of sample_batch first (e then k shared targets: lde = 0).  Passes of at most 32
  // vectors per member (for_each_block), three launches each whatever nbatch.
  int constrain_batch(int op, int nvec, double* x, int64_t ldx, const double* e, int64_t lde, double* lambda, int64_t ldl,
                      bool dev, uint64_t seed = 0, uint64_t first = 0, uint32_t stream0 = 0, int stream_step = 1,
                      const double* mean = nullptr, int64_t ldmean = 0);
  int inverse_diag_constrained_batch(double* out, int64_t ldout);   // host, out[b * ldout + i]; needs batch_inverse_valid()
  // out: k, rebuilds, device bytes held, kernel launches of this family in the last call; stat (may be null): log det
  // S_b and the smallest relative pivot of member b at stat + b * ldstat, NaN for a failed member or a stale build
  void constraints_batch_info(int64_t out[4], double* stat, int64_t ldstat) const;
  int release_constraints_batch();
  bool factored() const { return factored_ && !ud_invalid_; }
  // ---- low-rank update / downdate (updown.hip, single GPU): the factor of P (A + sign W W^T) P^T in place of
  // the current one, same layout, the dinv slots of the visited block columns rebuilt -- every solve then works
  // on the modified factor.  W: k columns, CSC, 1-based, user variable order; sign +1 / -1.  Every check
  // (build_updown_plan, by the caller) happens before anything is enqueued; the call returns with the stream drained.  A
  // success marks the selected inverse stale.  A downdate that meets a non-positive pivot returns -20 and
  // leaves the factor INVALID (factor_valid() false) until the next factorization.  The work array (n x 8
  // doubles, zero between calls) and the coefficient scratch stay with the engine; the staged entries of W
  // are returned before the call ends.
  // all / first: the plan and the first pivot positions of build_updown_plan for these columns (the caller has
  // validated them: schedule.hpp).  A launch or a wait that fails mid-sweep leaves the factor invalid as well.
  int updown(int k, const int* wptr, const int* wrow, const double* wval, int sign, const std::vector<int>& all,
             const std::vector<int>& first);
  double updown_device_ms() const { return ud_device_ms_; }   // last updown(): first scatter to last kernel, HIP events
  bool factor_valid() const { return !ud_invalid_; }     // false: a failed downdate destroyed the factor
  // of the last updown(): block columns visited, entries of L in them, kernel launches, passes
  const int64_t* updown_info() const { return ud_info_; }
  // ---- selected inversion (selinv.hip, single GPU): Z = (P A P^T)^-1 on the pattern of L, in a
  // second arena with L's layout.  Computed from the current factor (after wait()); a later
  // factorization marks it stale: the readers below then fail instead of returning old numbers.
  int selected_inverse();
  bool inverse_valid() const { return z_valid_; }
  int download_inverse(double* out, int64_t count);   // Z arena -> host
  int inverse_diag(double* out, int n);               // (A^-1)_ii, user variable order, host
  int log_det(double* out);                           // 2 sum log L_jj of the current factor
  int release_inverse();                              // give the Z arena back to the pool
  // out[k] = (A^-1) at the k-th entry of the analysed CSC-lower pattern (nnz doubles, host): the gather
  // kernel of the batched inversion with one member
  int inverse_on_pattern(double* out);
  int inverse_on_pattern_dev(double* out_dev);        // the same launch, nnz doubles of device memory
  // ---- sampled outer product on the analysed pattern (pattern_outer.hip, single GPU): needs the analysis
  // only, no factor.  out[b * ldout + k] = alpha sum_q (u_q[i] v_q[j] + [i != j] u_q[j] v_q[i]) for entry k =
  // (i, j) of the pattern and member b, vector q of member b at u[(b * nvec + q) * ldu ..], user order.  The
  // (row, column) tables go to the device on first use and stay with the engine.  dev: device pointers, read
  // and written in place; else the three arrays are staged through a buffer that grows with the call.
  int pattern_outer(int nbatch, int nvec, const double* u, int64_t ldu, const double* v, int64_t ldv, double alpha,
                    double* out, int64_t ldout, bool dev);
  double* device_Z() { return z_valid_ ? d_Z_ : nullptr; }
  // ---- reverse-mode derivative of the factor (factor_adjoint.hip, single GPU): G, a third arena with L's
  // layout, holds d loss / d L (seeded or uploaded), and after the sweep d loss / d (P A P^T) on every stored
  // lower position.  The sweep runs siprog_ (the tables and the scratch are shared with the selected inverse).
  // G is taken on first use and kept until release_factor_adjoint; a factorization or an update of the factor
  // makes it unseeded again.  Every check happens before anything is enqueued; every call returns with the
  // stream drained.
  enum FadjState : int { FADJ_UNSEEDED = 0, FADJ_SEEDED = 1, FADJ_SWEPT = 2 };
  int fadj_state() const { return fadj_state_; }
  // G (+)= alpha sum_q a_q b_q^T on the lower positions; vector q at a + q * ld; order_flags bit 0 / 1: a / b is in
  // pivot order (else user order); dev: device pointers
  int fadj_seed(int nvec, const double* a, const double* b, int64_t ld, double alpha, bool accumulate, int order_flags,
                bool dev);
  int fadj_upload(const double* host_arena, int64_t count);   // an arbitrary seed, the layout of download()
  int fadj_download(double* out, int64_t count);
  int fadj_sweep(double* gval, bool dev);                     // gval: nnz doubles in the order of val
  double* device_G() { return fadj_state_ != FADJ_UNSEEDED ? d_G_ : nullptr; }
  int release_factor_adjoint();
  const SelinvProgram& selinv_program() const { return siprog_; }
  // ---- batched factorization (batch.hip, single GPU): nbatch value sets on this pattern, factorized and
  // solved together by a second program of the same Symbolic (build_batch_program) whose every launch
  // carries all members.  The batch has its own arenas, dinv scratch and flags; the tables are shared
  // by the members and uploaded on the first call.  Independent of the engine's single factor.
  int factor_batch(const double* val, bool on_device, int nbatch, int64_t ldval);   // 0, -20 (some member), error
  int batch_count() const { return bt_.nbatch; }
  const std::vector<int>& batch_flags() const { return bt_.hflag; }   // per member: INT_MAX or 1-based pivot position
  int solve_batch(double* x, bool on_device, int nrhs, int64_t ldx, int job, bool pivot_order);
  int download_batch(int member, double* out, int64_t count);
  double* device_batch(int64_t* member_stride);
  int log_det_batch(double* out);
  int batch_launches() const { return bt_.launches; }
  int release_batch();
  // ---- batched selected inversion (batch_selinv.hip): Z_b = (P A_b P^T)^-1 on the pattern of L for every
  // member of the current batch, by a SelinvProgram built with pw = cb = 64 (the panels of the batch
  // factorization) whose every launch carries all members.  The Z arenas (capacity x lstride) and the step
  // scratch are taken on the first call, grow with nbatch and stay until release_batch /
  // release_inverse_batch.  factor_batch marks Z stale.  Independent of selected_inverse() and its arena.
  int selected_inverse_batch();                       // 0, -20 (some member failed: the others are inverted), error
  bool batch_inverse_valid() const { return bt_.z_valid; }
  int download_inverse_batch(int member, double* out, int64_t count);
  double* device_inverse_batch(int64_t* member_stride);
  int inverse_diag_batch(double* out, int64_t ldout);        // host, out[b * ldout + i], user order
  int inverse_on_pattern_batch(double* out, int64_t ldout);  // host, out[b * ldout + k], the order of val
  int inverse_on_pattern_batch_dev(double* out_dev, int64_t ldout);   // the same launch, device output
  int batch_selinv_launches() const { return bt_.si_launches; }
  int release_inverse_batch();
  const SelinvProgram& batch_selinv_program() const { return bt_.siprog; }
  // ---- reverse-mode derivative of the factors of a batch (batch_adjoint.hip): G_b, one more arena per member
  // (capacity x lstride), from d loss / d L_b (seeded or uploaded) to d loss / d (P A_b P^T) on every stored
  // lower position, by the batch's SelinvProgram: tables and step scratch are shared with the batched
  // inversion (whoever comes first takes them; the scratch counts its users), Z and G are separate.
  // The states are those of the single arena, for the whole batch: accumulate needs a seeded arena, the sweep
  // a freshly seeded one, download a seeded or swept one; factor_batch makes it stale.  Every check happens
  // before anything is enqueued; every call returns with the stream drained.  The single arena and its state
  // are not touched.
  int fadj_batch_state() const { return bt_.g_state; }
  // vector q of member b at a + (b * nvec + q) * ld (the layout of solve_batch); the host entry stages groups
  // of at most 32 vectors per member
  int fadj_seed_batch(int nvec, const double* a, const double* b, int64_t ld, double alpha, bool accumulate,
                      int order_flags, bool dev);
  int fadj_upload_batch(const double* host_arenas, int64_t ldarena);   // member b at host_arenas + b * ldarena
  int fadj_download_batch(int member, double* out, int64_t count);
  double* device_G_batch(int64_t* member_stride);
  // gval[b * ldout + k]: nnz doubles per member in the order of val, NaN for a member that is not positive
  // definite (-20 then, the others are served)
  int fadj_sweep_batch(double* gval, int64_t ldout, bool dev);
  int batch_adjoint_launches() const { return bt_.fa_launches; }   // of the last sweep, reader included
  int release_factor_adjoint_batch();
  // ---- low-rank update / downdate of the factors of the LAST batch (batch_updown.hip; include/
  // spllt_hip_updown_batch.h): the members' arenas afterwards hold the factors of P (A_b + sign W_b W_b^T) P^T, in
  // place, their dinv slots rebuilt -- every sweep over the batch then works on the modified factors.  ONE pattern
  // (wptr / wrow, host, validated by the caller: build_updown_plan gives all / first), member b's values at wval + b *
  // ldw (dev: a device pointer, read in place; else staged).  Per pass of up to kUpdownVec columns one scatter launch,
  // then per block column of the pass's plan a generate launch of one workgroup per member and, where it has rows
  // below, an apply launch of (strips x members) workgroups: the launch count does not depend on nbatch.  A member
  // whose downdate meets a non-positive pivot is flagged in the batch's own flags (batch_flags()) and skipped by every
  // batch consumer until the next factor_batch; the call serves the others and returns -20.  A call that reached the
  // device marks the members' inverses stale, their adjoints unseeded and bumps the batch generation.  Storage (work
  // arrays, coefficient scratch, one word per member): ONE transaction on first use, kept until release_batch /
  // release_updown_batch.  A launch or wait that fails mid-sweep leaves the batch without members.
  int updown_batch(int k, const int* wptr, const int* wrow, const double* wval, int64_t ldw, bool dev, int sign,
                   const std::vector<int>& all, const std::vector<int>& first);
  // of the last updown_batch(): block columns visited, entries of L in them per member, kernel launches, passes,
  // members served, members that failed in that call
  const int64_t* updown_batch_info() const { return bud_.info; }
  double updown_batch_device_ms() const { return bud_.device_ms; }
  int release_updown_batch();
  // ---- sparse right-hand sides and B^T A_b^-1 B for every member of the last batch (batch_solve_sparse.hip,
  // spllt_hip_solve_sparse_batch.h): solve_sparse / gram_sparse with every launch carrying
  // all members.  B's pattern is shared (one plan, one filtered program -- the batch's own, bt_.sprog -- and one
  // upload per group); bval: host values, one set (ldb = 0) or member b's at bval + b * ldb.  x: column q of member
  // b at x[(b * k + q) * ldx + t]; g: G_b at g + b * k * ldg.  A flagged member's outputs are NaN (-20 once the
  // others are served).  -98 while the reproducible batch is on.  All device memory is taken before anything runs
  // (-1: nothing of the feature stays allocated, the batch and everything else stay usable).
  int solve_sparse_batch(int k, const int* bptr, const int* brow, const double* bval, int64_t ldb, int nsel,
                         const int* sel, double* x, int64_t ldx, int job, bool dev);
  int gram_sparse_batch(int k, const int* bptr, const int* brow, const double* bval, int64_t ldb, double* g,
                        int64_t ldg, bool dev);
  // of the last call: the six fields of solve_sparse_info (block columns and entries per member, launches, sweep
  // workgroups summed over members), members served, members flagged
  const int64_t* solve_sparse_batch_info() const { return bss_.info; }
  int64_t solve_sparse_batch_host_us() const { return bss_.host_us; }
  int release_solve_sparse_batch();
  double* device_L() { return d_L_; }
  hipStream_t stream() { return stream_; }
  // entries of the ledger of device buffers and their bytes (host state only)
  void owned_info(int64_t out[2]) const;
  // the stream the pending exchange is packed / unpacked on (its collective belongs there); the chain stream when none is pending
  hipStream_t pending_exchange_stream() const { return awaiting_exchange_ ? exchange_stream(prog_.launches[cur_x_]) : stream_; }
  const Program& program() const { return prog_; }
  const Symbolic& symbolic() const { return *S_; }
  const FactorStats& stats() const { return stats_; }
  // per-launch device time of the last factorization (profiling mode)
  int profile_launches(const double* val_host, int64_t nnz, std::vector<float>& ms, bool serial = true);
  // when each event of the real program was reached (ms after the value scatter; see engine.cpp)
  int timeline(const double* val_host, int64_t nnz, std::vector<float>& t);

 private:
  int upload();
  int enqueue_program();
  int enqueue_range(size_t first, size_t last);
  int run_from(size_t first);                 // enqueue launches until the next exchange or the end
  int pre_exchange(const Launch& X);          // waits + pack
  int post_exchange(const Launch& X);         // unpack + record
  int finish_enqueue();
  int enqueue_launch(const Launch& l, bool serial);
  void emit_kernel(const Launch& l, const struct LaunchSink& sink, bool multi);
  int build_graph(int mode);
  int fail(int code, const char* what, hipError_t e);
  // hipStreamSynchronize with a deadline (SPLLT_HIP_TIMEOUT_S, default 180 s; 0 = wait forever):
  // a stream that does not drain makes the call FAIL with a report of the first launch of the
  // program whose event has not fired, instead of blocking the caller forever
  int sync_stream(hipStream_t st, const char* what);

  std::shared_ptr<const Symbolic> S_;
  EngineOptions opt_;
  Program prog_;
  int status_ = 0;
  std::string err_;
  int device_ = 0;
  // streams of the program (schedule.hpp StreamId).  stream_ = chain stream, also the
  // stream every caller-visible operation (H2D, pack, solve) is ordered on.
  hipStream_t stream_ = nullptr;
  hipStream_t streams_[ST_COUNT] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  int chain_prio_ = 1;                 // s_setprio for chain / side update launches
  // optional dynamic-LDS padding (bytes) of the trailing updates that run beside a panel
  // chain (caps their workgroups per CU); off by default: the bulk streams are masked off
  // reserve_cus CUs instead
  int bulk_pad128_ = 0, bulk_pad64_ = 0;
  std::vector<hipEvent_t> dag_events_;  // dependency events of the program
  hipEvent_t ev0_ = nullptr, ev1_ = nullptr, ev_h2d_ = nullptr, ev_init_ = nullptr;
  // device buffers of this engine (pointer, bytes): taken from / returned to the process-wide cache
  std::vector<std::pair<void*, size_t>> owned_;
  hipError_t dalloc(void** p, size_t bytes);
  // The memory of the optional features (engine_detail.hpp): one transaction per prepare_* / reserve_*, on its
  // stack (auto t = take()); buffers that grow with the calls; what a release_* returns.  All of them work on
  // owned_ through dalloc / release_buffer.
  friend struct EngineAlloc;
  friend struct EngineRelease;
  FeatureTake take() { return FeatureTake(EngineAlloc{this}, EngineRelease{this}); }
  template <class Tp> hipError_t grow(Tp** p, size_t* have, size_t need) {
    return spx::grow(EngineAlloc{this}, EngineRelease{this}, p, have, need);
  }
  template <class... Tp> void give_back(Tp*&... p) { spx::give_back(EngineRelease{this}, p...); }
  template <class Tp> hipError_t dev_upload(Tp** dptr, const std::vector<Tp>& v);
  // host-to-device copy of val through two pinned staging buffers (spllt_factor's val is pageable
  // user memory: handing it to hipMemcpyAsync makes the "asynchronous" copy a blocking one inside
  // the runtime, which pins or stages it there)
  static constexpr size_t kH2dChunk = (size_t)16 << 20, kH2dSmall = (size_t)256 << 10;
  size_t h2d_chunk_ = 0;
  void* h2d_buf_[2] = {nullptr, nullptr};
  hipEvent_t h2d_ev_[2] = {nullptr, nullptr};
  bool h2d_busy_[2] = {false, false};
  int stage_val(const double* val_host, int64_t nnz);
  int staged_d2h(void* out_host, const void* src_dev, size_t bytes);
  int wait_event(hipEvent_t ev, const char* what);
  bool poisoned_ = false;   // a wait ran into its deadline: see ~Engine
  bool comm_rehearsal_ = false;   // set_communicator accepted a one-rank stand-in (SPLLT_HIP_COMM_REHEARSAL): results are not the factor
  mutable bool localize_failed_ = false;
  int graph_mode_ = 0;
  const double* val_src_ = nullptr;   // eager factor_async_dev: the caller's device array, read in place (else d_val_)
  bool replays_graph() const { return graph_mode_ > 0 && prog_.exchanges.empty() && !opt_.poison_lds; }
  hipGraph_t graph_ = nullptr;
  hipGraphExec_t graph_exec_ = nullptr;
  bool pending_ = false;
  bool awaiting_exchange_ = false;
  size_t cur_x_ = 0;                // launch index of the exchange the engine waits for
  std::vector<int> top_owner_;      // per block column: owner in a distributed top tree (else empty)
  double* xbuf_ = nullptr;          // caller-owned device buffer of xchg_elems_ doubles
  void* comm_ = nullptr;            // ncclComm_t (set_communicator)
  int comm_rank_ = 0, comm_size_ = 1;
  int collective(const Exchange& E, hipStream_t xs);
  hipStream_t exchange_stream(const Launch& X) const;
  double* d_owned_ = nullptr;       // per pivot position: 1.0 where this rank contributes to a distributed vector
  std::vector<int> owner_;          // per node: owning rank or -1 (top tree)
  std::vector<int> top_bcols_;      // block columns of the top tree, in order
  std::vector<char> map_keep_;      // per val->L map entry: scattered on this rank?
  std::vector<std::pair<int64_t, int64_t>> zero_ranges_;  // (offset, count) of the arena this rank clears
  int64_t nmap_ = 0;                // entries of the (filtered) scatter map on the device
  int npd_col_ = -1;
  // A rank of a partition stores only the block columns it works on (its own branches + the top
  // tree), packed: loc_off_[b] = offset of block column b in THIS rank's arena (-1: not held
  // here).  Every table that carries an arena offset is translated after the program is built;
  // the host-side view (download) stays in the global layout.  Empty: one GPU, arena = global.
  std::vector<int64_t> loc_off_;
  int64_t arena_elems_ = 0;          // doubles of the device arena
  int64_t to_local(int64_t global_off) const;
  void localize_program();
  FactorStats stats_;

  double* d_L_ = nullptr;
  double* d_val_ = nullptr;
  double* d_dinv_ = nullptr;
  int64_t* d_map_dst_ = nullptr;
  int64_t* d_init_cptr_ = nullptr;          // val -> L map bucketed by arena chunk (k_init_arena; single GPU)
  unsigned short* d_init_loc_ = nullptr;
  int* d_init_src_ = nullptr;
  int64_t* d_map_src_ = nullptr;
  int64_t* d_bc_off_ = nullptr;
  int* d_bc_w_ = nullptr;
  char* d_tables_ = nullptr;        // one allocation behind the table pointers below
  char* d_solve_tables_ = nullptr;  // ... and behind the solve tables
  UpdUnit* d_units_ = nullptr;
  UpdTile* d_tiles_ = nullptr;
  ChainUnit* d_chain_ = nullptr;
  PanelUnit* d_panel_ = nullptr;
  SubTask* d_sub_tasks_ = nullptr;   // L_SUBTREE: one workgroup per small subtree
  SubNode* d_sub_nodes_ = nullptr;
  double* d_gen_ = nullptr;          // generated elements of the subtree tasks (zero between factorizations)
  bool solve_four_ = false;        // the solve may use k_solve_diag4 (panels of 64)
  int* d_panel_cnt_ = nullptr;     // two "last reader" counters per panel unit (zero between launches)
  GatherTile* d_gtiles_ = nullptr;
  GatherItem* d_gitems_ = nullptr;
  double* d_scratch_ = nullptr;    // MODE_BUFFER products (deterministic engine)
  // device solve (built on first use)
  SolveProgram sprog_;
  bool solve_ready_ = false;
  SolveUnit* d_sunits_ = nullptr;
  int* d_slist_ = nullptr;
  UpdTile* d_stiles_ = nullptr;
  double* d_y_ = nullptr;
  int* d_relpos_ = nullptr;
  int* d_rlist_ = nullptr;
  int* d_flag_ = nullptr;
  int* h_flag_ = nullptr;  // pinned
  // per launch of sprog_.fwd / .bwd (prepare_solve): may it use k_solve_diag4, and its ONE block column or null
  std::vector<SolveLaunchInfo> sv_fwd_, sv_bwd_;
  SolveTablesView solve_tables() const { return {d_slist_, d_stiles_, d_sunits_, d_L_, d_dinv_, d_rlist_}; }
  // the rule of prepare_solve for one launch over the lists it indexes (the program's, or filtered ones)
  SolveLaunchInfo solve_launch_info(const SolveLaunch& l, const int* list, const UpdTile* tiles) const;
  // where every block column sits in sprog_ (prepare_solve; ss_filter.hpp) -- what filtering the program to a set
  // of block columns walks
  SolveSlots sv_slots_;
  // f(launch, info) for the launches `job` and `phase` ask for, in program order (engine_solve.cpp)
  template <class F> void for_each_solve_launch(int job, int phase, F&& f) const;
  // user variable -> pivot position, for every permutation on the device: uploaded on first use, kept
  int* d_order_ = nullptr;
  hipError_t ensure_order();
  // nv vectors of len doubles (-1: n) between host + q * ldx and the packed device block dev, on stream_
  int copy_vectors(bool to_device, double* dev, double* host, int64_t ldx, int64_t nv, const char* what,
                   int64_t len = -1);
  // (a read-only host side can only go to the device)
  int copy_vectors_to_device(double* dev, const double* host, int64_t ldx, int64_t nv, const char* what,
                             int64_t len = -1) {
    return copy_vectors(true, dev, const_cast<double*>(host), ldx, nv, what, len);
  }
  std::string feature_err_;
  // What a vector entry point does before it touches the device: feature_err_ cleared, then status_, the
  // arguments (-10), a partitioned handle (-98), pending_ (-10), an empty call (0), hipSetDevice.  False: the
  // caller returns *rc.
  bool enter(bool args_ok, bool empty, int* rc);
  // ... and a release_*: status_, nothing held (0), hipSetDevice, the stream idle (`what` names the wait)
  bool enter_release(bool held, const char* what, int* rc);
  // The walk of a blocked feature over the vectors of a call (engine_detail.hpp, for_each_block), on the device
  // or through a staging buffer.  x: vector q of member b at x + (b * total + q) * ldx; members = 1: one arena.
  struct BlockWalk {
    const char* label;        // of the feature, for the texts of a HIP failure
    double* x;
    bool on_device;
    int total;                // vectors per member
    int64_t ldx;
    int members;
    double* stage;            // host x: members * min(total, 32) * n doubles on the device
    int cap;                  // widest block (32 or 16)
    bool pivot_order = false; // of device vectors (staged ones are in user order)
    bool upload = true;       // false: the block is produced on the device (the samplers)
  };
  struct BlockTally { int64_t blocks = 0, launches = 0; };
  // enqueue(done, xdev, xstride, ld, nv, rb, pivot_order) -> launches made, or a negative code that ends the walk.
  // Device x: every block enqueued on x itself, ONE launch check and ONE sync behind the walk.  Host x, per block
  // (the staging buffer is reused): H2D per member, enqueue on the packed block (member b at stage + b * nv * n,
  // ld = n), launch check, D2H per member unless enqueue refused, sync.  Returns 0, what enqueue refused with
  // (once the stream is idle), or kErrHip.
  template <class Enq> int walk_blocks(const BlockWalk& w, Enq&& enqueue, BlockTally* tally = nullptr);
  // Blocks of 32 vectors, and when that does not fit, blocks of 16: one Take per width, every buffer of the list
  // through its block(), in order, at *rb = 32; a failure rolls that width back, and "out of memory" (alone) tries
  // *rb = 16 once.  *want: the bytes of the last width tried.
  struct BlockBuffer { void** p; size_t bytes; };   // bytes per vector of a block
  hipError_t take_block_buffers(std::initializer_list<BlockBuffer> bufs, int* rb, size_t* want);
  // reproducible solve (tables and scratch taken on first use, all or nothing)
  int enqueue_solve_repro(double* y, int64_t ldy, int cur, int job);
  bool repro_on_ = false;
  bool rs_ready_ = false;
  char* d_rstab_ = nullptr;        // one allocation behind the tables below
  int64_t* d_rsfslot_ = nullptr;
  int64_t* d_rsbfirst_ = nullptr;
  int64_t* d_rsgptr_ = nullptr;
  int64_t* d_rsgsrc_ = nullptr;
  int64_t* d_rsbslot_ = nullptr;
  double* d_rsscratch_ = nullptr;  // 4 x rs_stride_ doubles
  double* d_rsstage_ = nullptr;    // 4 n doubles: host vectors in the caller's order
  int64_t rs_stride_ = 0;
  // the RsolveTables on the device, uploaded within the caller's transaction when absent.  Users (rs_users_): the
  // reproducible solve (rs_ready_) and the tables of the factor products (while d_fmtab_ is held).
  void ensure_rsolve_tables(FeatureTake& t);
  void unhold_rsolve_tables();
  Shared rs_users_;
  // factor products (taken on first use, all or nothing).  The chunk list, uploaded within the caller's
  // transaction when absent.  Users (fm_users_): the single-handle products (fm_ready_) and the batched ones
  // (bm_ready_); the first hold takes the RsolveTables along, the last drop lets them go.
  void ensure_fmult_tables(FeatureTake& t);
  void hold_fmult_tables();
  void unhold_fmult_tables();
  Shared fm_users_;
  int prepare_factor_mult(bool host_stage);
  int run_factor_mult(double* x, bool on_device, int nvec, int64_t ldx, int job, bool pivot_order);   // both entry points
  void enqueue_factor_mult_block(double* x_dev, int64_t ldx, int nv, int rb, int job, bool pivot_order);
  bool fm_ready_ = false;
  int fm_rb_ = 32;                 // widest block the workspace and the scratch hold (32, or 16 when memory is short)
  char* d_fmtab_ = nullptr;        // the (block column, chunk of 64 positions) pairs
  UpdTile* d_fmchunks_ = nullptr;
  int64_t fm_nchunks_ = 0;
  double* d_fmW_ = nullptr;        // fm_rb_ * n doubles: the second workspace
  double* d_fmscratch_ = nullptr;  // fm_rb_ * rs_stride_ doubles
  double* d_fmmean_ = nullptr;     // n doubles: the mean of a host entry point
  // batched factor products: workspaces and scratch for bm_capacity_ members
  int prepare_factor_mult_batch();
  int run_factor_mult_batch(double* x, bool on_device, int nvec, int64_t ldx, int job, bool pivot_order);   // both entry points
  void drop_factor_mult_batch();
  BmultView bmult_view(int rb) const;
  void enqueue_factor_mult_batch_block(double* x_dev, int64_t xstride, int64_t ldx, int nv, int rb, int job,
                                       bool pivot_order);
  int batch_failed() const;        // -20 when a member of the last batch is not positive definite
  bool bm_ready_ = false;
  int bm_rb_ = 32;                 // widest block the workspaces and the scratch hold
  int bm_capacity_ = 0;            // members they hold
  int bm_member_fast_ = 0;         // grid order of the product kernels (experiment knob, batch_mult.hip)
  double* d_bmW_[2] = {nullptr, nullptr};   // bm_capacity_ * bm_rb_ * n doubles each
  double* d_bmscratch_ = nullptr;  // bm_capacity_ * bm_rb_ * rs_stride_ doubles
  double* d_bmmean_ = nullptr;     // the means of a host entry point
  size_t bm_mean_elems_ = 0;
  // batched blocked solve: the workspace for bsm_capacity_ members
  int prepare_solve_many_batch();
  void drop_solve_many_batch();
  int enqueue_solve_many_batch_block(double* x_dev, int64_t xstride, int64_t ldx, int nv, int rb, int job,
                                     bool pivot_order);   // launches made, -1: a launch overflows a grid
  bool bsm_ready_ = false;
  bool bsm_on_ = false;            // sample_batch kind 0 goes through the blocked path
  int bsm_rb_ = 32;                // widest block the workspace holds
  int bsm_capacity_ = 0;           // members it holds
  double* d_bsmW_ = nullptr;       // bsm_capacity_ * bsm_rb_ * n doubles: W_b[p * rb + q]
  int64_t bsm_info_[4] = {0, 0, 0, 0};
  // bit-reproducible batch: the deterministic program and its tables (once per engine), the factor scratch (with
  // the batch), the tables and the scratch of the sweep (first reproducible sweep, for sw_capacity members)
  struct BreproState {
    bool ready = false;              // the deterministic program is built and its tables are on the device
    Program prog;
    char* d_tab = nullptr;
    UpdUnit* units = nullptr;
    UpdTile* tiles = nullptr;
    ChainUnit* chain = nullptr;
    int* relpos = nullptr;
    GatherTile* gtiles = nullptr;
    GatherItem* gitems = nullptr;
    double* fscratch = nullptr;      // f_capacity x fstride
    int f_capacity = 0;
    int64_t fstride = 0;
    bool last_det = false;           // the last batch was factorized by the deterministic program
    char* d_swtab = nullptr;
    int64_t* fslot = nullptr;
    int64_t* bfirst = nullptr;
    int64_t* gptr = nullptr;
    int64_t* gsrc = nullptr;
    int64_t* bslot = nullptr;
    int64_t slots = 0;               // max(frows, bsize, 1): scratch slots per right-hand side
    double* swscratch = nullptr;     // sw_capacity x sw_rb x slots
    int sw_rb = 0, sw_capacity = 0;
    int last_rb = 0;
  } brp_;
  bool brp_on_ = false;
  bool brp_force_ = false;           // solve_repro_batch is running
  bool brp_sweep() const { return brp_on_ || brp_force_; }
  int prepare_batch_repro();         // program + tables
  int prepare_solve_repro_batch();   // the sweep's tables and scratch for the members of the last batch
  void drop_solve_repro_batch();
  BatchReproView brepro_factor_view(int nbatch) const;
  // blocked solve (workspace allocated on first use, kept with the engine)
  int prepare_solve_many(bool host_stage);
  int run_solve_many(double* x, bool on_device, int nrhs, int64_t ldx, int job, bool pivot_order);   // both entry points
  void enqueue_solve_many_block(double* x_dev, int64_t ldx, int nv, int rb, int job, bool pivot_order);
  double* d_smW_ = nullptr;        // n * 32 doubles: W[p * rb + q]
  double* d_smstage_ = nullptr;    // n * 32 doubles: a block of host vectors in the caller's order (solve_many)
  // sparse right-hand sides: one group of columns, planned and filtered on the host
  struct SsGroup {
    int c0 = 0, nv = 0, rb = 16;
    bool bwd_full = false;                        // all entries wanted: the backward sweep is the unfiltered program
    std::vector<SolveLaunch> fwd, bwd;            // filtered launches, `first` into the compacted lists
    std::vector<SolveLaunchInfo> fwd_i, bwd_i;
    std::vector<int> list, chunks, selpos;        // compacted diag list; (first, length) chunks; wanted positions
    std::vector<UpdTile> tiles;
    std::vector<int64_t> pos;                     // scatter: pivot position * rb + column
    std::vector<int> ent;                         // the 0-based CSC entry each of pos comes from
    int64_t info[6] = {0, 0, 0, 0, 0, 0};
    size_t bytes = 0;                             // of the staged tables with their values (ss_table_bytes)
  };
  struct SsTables { int* list; UpdTile* tiles; int* chunks; int* selpos; int64_t* pos; double* val; };
  // the sequence of a call is ss_driver.hpp's; its two backends: the handle on sprog_ / sv_slots_ / d_smW_ with three
  // buffers that grow, the batch on bt_.sprog / bss_.slots / d_bsmW_ with one transaction for the three
  struct SsBackend;
  struct SsHandleBackend;
  struct SsBatchBackend;
  static void ss_filter(const SolveProgram& P, const SolveSlots& sl, bool bwd, const std::vector<int>& set, SsGroup& g);
  // launch_info: a SolveLaunchInfo per filtered launch (what the handle's kernels take)
  void ss_plan_group(const SolveProgram& P, const SolveSlots& sl, bool launch_info, SsGroup& g, const int* bptr,
                     const int* brow, int nsel, const int* sel, int job, const std::vector<int>* zero_ranges);
  static size_t ss_table_bytes(const SsGroup& g, size_t copies);
  // tables of a group and `copies` sets of its values (set b: bval + b * ldb) into s.tab (the stream is idle)
  int ss_upload(const SsState& s, const SsGroup& g, const double* bval, int64_t ldb, size_t copies, SsTables& t);
  void ss_drop(SsState& s);
  int ss_release(SsState& s, const char* what);
  int ss_filterable();
  SsState ss_;
  // ... for the members of a batch (batch_solve_sparse.hip): the slots of bt_.sprog (once per engine); the storage
  // of a call is taken together in ONE transaction, kept while it is large enough
  struct BssState : SsState {
    bool slots_ready = false;
    SolveSlots slots;
  } bss_;
  int bss_enter();                                 // the batch's program is filterable, the workspace is there
  int bss_take(size_t tab_bytes, size_t out_elems, size_t gram_elems, const char* what);
  // refined solves: operator tables and work vectors (taken on first use, all or nothing)
  int prepare_refine(bool host_val);
  int refine_apply_factor(double* v, int nv);
  // the two backends of refine_iterate (refine_driver.hpp): one group of the handle, one pass of the batch
  struct RefineBackend;
  struct RefineBatchBackend;
  RfOperator refine_operator() const;
  // the operator tables, uploaded within the caller's transaction when absent.  Users (rf_users_): the single
  // handle's refined solve (refine_ready_), the batch's (brf_ready_) and the product of a batch (brf_mv_held_).
  void ensure_refine_tables(FeatureTake& t);
  void unhold_refine_tables();
  Shared rf_users_;
  // refined solves of a batch: six work arrays, partials, scalars and states for brf_capacity_ members
  int prepare_refine_batch(int members);
  void drop_refine_batch();
  int refine_batch_apply_factor(double* v, int nv, int64_t* launches);
  BrfView brf_view(int nv) const;   // nv vectors of every member of the batch on the scalars of a pass
  bool brf_ready_ = false;
  bool brf_mv_held_ = false;       // matvec_batch has uploaded or found the operator tables and keeps them
  bool brf_held() const { return brf_ready_ || brf_mv_held_ || d_brfval_ || d_brfmv_; }
  int brf_rb_ = 0;                 // pass width the work arrays hold (32, 16 or 8)
  int brf_capacity_ = 0;           // members they hold
  double* d_brfwork_ = nullptr;    // 6 x capacity x brf_rb_ x n: b, x, r, p, q, best x
  double* d_brfpart_ = nullptr;
  double* d_brfds_ = nullptr;      // amax[capacity], sigma[capacity], then the scalars of a pass (refine.hpp)
  int* d_brfis_ = nullptr;
  double* d_brfval_ = nullptr;     // the values of a host entry point
  size_t brf_val_elems_ = 0;
  double* d_brfmv_ = nullptr;      // the product's own workspace: three arrays of members x min(nvec, 32) x n
  size_t brf_mv_elems_ = 0;
  int64_t brf_info_[4] = {0, 0, 0, 0};
  bool factored_ = false;          // a factorization has been enqueued on this engine
  bool refine_ready_ = false;
  char* d_rftab_ = nullptr;        // one allocation behind the four tables below
  int64_t* d_rfrowptr_ = nullptr;
  int* d_rfcol_ = nullptr;
  int* d_rfsrc_ = nullptr;
  int* d_rfrows_ = nullptr;        // rows by length class
  int rf_nrows_[3] = {0, 0, 0};
  double* d_rfwork_ = nullptr;     // 6 x 32 x n: b, x, r, p, q, best x
  double* d_rfpart_ = nullptr;     // partial sums of the reductions
  double* d_rfds_ = nullptr;       // device scalars (refine.hpp)
  int* d_rfis_ = nullptr;
  double* d_rfval_ = nullptr;      // nnz doubles: the values of a host entry point
  // hard linear constraints: C, U, G, the partials and t (taken by set_constraints, all or nothing)
  struct CnState {
    int k = 0;                     // rows of C held (0: none)
    int64_t serial = -1;           // the factor U, G and the scalars belong to
    int64_t rebuilds = 0, launches = 0;
    size_t bytes = 0;
    double* C = nullptr;           // k x n, row i at C + i * n
    double* U = nullptr;           // k x n, column j of U at U + j * n
    double* G = nullptr;           // kCnMaxRows^2, then stat[4]
    double* part = nullptr;        // cn_nchunks(n) * kCnMaxRows^2
    double* T = nullptr;           // kCnPass * kCnMaxRows, then the staged e and lambda (as much each)
    double logdet = 0.0, minrel = 0.0;
  } cn_;
  void drop_constraints();
  int build_constraints(int64_t serial);   // U, G and the scalars from C and the current factor
  int cn_pass(double* xd, int64_t ld, int nv, const double* e, int64_t lde, double* lambda, int64_t ldl);   // enqueue only
  // ... for the members of a batch: C once, everything else per member (taken in one transaction for `capacity`
  // members)
  struct BcnState {
    int k = 0;                     // rows of C held (0: none)
    int capacity = 0;              // members the storage holds
    int64_t generation = -1;       // the batch U_b, G_b and the scalars belong to (-1: none)
    int64_t rebuilds = 0, launches = 0;
    size_t bytes = 0;
    double* C = nullptr;           // k x n
    double* U = nullptr;           // capacity x k x n
    double* G = nullptr;           // capacity x kCnMaxRows^2, then capacity x kBcnStat scalars
    double* part = nullptr;        // capacity x cn_nchunks(n) x kCnMaxRows^2
    double* T = nullptr;           // capacity x kCnPass x kCnMaxRows, then the staged e and lambda (as much each)
    std::vector<double> stat;      // nbatch x 2 of the last build: log det S_b, min pivot_j / S_jj
  } bcn_;
  void drop_constraints_batch();
  int take_constraints_batch(int k, int members, bool keep_c);   // the storage, all or nothing
  int build_constraints_batch();           // U_b, G_b and the scalars from C and the current batch
  int refresh_constraints_batch();         // the build when the batch is newer than the numbers held
  BcnView bcn_view() const;
  // one pass of nv <= kCnPass vectors per member (member b's at xd + b * xs): enqueue only; launches made or -1
  int bcn_pass(double* xd, int64_t xs, int64_t ld, int nv, const double* e, int64_t es, int64_t lde, double* lambda,
               int64_t ls, int64_t ldl);
  // update / downdate: work array and coefficient scratch (taken on first use, both or neither)
  bool ud_invalid_ = false;
  int64_t ud_info_[4] = {0, 0, 0, 0};
  double ud_device_ms_ = 0.0;
  double* d_udW_ = nullptr;        // n x kUpdownVec doubles, zero between calls
  double* d_udcoef_ = nullptr;     // (widest block column) x kUpdownVec x 3 doubles + the flag word
  // ... of the batch: per member a work array (wstride = kUpdownVec n doubles, zero between calls), a coefficient
  // scratch (cstride doubles) and a word; all three or none
  struct BudState {
    double* W = nullptr;
    double* coef = nullptr;
    int* flag = nullptr;
    int capacity = 0;                // members the storage holds
    int64_t wstride = 0, cstride = 0;
    int64_t info[6] = {0, 0, 0, 0, 0, 0};
    double device_ms = 0.0;
    std::vector<int> hflag_pending;  // destination of the words' D2H copy (outlives a wait that fails)
  } bud_;
  void drop_updown_batch();
  // selected inversion (tables uploaded once per pattern, on first use)
  int prepare_selinv();
  void release_buffer(void* p);
  SelinvProgram siprog_;
  bool selinv_ready_ = false;
  bool z_valid_ = false;
  char* d_selinv_tables_ = nullptr;
  SelinvUnit* d_siunits_ = nullptr;
  UpdTile* d_sitiles_ = nullptr;
  SelinvRow* d_sirows_ = nullptr;
  int* d_sirelpos_ = nullptr;
  int64_t* d_sidiag_ = nullptr;
  double* d_Z_ = nullptr;
  double* d_siscratch_ = nullptr;  // users (si_users_): the inverse arena d_Z_ and the adjoint arena d_G_
  Shared si_users_;
  double* d_siout_ = nullptr;      // n + 1 doubles: diag(A^-1), log det
  double* d_sipat_ = nullptr;      // nnz doubles: A^-1 on the analysed pattern (inverse_on_pattern)
  int gather_inverse_on_pattern(double* out_dev, double* arena = nullptr);   // arena: null = d_Z_
  // factor adjoint: the arena, the (block column, strip) tiles of the seed kernel and the position -> variable table
  int prepare_fadj();
  int prepare_fadj_tables();
  int fadj_state_ = FADJ_UNSEEDED;
  double* d_G_ = nullptr;
  double* d_gpat_ = nullptr;       // nnz doubles: the gradient on the analysed pattern (host entry point)
  char* d_fadj_tables_ = nullptr;
  FadjCol* d_facols_ = nullptr;
  UpdTile* d_fatiles_ = nullptr;
  int* d_faporder_ = nullptr;
  int64_t fa_ntiles_ = 0;
  // sampled outer product: the (row, column) tables of the pattern (one allocation, on first use) and the
  // staging block of the host entry point
  char* d_potab_ = nullptr;
  int* d_porow_ = nullptr;
  int* d_pocol_ = nullptr;
  double* d_postage_ = nullptr;
  size_t po_stage_elems_ = 0;
  // batched factorization: tables (uploaded once, on the first batch call) and per-batch storage (grows
  // with nbatch, stays with the engine until release_batch)
  struct BatchState {
    bool ready = false;
    Program prog;
    SolveProgram sprog;
    char* d_tab = nullptr;           // one allocation behind the table pointers below
    UpdUnit* units = nullptr;
    UpdTile* tiles = nullptr;
    ChainUnit* chain = nullptr;
    int* relpos = nullptr;
    int64_t* init_cptr = nullptr;    // the value map bucketed by arena chunk (k_batch_init)
    unsigned short* init_loc = nullptr;
    int* init_src = nullptr;
    int64_t* diag = nullptr;         // per pivot position: arena offset of its diagonal entry
    SolveUnit* sunits = nullptr;
    int* slist = nullptr;
    UpdTile* stiles = nullptr;
    double* L = nullptr;             // capacity x lstride
    double* dinv = nullptr;          // capacity x dstride
    int* flag = nullptr;             // capacity
    double* out = nullptr;           // capacity (log det)
    int capacity = 0, nbatch = 0;
    int64_t lstride = 0, dstride = 0;
    double* Y = nullptr;             // solve workspace, pivot order
    size_t y_elems = 0;
    double* stage = nullptr;         // host entry points: the caller's values / vectors on the device
    size_t stage_elems = 0;
    std::vector<int> hflag;          // flags of the last batch
    std::vector<int> hflag_pending;  // destination of the flags' D2H copy (outlives a wait that fails)
    bool own_init = false;           // init_* are the batch's own upload (else the engine's d_init_* tables)
    int launches = 0;
    int solve_launches = 0;          // kernel launches of the last solve_batch
    int member_fast = 0;
    // batched selected inversion: program and tables (once per engine), Z arenas and scratch (per batch)
    bool si_ready = false;
    SelinvProgram siprog;
    std::vector<char> si_fusable;    // per launch of siprog: the DIAG launch of a step the fused kernel can take
    char* d_sitab = nullptr;
    SelinvUnit* siunits = nullptr;
    UpdTile* sitiles = nullptr;
    SelinvRow* sirows = nullptr;
    int* sirelpos = nullptr;
    double* Z = nullptr;             // z_capacity x lstride
    double* siscratch = nullptr;     // z_capacity x sstride
    int z_capacity = 0;
    int64_t sstride = 0;
    bool z_valid = false;
    int si_launches = 0;
    int sc_capacity = 0;             // members the step scratch holds
    Shared sc_users;                 // of the step scratch: the inverse arenas Z and the adjoint arenas G
    // factor adjoint of the batch: the arenas and their state (FadjState, for the whole batch)
    double* G = nullptr;             // g_capacity x lstride
    int g_capacity = 0;
    int g_state = 0;
    int fa_launches = 0;
    int64_t generation = 0;          // counts the factor_batch calls that replaced the members' factors
  } bt_;
  int prepare_batch();
  int reserve_batch(int nbatch, bool deterministic);   // (deterministic: the factor scratch too, one transaction)
  int grow_batch_buffer(double** p, size_t* have, size_t need, const char* what);   // grow + the batch's message
  BatchView batch_view() const;
  int prepare_batch_selinv();
  int reserve_batch_inverse(int nbatch);
  // The steps [SYMM] [SCALE] DIAG of bt_.siprog in order: fused_step(DIAG launch of the step) where fused and the
  // step is fusable, else one_launch(launch) for each of its launches; both return launches made, or -1.  Returns
  // the sum, or -1 when a grid overflowed (the walk ends there).
  template <class Fused, class One> int walk_batch_steps(bool fused, Fused&& fused_step, One&& one_launch);
  BatchSelinvView batch_selinv_view() const;
  int reserve_batch_arenas(double** arena, int* capacity, int nbatch, const char* feature, const char* which,
                           bool* retaken);
  int reserve_batch_adjoint();
  BatchSelinvView batch_adjoint_view() const;
};

inline hipError_t EngineAlloc::operator()(void** p, size_t bytes) const { return eng->dalloc(p, bytes); }
inline void EngineRelease::operator()(void* p) const { eng->release_buffer(p); }

// The batch program of a pattern: build_program with fixed options (single stream, no fused panels, no
// chain blocks, no subtree tasks, atomics, pw = tile = 64, no partition), whatever the handle's engine
// flags say.  0, or -99 with *why when the program holds anything batch.hip does not implement (launch
// kinds other than L_CHAIN / L_GEMM, tile edges other than 32 / 64, unit modes other than DIRECT /
// SCATTER / TRSM, an atomic DIRECT unit): nothing is skipped silently.
// deterministic: the same options with ScheduleOptions::deterministic (batch_repro.hip) -- MODE_BUFFER units in
// the place of the SCATTER ones and L_GATHER launches are accepted besides, and nothing else.
int build_batch_program(const Symbolic& S, Program& P, std::string* why, bool deterministic = false);
// arena offset of the diagonal entry of every pivot position (from the Symbolic structure alone)
void batch_diag_positions(const Symbolic& S, std::vector<int64_t>& pos);

}  // namespace spx
