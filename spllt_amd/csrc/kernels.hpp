// Launch wrappers of the gfx950 kernels (kernels.hip).  Every wrapper only
// enqueues work on `st`; none synchronises.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "schedule.hpp"

namespace spx {

// Where a kernel goes: onto a stream (eager), or into a HIP graph as a kernel node behind
// `deps` (graph construction, Engine::build_graph; `node` returns the node, `err` the status).
struct LaunchSink {
  hipStream_t stream = nullptr;
  hipGraph_t graph = nullptr;
  const hipGraphNode_t* deps = nullptr;
  size_t ndeps = 0;
  mutable hipGraphNode_t node = nullptr;
  mutable hipError_t err = hipSuccess;
  LaunchSink() = default;
  LaunchSink(hipStream_t st) : stream(st) {}   // every wrapper below also takes a plain stream
};

void launch_scatter_val(const LaunchSink& st, double* L, const double* val, const int64_t* dst,
                        const int64_t* src, int64_t n);
// the arena cleared and A copied in, in one pass (cptr / loc / src: the val -> L map bucketed by
// chunks of kInitChunk doubles of the arena: entries of chunk c are [cptr[c], cptr[c + 1]), loc = the
// entry's position inside the chunk, src = its index in val)
constexpr int kInitChunk = 4096;
void launch_init_arena(const LaunchSink& st, double* L, int64_t arena, const double* val, const int64_t* cptr,
                       const unsigned short* loc, const int* src);
// (unit0 = host copy of units[0]: travels with the kernel arguments)
void launch_potrf(hipStream_t st, const PotrfUnit* units, int64_t count, double* L, double* dinv,
                  int* flag, const PotrfUnit& unit0);
// one small subtree per workgroup (SubTask): its nodes in post-order, what leaves the subtree through the
// generated-element scratch `gen` (zero before and after)
void launch_subtree(const LaunchSink& st, const SubTask* tasks, int64_t count, const SubNode* nodes,
                    const UpdUnit* units, const int* relpos, const int* rlist, double* L, double* dinv, double* gen,
                    int* flag);
// one step of the panel chain per workgroup (ChainUnit): POTRF of the panel + its inverse
void launch_chain_panel(const LaunchSink& st, const ChainUnit* units, int64_t count, double* L, double* dinv,
                        int* flag, const ChainUnit& unit0);
// one chain block of up to four panels per workgroup (ChainUnit, pn = its width <= 4 pw): the whole
// diagonal block factored, the panels' inverses emitted
void launch_chain_block(const LaunchSink& st, const ChainUnit* units, int64_t count, double* L, double* dinv,
                        int* flag, int pw, const ChainUnit& unit0);
// the rows below a chain block solved against it, 64 rows x all columns per workgroup (tiles: unit, ti)
void launch_trsm_rows(const LaunchSink& st, const UpdTile* tiles, int64_t count, const UpdUnit* units, double* L,
                      const double* dinv, int pw, int prio);
// one whole panel step per launch (PanelUnit; tiles: unit, ti = 64-row block below the panel)
// counters: two zero-initialised ints per panel unit (left zero again by the launch)
void launch_panel(const LaunchSink& st, const UpdTile* tiles, int64_t count, const PanelUnit* units, double* L,
                  double* dinv, int* counters, int* flag);
// deterministic assembly of buffered inter-node update blocks (GatherTile / GatherItem)
void launch_gather(const LaunchSink& st, const GatherTile* tiles, int64_t count, const GatherItem* items,
                   double* L, const double* scratch, const int* relpos, const int* rlist);
// multi-GPU: not-positive-definite flag <-> extra element of the exchange buffer
void launch_flag_pack(hipStream_t st, const int* flag, double* slot);
void launch_flag_unpack(hipStream_t st, const double* slot, int* flag);
// y[q * ldy + i] *= keep[i]  (multi-GPU solve: a rank's share of a distributed vector)
void launch_mask(hipStream_t st, double* y, const double* keep, int n, int nrhs, int64_t ldy);
// y[q * n + order[i]] = x[q * ldx + i] (unpack: the other way), q < nv: user order <-> pivot order, a copy of
// the 64 bits of every entry
void launch_permute_vectors(hipStream_t st, bool unpack, double* x, int64_t ldx, const int* order, int n, int nv,
                            double* y);
// debug: fill the LDS of every CU with signalling NaNs
void launch_poison_lds(hipStream_t st);
void launch_update(const LaunchSink& st, int tile, const UpdTile* tiles, int64_t count,
                   const UpdUnit* units, const int64_t* bc_off, const int* bc_w, double* L,
                   const int* relpos, const int* rlist, const double* dinv, int prio = 0,
                   int lds_pad = 0, bool allow_dma = true, bool latency = false);
// (latency: a small launch on the critical path -- 64 columns of K per LDS step instead of 16, so
// that a tile makes a quarter of the dependent round trips to memory)
// (allow_dma = false: the register-staged kernels -- for operands in caller-owned buffers without
// slack behind them: the DMA kernels load whole 16-column chunks)
void launch_scatter_block(hipStream_t st, int s_m, int s_n, const int* rsrc_index,
                          const int* csrc_index, const double* src, int lds,
                          const int* rdest_index, int d_m, const int* cdest_index, int d_n,
                          double* dest, int ldd);

// the device tables every launch of a SolveProgram reads, and the factor they point into
struct SolveTablesView {
  const int* list;
  const UpdTile* tiles;
  const SolveUnit* units;
  const double* L;
  const double* dinv;
  const int* rlist;
};
// per launch of a SolveProgram, decided once on the host: four -- every block column of a DIAG launch has at
// most four 64-wide panels (pw = cb = 64, w <= 256), the kernel that reads L in one round trip; one -- the
// launch works on ONE block column (host copy of its unit; strips: strip i = workgroup i), the descriptor
// travels with the arguments
struct SolveLaunchInfo {
  bool four;
  const SolveUnit* one;
};
// one launch of the device solve on nr = 1, 2 or 4 vectors y[q * ldy + i]
void launch_solve(hipStream_t st, const SolveTablesView& t, const SolveLaunch& l, const SolveLaunchInfo& li, double* y,
                  int nr, int64_t ldy);
// blocked solve for many right-hand sides (solve_many.hip): one launch of the SAME solve program on the
// workspace W[p * rb + q] (pivot position p, right-hand side q < rb; rb = 16 or 32), products on fp64 MFMA
void launch_solve_many(hipStream_t st, const SolveTablesView& t, const SolveLaunch& l, const SolveLaunchInfo& li,
                       double* W, int rb);
// W <- the caller's nv <= rb vectors x[q * ldx + i] (order: user variable i -> pivot position, null = x is in
// pivot order), columns nv .. rb - 1 of W zero; and back (only the nv real vectors are written)
void launch_solve_many_pack(hipStream_t st, const double* x, int64_t ldx, const int* order, int n, int nv, int rb,
                            double* W);
void launch_solve_many_unpack(hipStream_t st, double* x, int64_t ldx, const int* order, int n, int nv, int rb,
                              double* W);
// ---- sparse right-hand sides and selected outputs (solve_sparse.hip), on the workspace W of solve_many ----
constexpr int kSsChunkRows = 1024;   // most rows of one chunk of the touched-row list
// chunks: (first pivot position, length <= kSsChunkRows) pairs on the device; the rows of every chunk <- 0
void launch_ss_zero(hipStream_t st, const int* chunks, int nchunk, int rb, double* W);
// W[pos[i]] = val[i], pos[i] = pivot position * rb + column of the group
void launch_ss_scatter(hipStream_t st, const int64_t* pos, const double* val, int64_t count, double* W);
// x[q * ldx + t] = W[pos[t] * rb + q] for t < nsel, q < nv (pos: pivot positions)
void launch_ss_gather(hipStream_t st, double* x, int64_t ldx, const int* pos, int64_t nsel, int nv, int rb,
                      const double* W);
// part[c * 1024 + i * 32 + j] = sum over the rows p of chunk c of WI[p * rbI + i] WJ[p * rbJ + j] (fp64 MFMA)
void launch_ss_gram(hipStream_t st, const int* chunks, int nchunk, const double* WI, int rbI, const double* WJ, int rbJ,
                    double* part);
// Gij[j * ldg + i] = Gji[i * ldg + j] = the blocks summed in ascending chunk order, i < nvI, j < nvJ (diag: I = J)
void launch_ss_gram_reduce(hipStream_t st, const double* part, int nchunk, int nvI, int nvJ, bool diag, double* Gij,
                           double* Gji, int64_t ldg);
// selected inversion (selinv.hip): one launch of a SelinvProgram (SI_SYMM / SI_SCALE: tiles[first ..];
// SI_DIAG: units[first ..]) on the Z arena; scratch: the program's scratch_size doubles
void launch_selinv(hipStream_t st, const SelinvLaunch& l, const SelinvUnit* units, const UpdTile* tiles,
                   const SelinvRow* rows, const int* relpos, const double* L, const double* dinv, double* Z,
                   double* scratch);
// the SI_SYMM launch with the diagonal of the gathered symmetric block doubled (the factor adjoint)
void launch_selinv_symm_doubled(hipStream_t st, const SelinvLaunch& l, const SelinvUnit* units, const UpdTile* tiles,
                                const SelinvRow* rows, const int* relpos, const double* L, const double* G,
                                double* scratch);
// ---- reverse-mode derivative of the factor (factor_adjoint.hip) --------------------------------------
// a block column for k_fadj_seed: rows rlist[idx_off ..], columns the pivot positions gcol0 .. gcol0 + w - 1
struct FadjCol {
  int64_t off;       // arena offset of the block column
  int64_t idx_off;   // offset into rlist[] of its first row
  int w, nrow;
  int gcol0;
  int pad_;
};
// G[lower position (r_i, c_j)] = (accumulate ? G : 0) + alpha sum_q a[q ld + x(r_i)] b[q ld + x(c_j)], one fma
// chain per entry in ascending q; x(p) = p for a vector in pivot order (order_flags bit 0: a, bit 1: b), else
// porder[p].  tiles: (block column, 64-row strip) pairs (UpdTile: unit, ti)
void launch_fadj_seed(hipStream_t st, const UpdTile* tiles, int64_t ntiles, const FadjCol* cols, const int* rlist,
                      const int* porder, double* G, int nvec, const double* a, const double* b, int64_t ld, double alpha,
                      bool accumulate, int order_flags);
// one launch of the SelinvProgram on the adjoint arena G (arguments as launch_selinv)
void launch_fadj(hipStream_t st, const SelinvLaunch& l, const SelinvUnit* units, const UpdTile* tiles,
                 const SelinvRow* rows, const int* relpos, const double* L, const double* dinv, double* G,
                 double* scratch);
// out[v] = Z[diag_pos[order[v]]]  (diag(A^-1) in the user's variable order)
void launch_selinv_diag_gather(hipStream_t st, const double* Z, const int64_t* diag_pos, const int* order, int n,
                               double* out);
// out[0] = 2 sum_j log L[diag_pos[j]], in a fixed order
void launch_log_det(hipStream_t st, const double* L, const int64_t* diag_pos, int n, double* out);
// ---- batched factorization and solve (batch.hip): nbatch members on one pattern -------------------
// Member b's arena, dinv scratch and flag: L + b * lstride, dinv + b * dstride, flag + b; every table
// is shared.  member_fast: see batch.hip (the order of the workgroups of a launch).  Every wrapper
// returns the number of kernel launches it made: one, unless (work items) x (members) overflows a grid,
// in which case the members are split into ranges; -1 (nothing launched) when ONE member's work items overflow it.
struct BatchView {
  double* L;
  double* dinv;
  int* flag;
  int64_t lstride, dstride;
  int nbatch;
  int member_fast;
};
// test hook: the number of workgroups from which on the members of a launch are split into ranges (<= 0: the
// hardware limit of (2^32 - 1) / 256)
void set_batch_grid_limit(int64_t workgroups);
// arenas cleared, A_b = val[b * ldval ..] copied in (cptr / loc / src: the bucketed value map of
// launch_init_arena), flags set to INT_MAX
int launch_batch_init(hipStream_t st, const BatchView& v, int64_t arena, const double* val, int64_t ldval,
                      const int64_t* cptr, const unsigned short* loc, const int* src);
int launch_batch_chain(hipStream_t st, const BatchView& v, const ChainUnit* units, int64_t count);
// tile = 32 or 64; unit modes DIRECT (exclusive owner), SCATTER, TRSM
int launch_batch_update(hipStream_t st, const BatchView& v, int tile, const UpdTile* tiles, int64_t count,
                        const UpdUnit* units, const int64_t* bc_off, const int* bc_w, const int* relpos,
                        const int* rlist);
// nrhs vectors per member: x[(b nrhs + q) ldx + i] <-> Y[(b nrhs + q) n + p(i)] (order: user variable ->
// pivot position, null = x is in pivot order); members whose flag is set are skipped
int launch_batch_pack(hipStream_t st, const BatchView& v, bool unpack, double* x, int64_t ldx, int nrhs,
                      const int* order, int n, double* Y);
// one launch (kind = SolveKind) of a SolveProgram built with pw = cb = 64 on the workspace Y
int launch_batch_solve(hipStream_t st, const BatchView& v, int kind, const int* list, const UpdTile* tiles,
                       int64_t first, int64_t count, const SolveUnit* units, const int* rlist, double* Y, int nrhs,
                       int n);
// out[b] = 2 sum_j log L_b[diag_pos[j]] in a fixed order; NaN for a member whose flag is set
int launch_batch_log_det(hipStream_t st, const BatchView& v, const int64_t* diag_pos, int n, double* out);
// ---- blocked solve for the members of a batch (batch_solve_many.hip): the kernels of solve_many.hip per member ----
// Member b's workspace: W + b * rb * n, W_b[p * rb + q] (rb = 16 or 32); arena, dinv scratch and flag as above.
// W_b[p(i) * rb + q] = q < nv ? x[b * xstride + q * ldx + i] : 0 (unpack: the other way, q < nv only); a member
// whose flag is set is skipped
int launch_batch_solve_many_pack(hipStream_t st, const BatchView& v, bool unpack, double* x, int64_t xstride, int64_t ldx,
                                 const int* order, int n, int nv, int rb, double* W);
// one launch l of a SolveProgram built with pw = cb = 64 (list / tiles / units: its tables) for all members
int launch_batch_solve_many(hipStream_t st, const BatchView& v, const SolveLaunch& l, const int* list,
                            const UpdTile* tiles, const SolveUnit* units, const int* rlist, double* W, int rb, int n);
// the limit in force (set_batch_grid_limit) and the hardware limit, for the other batched translation units
int64_t batch_grid_limit();
int64_t batch_grid_limit_max();
// ---- bit-reproducible batch (batch_repro.hip): no atomic add anywhere ----------------------------------
// The batch's view plus member b's scratch at scratch + b * sstride: the MODE_BUFFER products of the deterministic
// batch program (factorization), or the stored strip products of a sweep.  When the members of a launch are split
// into ranges the scratch pointer moves with the first member, as L, dinv and flag do.  A member whose flag is set
// is skipped by every kernel before any barrier.  Return values as above.
struct BatchReproView {
  BatchView v;
  double* scratch;
  int64_t sstride;
};
// k_batch_update with the epilogues TRSM, DIRECT and BUFFER (the product stored at scratch_b[u.d_off + i N + j])
int launch_bdet_update(hipStream_t st, const BatchReproView& s, int tile, const UpdTile* tiles, int64_t count,
                       const UpdUnit* units, const int64_t* bc_off, const int* bc_w);
// k_gather for (gather tile, member): the buffered blocks subtracted from their destination tiles, items in table order
int launch_bdet_gather(hipStream_t st, const BatchReproView& s, const GatherTile* tiles, int64_t count,
                       const GatherItem* items, const int* relpos, const int* rlist);
// the tables of build_rsolve_tables for the batch's solve program on the device (shared by all members)
struct RsmTables {
  const int64_t* fslot;    // per block column
  const int64_t* bfirst;   // per block column (-1: no rows below)
  const int64_t* gptr;     // n + 1
  const int64_t* gsrc;     // frows
  const int64_t* bslot;    // per tile of the SolveProgram
};
// launch_batch_solve_many without atomics: a strip stores into member b's scratch (rb * max(frows, bsize) doubles),
// the diagonal launch subtracts the stored products in table order first (rsm_body.hpp)
int launch_batch_solve_repro(hipStream_t st, const BatchReproView& s, const SolveLaunch& l, const int* list,
                             const UpdTile* tiles, const SolveUnit* units, const int* rlist, const RsmTables& tb,
                             double* W, int rb, int n);
// ---- batched selected inversion (batch_selinv.hip): Z_b on the pattern of L for every member ----------
// The batch's view plus member b's inverse arena Z + b * v.lstride (L's layout) and step scratch
// scratch + b * sstride.  The tables are those of a SelinvProgram built with pw = cb = 64 and are shared.
// A member whose flag is set is skipped by every kernel; the two readers write NaN for it.  v.flag may be
// null for the readers: one arena known to be valid.  Return values as above.
struct BatchSelinvView {
  BatchView v;
  double* Z;
  double* scratch;
  int64_t sstride;
};
// one launch of the program (SI_SYMM / SI_SCALE / SI_DIAG) for all members
int launch_batch_selinv(hipStream_t st, const BatchSelinvView& s, const SelinvLaunch& l, const SelinvUnit* units,
                        const UpdTile* tiles, const SelinvRow* rows, const int* relpos);
// one whole step (SYMM + SCALE + DIAG) of units[0 .. count), each with nR <= 64 and nsplit <= 1, in one launch
int launch_batch_selinv_fused(hipStream_t st, const BatchSelinvView& s, const SelinvUnit* units, int64_t count,
                              const SelinvRow* rows, const int* relpos);
// out[b * ldout + i] = Z_b[diag_pos[order[i]]]  (diag(A_b^-1) in the user's variable order)
int launch_batch_selinv_diag_gather(hipStream_t st, const BatchSelinvView& s, const int64_t* diag_pos, const int* order,
                                    int n, double* out, int64_t ldout);
// out[b * ldout + map_src[e]] = Z_b[map_dst[e]]  (A_b^-1 at the entries of the analysed pattern, in the order of val)
int launch_batch_selinv_pattern(hipStream_t st, const BatchSelinvView& s, const int64_t* map_dst, const int64_t* map_src,
                                int64_t nmap, double* out, int64_t ldout);
// the SI_SYMM launch for all members with the diagonal of the gathered symmetric block doubled (the factor
// adjoint of the batch: s.Z is the adjoint arena)
int launch_batch_selinv_symm_doubled(hipStream_t st, const BatchSelinvView& s, const SelinvLaunch& l,
                                     const SelinvUnit* units, const UpdTile* tiles, const SelinvRow* rows,
                                     const int* relpos);
// ---- reverse-mode derivative of the factors of a batch (batch_adjoint.hip) ----------------------------
// The BatchSelinvView with the adjoint arenas in the place of Z: member b's G + b * v.lstride.  Tables, flags
// and return values as above.
// launch_fadj_seed for every member: vector q of member b at a[(b * nvec + q) * ld ..], b likewise
int launch_batch_fadj_seed(hipStream_t st, const BatchSelinvView& s, const UpdTile* tiles, int64_t ntiles,
                           const FadjCol* cols, const int* rlist, const int* porder, int nvec, const double* a,
                           const double* b, int64_t ld, double alpha, bool accumulate, int order_flags);
// one launch of the program (SI_SYMM / SI_SCALE / SI_DIAG) on the adjoint arenas of all members
int launch_batch_fadj(hipStream_t st, const BatchSelinvView& s, const SelinvLaunch& l, const SelinvUnit* units,
                      const UpdTile* tiles, const SelinvRow* rows, const int* relpos);
// one whole adjoint step of units[0 .. count), each with nR <= 64 and nsplit <= 1, in one launch
int launch_batch_fadj_fused(hipStream_t st, const BatchSelinvView& s, const SelinvUnit* units, int64_t count,
                            const SelinvRow* rows, const int* relpos);
// ---- sampled outer product on the analysed pattern (pattern_outer.hip) ---------------------------------
// out[b * ldout + k] = alpha * sum_q ( u_q[i] v_q[j] + [i != j] u_q[j] v_q[i] ) for entry k = (prow[k], pcol[k]) =
// (i, j) of the pattern (0-based user variables) and member b, whose vector q is at u + (b * nvec + q) * ldu;
// one fma chain per entry in ascending q, gather only.  Returns the number of kernel launches as the batched
// wrappers above (the members are split into ranges past the grid limit; -1: one member overflows a grid).
int launch_pattern_outer(hipStream_t st, const int* prow, const int* pcol, int64_t nnz, int nbatch, int nvec,
                         const double* u, int64_t ldu, const double* v, int64_t ldv, double alpha, double* out,
                         int64_t ldout);
// ---- low-rank update / downdate of the factor (updown.hip) ------------------------------------------
// Wd: the work array, n x kUpdownVec doubles, Wd[p * kUpdownVec + q] for pivot position p and vector q of the
// pass, zero between calls.  coef: (widest block column) x kUpdownVec x 3 doubles, the (c, t, 1 / c) of the
// block column in flight.  flag: INT_MAX, or the smallest pivot position + 1 at which a downdate failed.
constexpr int kUpdownVec = 8;      // vectors per pass
constexpr int kUpdownRows = 256;   // rows per workgroup of the apply kernel, one per thread
constexpr int kUpdownChunk = 16;   // columns of L staged through LDS at a time
// Wd[pos[i]] = val[i]; reset_flag: *flag = INT_MAX as well
void launch_updown_scatter(hipStream_t st, const int64_t* pos, const double* val, int64_t count, double* Wd, int* flag,
                           bool reset_flag);
// the diagonal square of block column u (host copy of its SolveUnit; pw = cb <= kPanelMax): coefficients,
// rotations, the dinv slots of its panels; one workgroup
// nv: the vectors of the pass (kernels for 1, 2, 4 and 8: the next of these)
void launch_updown_gen(hipStream_t st, const SolveUnit& u, double* L, double* dinv, double* Wd, double* coef, int* flag,
                       int sign, int nv);
// the rows below the square (nothing is launched when there are none)
void launch_updown_apply(hipStream_t st, const SolveUnit& u, double* L, const int* rlist, double* Wd, const double* coef,
                         int sign, int nv);
// ---- the same for the members of a batch (batch_updown.hip; the bodies of updown.hip per member: ud_body.hpp) ----
// The batch's view (arenas, dinv scratch, the batch's OWN flags) plus member b's work array Wd + b * wstride
// (kUpdownVec n doubles, zero between calls), coefficient scratch coef + b * cstride ((widest block column) x
// kUpdownVec x 3 doubles) and word udflag[b]: INT_MAX, or the smallest pivot position + 1 at which a downdate of this
// call failed.  v.flag[b] is merged from udflag[b] by the scatter launch of the NEXT pass (and by the host after
// the last one): it does not change while the block columns of a pass run, so the two exits below are uniform
// per (pass, member).  A generate workgroup leaves at once, before it reads L, when its member's v.flag is set, or
// when all kUpdownVec slots of its Wd at the block column's own columns compare equal to zero (the block column is
// an identity for that member); it then stores kBupdownSkip in coef[b * cstride], which the apply workgroups of
// that (block column, member) read.  Every wrapper returns the launches made (the members split into ranges as in
// batch_split.hpp), -1 when one member's work items overflow a grid.
struct BupdownView {
  BatchView v;
  double* Wd;
  double* coef;
  int* udflag;
  int64_t wstride, cstride;
};
constexpr double kBupdownSkip = -1.0;   // (c = r / d of a rotation is positive)
// Wd[b * wstride + pos[i]] = wval[b * ldw + ent[i]], i < count, for every member whose flags are clear; member b's
// thread 0 first merges udflag[b] into v.flag[b] (reset: sets udflag[b] = INT_MAX instead -- the first pass)
int launch_bupdown_scatter(hipStream_t st, const BupdownView& s, const int64_t* pos, const int* ent, int64_t count,
                           const double* wval, int64_t ldw, bool reset);
// one workgroup per member: the diagonal square of block column u (a SolveUnit of the batch's solve program, pw = 64)
int launch_bupdown_gen(hipStream_t st, const BupdownView& s, const SolveUnit& u, int sign, int nv);
// (strips x members) workgroups: the rows below the square; 0 when there are none
int launch_bupdown_apply(hipStream_t st, const BupdownView& s, const SolveUnit& u, const int* rlist, int sign, int nv);
// ---- sparse right-hand sides for the members of a batch (batch_solve_sparse.hip; the bodies of solve_sparse.hip
// per member: ss_body.hpp) ----
// The batch's flags and member count; member b's workspace at W + b * wstride.  The lists (chunks, pos) are shared
// by all members.  A flagged member's workspace is never touched; its outputs (gather, gram_reduce) are NaN.  Every
// wrapper returns the launches made (the members split into ranges as in batch_split.hpp), -1 when one member's
// work items overflow a grid.
struct BssView {
  const int* flag;
  int nbatch;
};
int launch_bss_zero(hipStream_t st, const BssView& s, const int* chunks, int nchunk, int rb, double* W, int64_t wstride);
// W_b[pos[i]] = val[b * ldv + i], i < count (ldv = 0: one set of values)
int launch_bss_scatter(hipStream_t st, const BssView& s, const int64_t* pos, const double* val, int64_t ldv,
                       int64_t count, double* W, int64_t wstride);
// x[b * xstride + q * ldx + t] = W_b[pos[t] * rb + q] for t < nsel, q < nv
int launch_bss_gather(hipStream_t st, const BssView& s, double* x, int64_t xstride, int64_t ldx, const int* pos,
                      int64_t nsel, int nv, int rb, const double* W, int64_t wstride);
// part[(b * nchunk + c) * 1024 + i * 32 + j] = the product of chunk c's rows of member b's two workspaces
int launch_bss_gram(hipStream_t st, const BssView& s, const int* chunks, int nchunk, const double* WI, int64_t wsI, int rbI,
                    const double* WJ, int64_t wsJ, int rbJ, double* part);
// launch_ss_gram_reduce for every member: G_b at Gij / Gji + b * gstride
int launch_bss_gram_reduce(hipStream_t st, const BssView& s, const double* part, int nchunk, int nvI, int nvJ, bool diag,
                           double* Gij, double* Gji, int64_t gstride, int64_t ldg);
// ---- reproducible substitution (solve_repro.hip): launch_solve without atomic adds ------------------
// The RsolveTables (schedule.hpp) on the device and the scratch: vector q of a sweep uses scratch + q * stride,
// stride >= max(frows, bsize).
struct RsolveView {
  const int64_t* fslot;    // per block column
  const int64_t* bfirst;   // per block column
  const int64_t* gptr;     // n + 1
  const int64_t* gsrc;     // frows
  const int64_t* bslot;    // per tile
  double* scratch;
  int64_t stride;
};
// one launch of the SolveProgram, arguments as launch_solve
void launch_solve_repro(hipStream_t st, const SolveTablesView& t, const SolveLaunch& l, const SolveLaunchInfo& li,
                        double* y, int nr, int64_t ldy, const RsolveView& rv);
// ---- products with the factor and Gaussian noise (factor_mult.hip) ----------------------------------
// The RsolveTables on the device and the scratch of the products: slot s of the tables is the row
// scratch[s * rb .. s * rb + rb) of a block of rb vectors, rb * max(frows, bsize) doubles in all.
struct FmultView {
  const int64_t* fslot;    // per block column
  const int64_t* bfirst;   // per block column
  const int64_t* gptr;     // n + 1
  const int64_t* gsrc;     // frows
  const int64_t* bslot;    // per tile
  double* scratch;
};
// Y = L X (transpose: L^T X) on the workspaces X[p * rb + q], Y[p * rb + q] (X != Y), rb = 16 or 32: one
// launch over all ntiles tiles of the SolveProgram (t.tiles) and one over the nchunks (block column, 64
// pivot positions) pairs of `chunks` (UpdTile: unit, ti = chunk); no atomic add
void launch_factor_mult(hipStream_t st, const SolveTablesView& t, int64_t ntiles, const UpdTile* chunks, int64_t nchunks,
                        bool transpose, const double* X, double* Y, int rb, const FmultView& fv);
// z[q * ldz + i] = the standard normal of (pivot position order[i] (null: i), sample first + q, seed), q < nsamp
void launch_white_noise(hipStream_t st, double* z, int64_t ldz, const int* order, int n, int nsamp, uint64_t seed,
                        uint64_t first);
// x[q * ldx + i] += mean[i], q < nvec
void launch_add_mean(hipStream_t st, double* x, int64_t ldx, const double* mean, int n, int nvec);
// ---- the same for every member of a batch (batch_mult.hip) -------------------------------------------
// Member b: arena L + b * lstride (the layout of the single arena: the tables of the handle's SolveProgram apply),
// flag[b], workspaces X + b * wstride and Y + b * wstride (wstride = rb * n), scratch fv.scratch + b * sstride.
// A member whose flag is set is skipped by every kernel of a product, pack and unpack included.
// member_fast: 0 = the member is the slow grid axis (the workgroups of one member are consecutive), 1 = the
// members of one work item are consecutive.  Every wrapper returns the number of kernel launches it made: the
// members are split into ranges above 65535 (the y extent of a grid) and above batch_grid_limit() workgroups.
struct BmultView {
  const double* L;
  const int* flag;
  int64_t lstride, wstride, sstride;
  int nbatch;
  int member_fast;
};
// W_b[p(i) * rb + q] = q < nv ? x[b * xstride + q * ldx + i] : 0 (unpack: the other way, q < nv only)
int launch_batch_mult_pack(hipStream_t st, const BmultView& v, bool unpack, double* x, int64_t xstride, int64_t ldx,
                           const int* order, int n, int nv, int rb, double* W);
// Y_b = L_b X_b (transpose: L_b^T X_b): two launches for all members, arguments as launch_factor_mult
int launch_batch_mult(hipStream_t st, const BmultView& v, const SolveTablesView& t, int64_t ntiles, const UpdTile* chunks,
                      int64_t nchunks, bool transpose, const double* X, double* Y, int rb, const FmultView& fv);
// z[b * zstride + q * ldz + i] = the standard normal of (pivot position order[i] (null: i), stream stream0 +
// b * stream_step, sample first + q, seed); NaN for a member whose flag is set
int launch_batch_white_noise(hipStream_t st, const BmultView& v, double* z, int64_t zstride, int64_t ldz, const int* order,
                             int n, int nsamp, uint64_t seed, uint64_t first, uint32_t stream0, int stream_step);
// x[b * xstride + q * ldx + i] += mean[b * ldmean + i], q < nvec (ldmean = 0: one mean for all members)
int launch_batch_add_mean(hipStream_t st, const BmultView& v, double* x, int64_t xstride, int64_t ldx, const double* mean,
                          int64_t ldmean, int n, int nvec);
void launch_expand_buffer(hipStream_t st, double* a, int blkn, const int* row_list, int rls,
                          const int* col_list, int cls, int ndiag, const double* buffer);
// ---- hard linear constraints C x = e (constrain.hip; user order throughout, no atomic add) ---------------------
// C: k <= kCnMaxRows rows of n at C + i * ldc; vectors as solve_many (vector q at X + q * ldx); U as the vectors (column j
// at U + j * ldu); G: the lower Cholesky factor of S = C W, G[i * kCnMaxRows + j], zero above the diagonal and behind k.
// The n positions are cut into chunks of cn_chunk(n) (a multiple of 64; at most 256 chunks): a product's partial
// of chunk c is part[(c * kCnMaxRows + i) * ldp + q], ldp = kCnPass for a pass of vectors and kCnMaxRows for S.
constexpr int kCnMaxRows = 64, kCnPass = 32;
int cn_chunk(int n);
inline int cn_nchunks(int n) { return n > 0 ? (n + cn_chunk(n) - 1) / cn_chunk(n) : 0; }
// part = C X^T per chunk for nv <= ldp vectors; lower: only the 16 x 16 tiles on and below the diagonal (S = C W)
void launch_cn_dot(hipStream_t st, const double* C, int64_t ldc, int k, const double* X, int64_t ldx, int nv, int n,
                   double* part, int ldp, bool lower);
// S = the sum of the partials in chunk order (lower triangle, mirrored), S = G G^T in one workgroup.  stat[0] = log det S,
// stat[1] = min_j pivot_j / S_jj, stat[2] = 0 or the 1-based row j whose pivot is <= 2^-26 S_jj or not finite
void launch_cn_chol(hipStream_t st, const double* part, int nchunks, int k, double* G, double* stat);
// U <- U G^-T in place (on entry U = W): every position an independent forward substitution over k
void launch_cn_scale(hipStream_t st, double* U, int64_t ldu, int n, int k, const double* G);
// r = (the sum of the partials in chunk order) - e, t = G^-1 r into T[q * kCnMaxRows + j] (zero behind k and nv), and
// lambda[q * ldl + j] = (G^-T t)_j when lambda is given.  e: null (zeros), lde = 0 (shared) or per vector.
void launch_cn_small(hipStream_t st, const double* part, int nchunks, int k, int nv, const double* G, const double* e,
                     int64_t lde, double* T, double* lambda, int64_t ldl);
// X[q * ldx + p] -= sum_j U[j * ldu + p] T[q * kCnMaxRows + j], q < nv <= kCnPass: one read and one write of X
void launch_cn_apply(hipStream_t st, double* X, int64_t ldx, int nv, int n, const double* U, int64_t ldu, int k,
                     const double* T);
// out[i] = zdiag[i] - sum_j U[j * ldu + i]^2, j ascending (out may be zdiag)
void launch_cn_var(hipStream_t st, const double* zdiag, const double* U, int64_t ldu, int n, int k, double* out);
// ---- the same for the members of a batch (constrain_batch.hip): the bodies of the kernels above (cn_body.hpp) on the
// arrays of member b, the member from the last grid dimension; a member whose flag is not INT_MAX is neither read nor
// written.  C is shared; everything else has a fixed stride per member.  Every launcher returns the launches made (0:
// nothing to do) or -1 when the members do not fit a grid dimension (nothing launched).
constexpr int kBcnStat = 4;   // doubles of scalars per member: log det S_b, min pivot_j / S_jj, the failed row, unused
struct BcnView {
  const int* flag;   // the batch's flags
  int nbatch, n, k;
  const double* C;   // k x n, row i at C + i * n
  double* U;         // member b at U + b * k * n, column j of U_b at + j * n
  double* G;         // member b at G + b * kCnMaxRows^2
  double* stat;      // member b at stat + b * kBcnStat
  double* part;      // member b at part + b * pstride, laid out as the single handle's
  double* T;         // member b at T + b * kCnPass * kCnMaxRows
  int64_t pstride;   // cn_nchunks(n) * kCnMaxRows^2
};
int launch_bcn_bcast(hipStream_t st, const BcnView& v);   // U_b = C (that is W_b = C^T before the solve) for every member
// member b's vectors at X + b * xstride, vector q at + q * ldx
int launch_bcn_dot(hipStream_t st, const BcnView& v, const double* X, int64_t xstride, int64_t ldx, int nv, int ldp,
                   bool lower);
int launch_bcn_chol(hipStream_t st, const BcnView& v);
int launch_bcn_scale(hipStream_t st, const BcnView& v);
// e: null, or member b's at e + b * estride, vector q's at + q * lde (lde = 0: one column); lambda alike, or null
int launch_bcn_small(hipStream_t st, const BcnView& v, int nv, const double* e, int64_t estride, int64_t lde,
                     double* lambda, int64_t lstride, int64_t ldl);
int launch_bcn_apply(hipStream_t st, const BcnView& v, double* X, int64_t xstride, int64_t ldx, int nv);
// member b's row at zdiag + b * ld and out + b * ld (out may be zdiag)
int launch_bcn_var(hipStream_t st, const BcnView& v, const double* zdiag, int64_t ld, double* out);

}  // namespace spx
