/*
 * spllt_hip.h -- additions of libspllt_hip.so next to the drop-in ABI of
 * spllt_iface.h.  Two groups:
 *
 *  (1) the per-kernel operator API.  The reference already exposes its factor
 *      kernels as bind(C) routines for the StarPU/PaRSEC task bodies
 *      (src/spllt_kernels_mod.F90:1193,1233,1295,2055,2241 and the CUDA launcher
 *      src/StarPU/expand_buffer_kernels.cu:48-62).  These are their
 *      stream-taking twins: same argument meaning, device pointers, plain
 *      index arrays instead of Fortran derived-type handles, asynchronous on
 *      the given HIP stream (passed as void* so that the header needs no HIP).
 *
 *  (2) engine control / introspection used by benchmarks and tests
 *      (exact 64-bit statistics, device-resident factorization, L download,
 *      export of the symbolic structure and of the stream-DAG program).
 */
#ifndef SPLLT_HIP_H
#define SPLLT_HIP_H
#include <stdint.h>

#include "spllt_iface.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- (1) kernel operators: all pointers are DEVICE pointers ---------------- */

/* twin of spllt_factor_diag_block_c(m, n, bc) (kernels_mod:1193): Cholesky of
 * the n x n head of a row-major m x n diagonal tile and the triangular solve
 * of its m-n trailing rows.  *dev_flag (int, device) receives min(column+1) of
 * a non-positive pivot, untouched otherwise (initialise it to INT_MAX). */
int spllt_factor_diag_block_hip(void *stream, int m, int n, double *bc, int *dev_flag);

/* twin of spllt_solve_block_c(m, n, bc_kk, bc_ik) (kernels_mod:1233):
 * bc_ik <- bc_ik * L_kk^-T, bc_ik is m x n row-major, bc_kk the factored n x n tile. */
int spllt_solve_block_hip(void *stream, int m, int n, const double *bc_kk, double *bc_ik);

/* twin of spllt_update_block_c(m, n, dest, isDiag, n1, src1, src2)
 * (kernels_mod:1295): dest -= src2 * src1^T; src1 is n x n1, src2 is m x n1. */
int spllt_update_block_hip(void *stream, int m, int n, double *dest, int is_diag, int n1,
                           const double *src1, const double *src2);

/* twin of spllt_update_between_c (kernels_mod:2241) with the index lists of
 * spllt_update_between_compute_map_c (:1725) passed explicitly and the
 * spllt_expand_buffer_c step (:2055) fused into the GEMM epilogue:
 *   dest[row_list[i]*blkn + col_list[j]] -= sum_k rsrc[i][k] * csrc[j][k],
 * i < rls, j < (i < ndiag ? i+1 : cls); csrc is cls x n1, rsrc is rls x n1,
 * row_list/col_list are 0-based device arrays. */
int spllt_update_between_hip(void *stream, double *dest, int blkn, int n1, const double *csrc,
                             int cls, const double *rsrc, int rls, const int *row_list,
                             const int *col_list, int ndiag);

/* twin of spllt_expand_buffer_c (kernels_mod:2055) / spllt_cu_expand_buffer
 * (StarPU/expand_buffer_kernels.cu:48): a[row_list[j]*blkn + col_list[i]] +=
 * buffer[j*cls + i], i < (j < ndiag ? j+1 : cls). */
int spllt_expand_buffer_hip(void *stream, double *a, int blkn, const int *row_list, int rls,
                            const int *col_list, int cls, int ndiag, const double *buffer);

/* twin of spllt_scatter_block (kernels_mod:1122): dest -= src with row/column
 * positions located in the destination index lists (all sorted, device). */
int spllt_scatter_block_hip(void *stream, int s_m, int s_n, const int *rsrc_index,
                            const int *csrc_index, const double *src, int lds,
                            const int *rdest_index, int d_m, const int *cdest_index, int d_n,
                            double *dest, int ldd);

/* twin of spllt_init_node_c / spllt_init_blk_c (kernels_mod:2367, :2425) for
 * the whole arena: L[dst[i]] = val[src[i]], i < n (L zeroed by the caller). */
int spllt_init_lfact_hip(void *stream, double *L, const double *val, const int64_t *dst,
                         const int64_t *src, int64_t n);

/* ---- (1b) matrix file readers ------------------------
 * What the reference keeps beside the path for its drivers: MatrixMarket coordinate files
 * (src/spllt_mod.F90:426-491 mm_double_read + :543-620 coo_to_csc_double) and Rutherford-Boeing
 * files of assembled symmetric matrices (SPRAL rb_read as the drivers call it,
 * drivers/spllt_omp.F90:78-85).  Both return the LOWER triangle as 1-based CSC with sorted
 * rows -- the arguments of spllt_analyse / spllt_factor -- in malloc'ed arrays that
 * spllt_hip_free_matrix releases.  values: 0 = as in the file (a pattern-only file is an error),
 * 3 = the drivers' rb_options%values = 3: off-diagonal values as in the file, or made up
 * (uniform in (-1, 1), splitmix64 from `seed`; the reference: SPRAL random_real,
 * spllt_mod.F90:480-485) for a pattern-only file, every diagonal entry 1 + the sum of the
 * |off-diagonal entries| of its row.  A general MatrixMarket matrix is read as (A + A^T) / 2.
 * Returns 0 or an SPLLT error flag (message on stderr). */
int spllt_hip_read_rb(const char *path, int values, int seed, int *n, int *nnz, int **ptr, int **row,
                      double **val);
int spllt_hip_read_mm(const char *path, int values, int seed, int *n, int *nnz, int **ptr, int **row,
                      double **val);
void spllt_hip_free_matrix(int *ptr, int *row, double *val);

/* ---- (2) engine control / introspection ----------------------------------- */

typedef struct {
  int64_t n, nnz_a, nnodes, nbcol, nblk, arena, nnz_l, flops, rlist_len;
  int nb, maxmn, maxdepth, nlevels;
  char ordering[16];
} spllt_hip_sym_info_t;

/* analyse with a caller-supplied pivot order (order_in[i] = 1-based position
 * of variable i; NULL = built-in nested dissection).  Otherwise identical to
 * spllt_analyse. */
void spllt_hip_analyse_ordered(void **akeep, void **fkeep, spllt_options_t *options, int n,
                               const int *ptr, const int *row, spllt_inform_t *info, int *order,
                               const int *order_in);

/* analyse from a complete symbolic factorization: the quintuple SpLLT's own spllt_analyse
 * takes from SSIDS (akeep%sptr, %sparent, %rptr, %rlist and the pivot order, reference
 * src/spllt_analyse_mod.F90:129-158), all 1-based exactly as SSIDS delivers them: sptr
 * (nnodes+1), sparent (nnodes, virtual root = nnodes+1), rptr (nnodes+1, 64-bit), rlist
 * (pivot positions, sorted per node, the node's own columns first), order_in[i] = position
 * of variable i.  The factorization then uses exactly SSIDS' supernode partition and
 * assembly tree (no ordering, supernode detection or amalgamation of our own), so a
 * reference build that keeps SPRAL/Metis for the analyse gets the same tree on both paths.
 * Invalid input (not a permutation, nodes not postordered, unsorted row lists, pattern of A
 * not covered) -> info->flag = SPLLT_ERROR_PARAMETER. */
void spllt_hip_analyse_symbolic(void **akeep, void **fkeep, spllt_options_t *options, int n,
                                const int *ptr, const int *row, spllt_inform_t *info, int nnodes,
                                const int *sptr, const int *sparent, const int64_t *rptr,
                                const int *rlist, const int *order_in);

int spllt_hip_sym_info(const void *akeep, spllt_hip_sym_info_t *out);
/* copy a named 0-based array of the symbolic structure; returns its length in
 * elements (call with buf = NULL to query).  int32 arrays: "order", "sptr",
 * "sparent", "rlist", "small", "level", "bcol_node", "bcol_width", "bcol_r0",
 * "bcol_nrow"; int64 arrays: "rptr", "bcol_off", "map_dst", "map_src",
 * "lmap_ptr", "weight". */
int64_t spllt_hip_sym_get(const void *akeep, const char *name, void *buf, int64_t capacity);

/* engine knobs (before the first spllt_factor on this fkeep); flags: bit 0 =
 * reserved, bit 1 = single-stream program (no lookahead, program order),
 * bit 6 = issue the inter-node updates only at the end of each level (default:
 * in K slices on a separate stream while the level's panel chains still run),
 * bit 7 = debug: the LDS of every CU is filled with signalling NaNs before every
 * kernel launch (a kernel that reads LDS it has not written then computes NaNs),
 * bit 8 = no CU reservation (the default since round 4; SPLLT_HIP_RESERVE_CUS=32 masks the
 * streams that carry the trailing updates off the last 32 CUs, which the latency-critical
 * panel-chain kernels then find free: 0.6 % on the bench workload, and CU-masked streams are
 * what rocprofv3 crashes on at exit).  Bit 9 = no fused panel launches: by default a panel step whose block columns have
 * few rows below the panel (at most 64 blocks of 64 rows in the launch) runs as ONE kernel -
 * every workgroup factors the 64 x 64 diagonal block itself, solves its own rows and applies
 * the left-looking update of the next panel's columns to them - instead of a POTRF, a TRSM
 * and an update launch (used when the chain block is one panel, the default).
 * Bit 10 / bit 11 = force the zone pipeline on / off (inter-node updates at the end
 * of a level issued by destination block column so that the next level's panel chains
 * start beside them; default: on for latency-bound problems, see schedule.hpp).
 * Bit 12 = deterministic engine: no atomic adds anywhere in the factorization.  The
 * inter-node updates store their products in a scratch buffer and one workgroup per
 * destination tile subtracts them in a fixed order (the reference's buffer + expand_buffer
 * steps, serialised per destination like its OpenMP path, task_mod:1239-1241); two
 * factorizations of the same values then give bit-identical factors.  Implies no zone
 * pipeline and no early slices.
 * Bit 13 / bit 14 = (multi-GPU) top tree distributed over the ranks / replicated on every rank
 * (default: by the weight of the top tree, see spllt_hip_set_partition).
 * Bit 15 / bit 16 = HIP-graph replay of the factorization (analyse once, factorize many): one
 * graph per pattern built from the program tables, a chain of kernel nodes in program order / the
 * DAG of the multi-stream program; bit 17 = eager launches.  Default: by problem size -- up to
 * 40 GFLOP the chain replay, and for it the SINGLE-STREAM program (a chain runs in program order
 * anyway: no zones, slices, markers or events -- 27 instead of 36 kernels on BASELINE config 1):
 * 0.22 vs 0.48 ms eager at the smoke size, 0.36 vs 0.69 ms on BASELINE config 1, 2.80 vs 3.28 ms at
 * 19 GFLOP, 4.02 vs 4.66 ms at 33 GFLOP; eager launches above (level at 313 GFLOP: on ROCm 7.2
 * hipGraphLaunch submits nothing before all nodes are enqueued; 25.1 / 24.4 ms against 23.7 eager
 * on the 650 launches of the bench workload).  SPLLT_CHAIN_GRAPH_SERIAL=0 keeps the multi-stream
 * program under the chain replay.
 * Bit 18 / bit 19 = small subtrees as single device tasks on / off (L_SUBTREE, k_subtree: one
 * workgroup factorizes a whole subtree of one-panel nodes in post-order, what leaves the subtree
 * goes through a private generated element and reaches the ancestors in ONE extend-add from the
 * subtree's root -- the reference's pruned-subtree task, src/spllt_factorization_mod.F90:39-261).
 * Default off: slower than the level-batched launches at every size and budget measured
 * (profiles/r04/subtree_tasks_ab.txt); env SPLLT_SUBTREES=1, SPLLT_SUBTREE_US=<modelled us per task>.
 * Single-GPU, non-deterministic engines only.
 * Bits 2-5 selected round-1 experiments that have been removed.
 * Every variant produces the same factor (tests/test_gpu_parity.py). */
int spllt_hip_set_engine(void *fkeep, int panel_width, int tile, int flags);
/* Accepted and ignored.  (It set the edge of diagonal sub-tiles that a single-workgroup chain
 * kernel walked, several panels per sub-tile; that variant was slower at every setting and has
 * been removed: the chain block is always one panel.) */
int spllt_hip_set_chain_block(void *fkeep, int chain_block);

/* ---- multi-GPU: one process per GPU, subtree partition ----------------------
 * Call after spllt_analyse (options.prune_tree = 1, options.ncpu = nranks) and
 * before the first spllt_factor.  Every rank factorizes the pruned subtrees it
 * owns; spllt_factor then stops at the first EXCHANGE point of the rank's program.  The
 * caller drives the exchanges:
 *
 *   spllt_hip_factor_dev(...);
 *   while ((k = spllt_hip_pending_exchange(fkeep)) >= 0) {
 *     <collective of exchange k on the exchange buffer, enqueued on spllt_hip_engine_stream>
 *     spllt_hip_continue(fkeep);        // unpack, enqueue up to the next exchange, pack
 *   }
 *   spllt_hip_wait(fkeep);
 *
 * Exchange k is described by spllt_hip_program_get "exchanges" (int64 x 5: kind, first item,
 * items, elems, chunk) and "xitems" (int64 x 6: block column, root, offset in the buffer, count,
 * offset in the arena or the dinv scratch, space 0 = arena / 1 = dinv scratch); every rank
 * has the same list.  kind 0: all-reduce(sum) of buffer[0:elems] - the extend-add of the whole
 * top tree (replaces spllt_scatter_block on generated elements, reference
 * src/spllt_factorization_mod.F90:39-191; the last element carries the "not positive definite"
 * indicator); the top tree is then factorized on every rank (replicated).
 * Distributed top tree (engine flag bit 13, or chosen by the engine when the top tree is
 * heavy): kind 1: reduce-scatter(sum) of the REGION buffer[base:elems], base = elems - nranks *
 * chunk, in nranks chunks, rank r receives chunk r AT buffer[base + r*chunk : base + (r+1)*chunk]
 * (the block columns of ONE LEVEL of the top tree that r owns: there is one such exchange per
 * level of the top tree, lowest level first, each with a region of its own, so that the lowest
 * level is factorized while the chunks of the levels above travel; spllt_hip_exchange_stream);
 * kind 2:
 * for every root with items, broadcast of that root's segment of the buffer (its items are
 * contiguous) - the block columns of a finished step go from their owners to all ranks, which
 * then update the destination block columns they own; kind 3: all-reduce(sum) of buffer[0:1],
 * the "not positive definite" indicator, at the very end.
 * exchange_elems: doubles the exchange buffer must hold (all reduce regions + the largest broadcast). */
int spllt_hip_set_partition(void *fkeep, int rank, int nranks, int64_t *exchange_elems);
/* The collectives INSIDE the library: hand over the caller's RCCL communicator (ncclComm_t, one
 * rank per GPU, its rank / size = the partition's) after spllt_hip_set_partition.  From then on
 * the unchanged spllt_iface.h calls are all a C or Fortran caller needs: spllt_factor enqueues
 * the rank's subtrees, every exchange of the program (all-reduce of the top tree, or
 * reduce-scatter to the owners + one broadcast per block-column step, and the flag) between its
 * pack and unpack on the engine's stream, and the top tree; spllt_wait drains it; spllt_solve
 * (job 0) adds the two all-reduces of the right-hand sides.  The exchange buffer is then the
 * library's own.  What the reference's distributed build keeps inside the library too
 * (src/PaRSEC/spllt_parsec_blk_data.c:33-64, factorize.jdf).  librccl is resolved at run time
 * from the copy the process already uses.  NULL detaches (the caller drives the exchanges again,
 * spllt_hip_pending_exchange / spllt_hip_continue). */
int spllt_hip_set_communicator(void *fkeep, void *nccl_comm);
/* index of the exchange the handle is waiting for (-1: none, the program has been enqueued
 * to its end) */
int spllt_hip_pending_exchange(void *fkeep);

/* Substitution on DEVICE vectors in pivot order: y_dev holds nrhs vectors of
 * length n, y[q*n + p(i)] = b_q[i], p = 0-based pivot position ("order" of spllt_hip_sym_get); overwritten by the solution in the same
 * order.  job as spllt_solve (0 both sweeps, 1 forward, 2 backward; reference
 * src/spllt_solve_mod.F90:203-221).  phase = -1: the whole solve (single GPU).
 * On a partitioned factor the solve runs in three phases with the caller's
 * exchange, like the factorization:
 *   y = b on the entries this rank owns (own subtrees; rank 0 also the top tree), 0 elsewhere
 *   phase 0 (forward, own subtrees)            -> all-reduce(sum) of y over the ranks
 *   phase 1 (top tree, forward and backward), phase 2 (backward, own subtrees)
 *   zero the entries this rank does not own    -> all-reduce(sum): x on every rank.
 * spllt_solve itself returns SPLLT_ERROR_UNIMPLEMENTED on a partitioned factor. */
int spllt_hip_solve_dev(void *fkeep, void *y_dev, int nrhs, int job, int phase);
/* ---- blocked solve for many right-hand sides (single GPU) ---------------------
 * The substitution of spllt_solve on blocks of 32 right-hand sides per sweep (a tail of at most 16:
 * one block of 16), products on the fp64 matrix cores, so that L is read once per block instead of
 * once per four vectors.  X holds nrhs vectors, vector q at x[q*ldx .. q*ldx + n), ldx >= n,
 * overwritten by the solution; entries outside those ranges are neither read nor written, and a
 * tail that does not fill a block is padded inside the library.  job as spllt_solve (0 both sweeps,
 * 1 forward, 2 backward).  nrhs = 0 is a no-op.  The permutation to pivot order and the transposition
 * into the workspace (n*32 doubles, allocated on first use, kept with the handle) happen on the
 * device.  The work is ordered on the engine's stream (spllt_hip_engine_stream) and has finished
 * when the call returns.  A later factorization on the handle is picked up.
 * Reproducibility: the row strips add into the right-hand sides with fp64 atomic adds, like
 * spllt_solve: two runs agree to rounding, not bit for bit (spllt_hip_solve_repro below is the solve that
 * repeats bit for bit; spllt_hip_set_reproducible_solve does not change this entry point).
 * Errors: null pointer, nrhs < 0, ldx < n, bad job, nothing factorized yet -> SPLLT_ERROR_PARAMETER;
 * partitioned factor (spllt_hip_set_partition with nranks > 1) -> SPLLT_ERROR_UNIMPLEMENTED; no
 * device memory for the workspace -> SPLLT_ERROR_ALLOCATION (the factor and spllt_solve stay
 * usable).  Messages: spllt_hip_last_error. */
int spllt_hip_solve_many(void *fkeep, int nrhs, double *x_host, int64_t ldx, int job);      /* host, user order */
int spllt_hip_solve_many_dev(void *fkeep, int nrhs, double *x_dev, int64_t ldx, int job,
                             int pivot_order);   /* device; 0 = user order, 1 = pivot order as spllt_hip_solve_dev */
/* ---- reproducible solve (single GPU) --------------------------------------------
 * The substitution of spllt_solve -- the same block columns, the same (block column, strip) tiles, the same
 * launch order -- with no atomic add: a row strip STORES its products into a scratch vector, and the launch
 * that solves with a diagonal tile first subtracts the stored products from its rows in an order fixed by
 * tables built from the symbolic structure alone (spllt_hip_program_get, all int64, offsets in doubles
 * inside the scratch of ONE vector):
 *   "rsolve_fslot"  per block column b: slot of the product for its first row below the diagonal tile
 *                   (block column row w); rows w .. nrow-1 take consecutive slots
 *   "rsolve_frows"  scalar: slots in all, the sum of nrow - w
 *   "rsolve_gptr"   n + 1, "rsolve_gsrc" frows: for pivot position p, gsrc[gptr[p] .. gptr[p+1]) are the
 *                   slots subtracted from y[p], ascending by source block column (elimination order).  On the
 *                   device 16 lanes share a list: lane s adds the entries s, s + 16, ... in that order, the
 *                   16 sums are combined by a fixed butterfly, the total is subtracted from y[p]
 *   "rsolve_bslot"  per entry of "solve_tiles": offset of the w column sums the strip produces in the
 *                   backward sweep; "rsolve_bsize": scalar, their total.  The strips of one block column are
 *                   consecutive: strip t at "rsolve_bfirst"[b] + t * w (per block column, -1 without rows
 *                   below); they are subtracted in ascending t.
 * The promise: the same factor bits and the same right-hand-side bits give the same solution bits -- across
 * calls, across group sizes (a vector's arithmetic does not depend on how many vectors share its sweep nor
 * on its position among them), across the host / device / pivot-order entry points, and across handles
 * with the same analysis and engine settings.  The limit: a bit-identical FACTOR across runs still needs
 * engine flag 4096 (spllt_hip_set_engine); with the default engine the factor itself varies in its last bits.
 * Layout, job, nrhs = 0, stream ordering and pickup of a later factorization or spllt_hip_updown as
 * spllt_hip_solve_many above; vectors are swept 4, 2 or 1 at a time; the permutation between user and pivot
 * order is a bitwise copy on the device.  On first use the tables, a scratch of 4 * max(rsolve_frows,
 * rsolve_bsize) doubles and a staging block of 4 n doubles are taken from the device pool and kept until
 * spllt_hip_release_solve_repro or spllt_deallocate_fkeep.
 * Errors: null pointer, nrhs < 0, ldx < n, bad job, nothing factorized yet -> SPLLT_ERROR_PARAMETER;
 * partitioned handle -> SPLLT_ERROR_UNIMPLEMENTED; no device -> SPLLT_ERROR_HIP; no device memory ->
 * SPLLT_ERROR_ALLOCATION (nothing is kept half-allocated, the factor and every other solve stay usable).
 * Messages: spllt_hip_last_error.  Debug: spllt_hip_debug("rsolve_poison=1") fills the scratch with NaN
 * before every sweep ("=0": off), so that a slot read without having been written shows up in the result. */
int spllt_hip_solve_repro(void *fkeep, int nrhs, double *x_host, int64_t ldx, int job);      /* host, user order */
int spllt_hip_solve_repro_dev(void *fkeep, int nrhs, double *x_dev, int64_t ldx, int job,
                              int pivot_order);   /* device; 0 = user order, 1 = pivot order as spllt_hip_solve_dev */
/* on != 0: spllt_solve (single GPU), spllt_hip_solve_dev(phase = -1) and every M^-1 of
 * spllt_hip_solve_refined* (for every group size, in sweeps of 4) go through the reproducible path; a
 * refined solve is then bit-reproducible as a whole.  spllt_hip_solve_many* is NOT affected by the switch.
 * Returns the PREVIOUS setting (0 / 1) or a negative flag (null handle: SPLLT_ERROR_PARAMETER; switching on
 * for a partitioned handle: SPLLT_ERROR_UNIMPLEMENTED).  Default 0.  Needs no device. */
int spllt_hip_set_reproducible_solve(void *fkeep, int on);
int spllt_hip_release_solve_repro(void *fkeep);   /* tables and scratch back to the pool */
/* ---- products with the factor (single GPU) ----------------------------------------
 * The calls that APPLY the factor in the arena, where the solves invert it.  X holds nvec vectors laid out as
 * in spllt_hip_solve_many (vector q at x[q*ldx .. q*ldx + n), ldx >= n, overwritten in place, nothing outside
 * those ranges read or written).  The job numbers mirror spllt_solve, so that factor_mult(job) undoes
 * solve_many(job) and the other way round:
 *   job 0   x <- P^T L L^T P x   the product with the matrix the factor stands for (after spllt_hip_updown:
 *                                A +- W W^T, for which no value array exists)
 *   job 1   x <- P^T L x         the input is a pivot-order vector laid out in user positions, exactly as
 *                                solve_many(job = 1) leaves it
 *   job 2   x <- L^T P x         the mirror: what solve_many(job = 2) takes
 * pivot_order = 1 skips both permutations, as in spllt_hip_solve_many_dev.  nvec = 0 is a no-op.
 * Blocks of 32 vectors (a tail of at most 16: one block of 16) in the workspace layout of solve_many; a
 * product is out of place between that workspace and a second one and has no dependency chain: per direction
 * one launch over all (block column, strip) tiles of "solve_tiles", which STORE their products at the slots
 * of the "rsolve_*" tables above (a slot is one row of 16 or 32 doubles here), and one launch over the chunks
 * of 64 pivot positions of every block column, which multiplies with the diagonal tile -- read from the
 * arena and masked to its lower triangle, never from the inverted panels -- and adds the stored products:
 * for L x those of "rsolve_gsrc"[gptr[p] .. gptr[p+1]) in that order, one after the other; for L^T x the
 * strips of the block column in ascending order.  Two launches per direction, four for job 0, plus pack and
 * unpack; every product on v_mfma_f64_16x16x4_f64.
 * Reproducibility: no atomic add anywhere.  The same factor bits and vector bits give the same result bits
 * across calls, group sizes, positions within a group, and the host / device / pivot-order entry points.
 * Memory: on first use the tables (shared with the reproducible solve when they are resident), a second
 * workspace of 32 n doubles and a scratch of 32 * max(rsolve_frows, rsolve_bsize) doubles are taken from the
 * device pool and kept until spllt_hip_release_factor_mult or spllt_deallocate_fkeep.  When that does not
 * fit, both are taken for 16 vectors and every block is a block of 16: per vector the bits are the same.
 * The work is ordered on the engine's stream and has finished when the call returns; a later spllt_factor or
 * spllt_hip_updown on the handle is picked up.
 * Errors: null pointer, nvec < 0, ldx < n, bad job, nothing factorized yet -> SPLLT_ERROR_PARAMETER;
 * partitioned handle -> SPLLT_ERROR_UNIMPLEMENTED; no device memory for blocks of 16 either ->
 * SPLLT_ERROR_ALLOCATION (nothing is kept half-allocated, the factor and every solve stay usable).
 * Debug: spllt_hip_debug("fmult_poison=1") fills the scratch with NaN before every direction ("=0": off);
 * "fmult_alloc_fail=N" makes the next N allocations of the second workspace and the scratch fail;
 * "alloc_fail_at=K" makes the K-th allocation of any optional feature's device memory from now on fail once
 * (0: off; "alloc_fail_armed" returns 1 while it still waits).  spllt_hip_program_get "owned" returns two
 * int64: the device buffers the handle's engine holds and their bytes. */
int spllt_hip_factor_mult(void *fkeep, int nvec, double *x_host, int64_t ldx, int job);      /* host, user order */
int spllt_hip_factor_mult_dev(void *fkeep, int nvec, double *x_dev, int64_t ldx, int job,
                              int pivot_order);   /* device; 0 = user order, 1 = pivot order */
int spllt_hip_release_factor_mult(void *fkeep);   /* workspace, scratch and tables back to the pool */
/* ---- Gaussian sampling (single GPU) -----------------------------------------------
 * Noise: entry (pivot position p, sample s) is ONE Philox4x32-10 block with counter (p, 0, s lo, s hi) and
 * key (seed lo, seed hi), s = first_sample + q.  Words 0 (low) and 1 (high) give u1 = ((w >> 11) + 1) 2^-53
 * in (0, 1], words 2 and 3 give u2 = (w >> 11) 2^-53 in [0, 1); z = sqrt(-2 ln u1) cos(2 pi u2) in fp64.
 * Only this one value of a block is used: an entry depends on (seed, p, s) alone -- not on nsamp, the group
 * it falls into or the entry point.  spllt_hip_white_noise_dev writes z in PIVOT order, z[q*ldz + p].
 * spllt_hip_sample*: sample q at x[q*ldx .. q*ldx + n), user order.
 *   kind 1 (A is a covariance):  x = mean + P^T L z, through the product above: repeats bit for bit.
 *   kind 0 (A is a precision):   x = mean + P^T L^-T z, the backward sweep.  With
 *          spllt_hip_set_reproducible_solve on for the handle it goes through spllt_hip_solve_repro and
 *          repeats bit for bit; otherwise through spllt_hip_solve_many, which is faster and repeats to
 *          rounding only.
 * mean: null, or n doubles in user order (device memory for _dev), added on the device.
 * Errors as for the products, and a kind other than 0 or 1 -> SPLLT_ERROR_PARAMETER. */
int spllt_hip_sample_dev(void *fkeep, int nsamp, double *x_dev, int64_t ldx, int kind,
                         uint64_t seed, uint64_t first_sample, const double *mean_dev);
int spllt_hip_sample(void *fkeep, int nsamp, double *x_host, int64_t ldx, int kind,
                     uint64_t seed, uint64_t first_sample, const double *mean_host);
int spllt_hip_white_noise_dev(void *fkeep, int nsamp, double *z_dev, int64_t ldz,
                              uint64_t seed, uint64_t first_sample);
int spllt_hip_set_exchange_buffer(void *fkeep, void *dev_ptr);
/* The HIP stream (hipStream_t) every caller-visible operation of this handle is ordered on:
 * spllt_factor ends by packing the exchange buffer on it and spllt_hip_continue starts by
 * unpacking it there.  A caller that enqueues its collective ON this stream (RCCL takes a
 * stream argument; torch: torch.cuda.ExternalStream) needs no host synchronisation between
 * the phases of a partitioned factorization.  Creates the device engine if necessary;
 * NULL without a HIP device. */
void *spllt_hip_engine_stream(void *fkeep);
/* The stream the PENDING exchange (spllt_hip_pending_exchange) is packed and unpacked on: the
 * stream of spllt_hip_engine_stream, except for the per-level reduce-scatters of a distributed
 * top tree, which the multi-stream program issues on a side stream so that the chunks of the
 * upper top-tree levels travel while the lowest one is already being factorized (SURVEY 8(e):
 * "pipeline per ancestor node").  The caller's collective for that exchange goes on THIS stream. */
void *spllt_hip_exchange_stream(void *fkeep);
int spllt_hip_continue(void *fkeep);
/* "arena_elems" (int64 x 2: doubles of the factor arena held on this rank's device once its engine
 * exists - a rank stores only its own branches and the top tree, packed -, doubles of the whole arena),
 * "owner" (int32 per node: rank or -1 = top tree), "top_bcols" (int32),
 * "top_bcol_owner" (int32 per block column: owner in a distributed top tree, -1 outside it;
 * empty when the top tree is replicated),
 * "map_keep" (uint8 per val->L map entry: scattered on this rank) */
int64_t spllt_hip_partition_get(void *fkeep, const char *name, void *buf, int64_t capacity_bytes);

/* spllt_factor with val already resident in HBM (device pointer).  val_dev must stay valid and
 * unchanged until spllt_hip_wait returns: the factorization reads it in place. */
void spllt_hip_factor_dev(void *akeep, void *fkeep, spllt_options_t *options, int nnz,
                          const double *val_dev, spllt_inform_t *info);
/* wait for ONE factorization and return its flag (spllt_wait() has no way to) */
int spllt_hip_wait(void *fkeep);
/* copy the whole L arena (block columns concatenated in order) to host memory */
int spllt_hip_get_factor(void *fkeep, double *out, int64_t count);
/* device pointer of the L arena (valid until spllt_deallocate_fkeep) */
/* (partitioned factorization: the rank's packed arena, not the global layout) */
double *spllt_hip_device_factor(void *fkeep);
/* ---- selected inversion (single GPU) -----------------------------------------
 * Z = (P A P^T)^-1 on the pattern of L (P: the pivot order, "order" of spllt_hip_sym_get), computed
 * on the device from the current factor by the Takahashi recurrences, panel by panel from the root
 * down.  The Z arena has exactly L's layout (spllt_hip_get_factor): every position that holds L
 * holds the entry of Z with the same (row, column) in pivot order; the never-read strict upper
 * triangle of the diagonal tiles is unspecified.  Entries of A^-1 outside the pattern of L need
 * solves: spllt_hip_solve_sparse with unit columns and the wanted rows.  A later factorization
 * makes Z stale: the readers then return SPLLT_ERROR_PARAMETER until spllt_hip_selected_inverse
 * runs again.  L and the solve stay usable.  No atomics: two runs on the same factor give a
 * bit-identical Z.  A partitioned factor returns SPLLT_ERROR_UNIMPLEMENTED; too little device
 * memory for the Z arena (L's size) returns SPLLT_ERROR_ALLOCATION.  Messages:
 * spllt_hip_last_error. */
int     spllt_hip_selected_inverse(void *fkeep);                       /* compute Z on the device */
int     spllt_hip_get_inverse(void *fkeep, double *out, int64_t count); /* Z arena -> host, L's layout */
double *spllt_hip_device_inverse(void *fkeep);                         /* device pointer of the Z arena */
int     spllt_hip_inverse_diag(void *fkeep, double *out, int n);        /* (A^-1)_ii, user order, host */
/* out[k] = (A^-1) at the k-th entry of the analysed CSC-lower pattern (ptr, row), nnz values in the
 * order of val, host: what tr(A^-1 dA/dtheta) needs.  One gather launch through the value map. */
int     spllt_hip_inverse_on_pattern(void *fkeep, double *out);
int     spllt_hip_log_det(void *fkeep, double *out);                    /* log det A of the last factor */
int     spllt_hip_release_inverse(void *fkeep);                        /* free the Z arena early */
/* ---- batched factorization (single GPU) ---------------------------------------
 * nbatch value arrays on the pattern of ONE akeep / fkeep pair are factorized together,
 * P A_b P^T = L_b L_b^T for b = 0 .. nbatch-1, and solved together.  The members share the symbolic
 * structure and one set of program tables (uploaded on the first batch call of a handle); every kernel
 * launch of the batch program carries all members, so the number of launches does not depend on nbatch
 * (spllt_hip_batch_launches).  Each member has its own factor arena (the layout of
 * spllt_hip_get_factor), its own not-positive-definite flag and its own log-determinant: one bad
 * member does not spoil the others.  The batch program is the single-stream, unfused program of the
 * pattern with 64-wide panels, whatever spllt_hip_set_engine chose for the handle's single
 * factorization; it is meant for the small, launch-latency-bound end.
 *
 * Storage for nbatch members (arena + inverted panels each) is taken on the first call, grows when a
 * later call brings a larger nbatch, and stays with the handle until spllt_hip_release_batch or
 * spllt_deallocate_fkeep.  If the device cannot hold it the call returns SPLLT_ERROR_ALLOCATION, keeps
 * nothing half-allocated, and the handle's single factorization stays usable.
 *
 * The batch and the handle's single factor are independent: spllt_hip_get_factor, spllt_solve,
 * spllt_hip_solve_many and a valid selected inverse stay valid across spllt_hip_factor_batch, and the
 * batch survives spllt_factor.  All work is ordered on spllt_hip_engine_stream and finished when a
 * call returns.  Reproducibility is the default engine's: inter-node updates and the solve's strips add
 * with fp64 atomics, two runs agree to rounding, not bit for bit.
 *
 * Only the allocation failure is promised to leave the single factorization usable: a HIP runtime error
 * inside a batch call (SPLLT_ERROR_HIP) marks the handle's engine as failed, single factorization included.
 *
 * Errors: null pointer, negative count, nnz not the pattern's, ldval < nnz, ldx < n, bad job, bad
 * member, a solve or reader before any batch -> SPLLT_ERROR_PARAMETER; a handle after
 * spllt_hip_set_partition with nranks > 1 -> SPLLT_ERROR_UNIMPLEMENTED; no device -> SPLLT_ERROR_HIP; a
 * batch program that holds something the batch kernels do not implement -> SPLLT_ERROR_UNKNOWN.
 * Messages: spllt_hip_last_error.  nbatch = 0 and nrhs = 0 are no-ops that return 0. */
/* values of member b at val[b*ldval .. b*ldval + nnz), ldval >= nnz.  0: every member factorized.
 * SPLLT_ERROR_NOT_POSDEF: at least one member is not positive definite; the OTHER members are
 * factorized and usable, spllt_hip_batch_status says which. */
int spllt_hip_factor_batch(void *akeep, void *fkeep, int nbatch, int nnz, const double *val_host, int64_t ldval);
int spllt_hip_factor_batch_dev(void *akeep, void *fkeep, int nbatch, int nnz, const double *val_dev, int64_t ldval);
/* flag[b] = 0 or SPLLT_ERROR_NOT_POSDEF; column[b] = 1-based pivot position of the first non-positive
 * pivot, 0 if none; either pointer may be NULL; at most `capacity` entries are written.  Returns the
 * nbatch of the last batch (0: none yet). */
int spllt_hip_batch_status(void *fkeep, int *flag, int *column, int capacity);
/* nrhs vectors PER MEMBER: vector q of member b at x[(b*nrhs + q)*ldx .. + n), ldx >= n, overwritten;
 * nothing else is read or written.  Vectors of a failed member are left unchanged; the return value is
 * SPLLT_ERROR_NOT_POSDEF then and the other members are solved.  job 0 / 1 / 2 as spllt_solve.
 * pivot_order as spllt_hip_solve_many_dev.  There is no nbatch argument: the call works on ALL members of
 * the last batch (spllt_hip_batch_status returns their number), so x must hold nbatch * nrhs vectors. */
int spllt_hip_solve_batch(void *fkeep, int nrhs, double *x_host, int64_t ldx, int job);
int spllt_hip_solve_batch_dev(void *fkeep, int nrhs, double *x_dev, int64_t ldx, int job, int pivot_order);
/* one member's arena -> host, the layout of spllt_hip_get_factor */
int spllt_hip_get_factor_batch(void *fkeep, int member, double *out, int64_t count);
/* device pointer of member 0's arena; member b starts *member_stride doubles further (NULL / 0: no batch) */
double *spllt_hip_device_factor_batch(void *fkeep, int64_t *member_stride);
/* out[b] = log det A_b, nbatch values; NaN for a failed member */
int spllt_hip_log_det_batch(void *fkeep, double *out);
/* kernel launches of the last batched factorization (initialisation included) */
int spllt_hip_batch_launches(void *fkeep);
/* give the batch's storage back; the next spllt_hip_factor_batch takes it again */
int spllt_hip_release_batch(void *fkeep);
/* ---- batched selected inversion (single GPU) -------------------------------------
 * Z_b = (P A_b P^T)^-1 on the pattern of L for every member of the last batch, from the members' factors
 * and inverted panels, by ONE selected-inversion program of the pattern (64-wide panels: those of the
 * batch factorization, whatever the handle's panel width) whose every kernel launch carries all members.
 * A step of the program whose panels all have at most 64 rows below them runs as one fused launch instead
 * of three; the number of launches does not depend on nbatch
 * (spllt_hip_batch_selinv_launches).  Member b's Z arena has the layout of spllt_hip_get_inverse.  No
 * atomics: two inversions of one batch give a bit-identical Z for every member.
 *
 * The Z arenas (nbatch x the arena) and a step scratch are taken on the first call, grow with nbatch and
 * stay until spllt_hip_release_inverse_batch, spllt_hip_release_batch or spllt_deallocate_fkeep.  Too
 * little device memory -> SPLLT_ERROR_ALLOCATION, nothing is kept half-allocated, and the batch factor,
 * spllt_hip_solve_batch and the single factorization stay usable.  All work is ordered on
 * spllt_hip_engine_stream and finished when a call returns.
 *
 * spllt_hip_factor_batch (and _dev) makes the batch's Z stale: the readers then return
 * SPLLT_ERROR_PARAMETER until spllt_hip_selected_inverse_batch runs again.  spllt_factor and
 * spllt_hip_selected_inverse neither touch the batch's Z nor are touched by this call.
 *
 * A member that is not positive definite is skipped (nothing of it is read or written): the inversion
 * returns SPLLT_ERROR_NOT_POSDEF and the other members are inverted; its rows of the two readers are NaN.
 *
 * Errors: null pointer, bad member, ldout too small, no batch yet, stale Z -> SPLLT_ERROR_PARAMETER; a
 * partitioned handle -> SPLLT_ERROR_UNIMPLEMENTED; no device -> SPLLT_ERROR_HIP.  Messages:
 * spllt_hip_last_error.  An empty batch is a no-op that returns 0. */
int     spllt_hip_selected_inverse_batch(void *fkeep);
/* one member's Z arena -> host, L's layout; a failed member: SPLLT_ERROR_NOT_POSDEF */
int     spllt_hip_get_inverse_batch(void *fkeep, int member, double *out, int64_t count);
/* device pointer of member 0's Z arena; member b starts *member_stride doubles further (NULL / 0: no valid Z) */
double *spllt_hip_device_inverse_batch(void *fkeep, int64_t *member_stride);
/* out[b*ldout + i] = (A_b^-1)_ii in the user's variable order, ldout >= n, host, one launch */
int     spllt_hip_inverse_diag_batch(void *fkeep, double *out, int64_t ldout);
/* out[b*ldout + k] = (A_b^-1) at the k-th entry of (ptr, row), the order of val, ldout >= nnz, host */
int     spllt_hip_inverse_on_pattern_batch(void *fkeep, double *out, int64_t ldout);
/* kernel launches of the last batched inversion */
int     spllt_hip_batch_selinv_launches(void *fkeep);
/* give the Z arenas and the scratch back; the batch factor and its solve stay */
int     spllt_hip_release_inverse_batch(void *fkeep);
/* ---- refined solves (single GPU) ---------------------------------------------------
 * The operator A on the analysed pattern lives on the device as a full (both triangles) CSR of P A P^T
 * in pivot order, built on first use from the pattern alone: "matvec_rowptr" (int64), "matvec_col"
 * (int32 pivot positions, sorted inside a row) and "matvec_src" (int32 indices into val) of
 * spllt_hip_program_get.  y_p = sum_k val[src[k]] * x[col[k]] is a gather with a fixed summation order:
 * no atomics, two products of the same inputs are bit-identical.
 *
 * spllt_hip_matvec: y = A x; val: nnz values in the order of spllt_factor (need not be the factored ones);
 * nvec vectors, user order, x[q*ldx + i], y[q*ldy + i]; only those ranges are read or written.  The _dev
 * twin takes device pointers; pivot_order = 1: x and y are in pivot order as for spllt_hip_solve_dev (x and
 * y must not overlap).  The product needs no factor.
 *
 * spllt_hip_solve_refined: solve A x = b with A = (pattern, val) and the CURRENT factor as M, to the
 * backward error e = ||b - A x||_2 / (||b||_2 + max|a_ij| ||x||_2) <= tol.  x holds b on entry, the solution
 * on exit.  method 0: iterative refinement x += M^-1 (b - A x); method 1: conjugate gradients preconditioned
 * by M, every vector with its own scalars; a vector that the recurrence residual declares converged is
 * confirmed with a true residual and goes on from it if the confirmation fails.  tol > 0; max_iter >= 0;
 * iterations (int) and error (double) receive nrhs values each, either may be NULL: iterations[q] = the
 * applications of M^-1 after the first (0: M^-1 b passed), error[q] = e of a true residual.  Returns 0 when
 * every vector reached tol and 1 when at least one did not: x then holds, per vector, the iterate with the
 * smallest confirmed error (never worse than M^-1 b), and error[] says which.  A NaN in val or b ends that
 * vector as not converged.  Vectors are worked on in groups of 32 (five work vectors and the best iterate
 * per member of a group, taken from the device pool on first use together with the operator; kept until
 * spllt_hip_release_refine or spllt_deallocate_fkeep).  M^-1 is spllt_hip_solve_dev for up to 4 vectors and
 * spllt_hip_solve_many_dev above; a later factorization on the handle is picked up.  All work is ordered on
 * spllt_hip_engine_stream and finished when a call returns; per iteration one array of 64 doubles is read
 * back.  Reproducibility: products and reductions are bit-reproducible, the solution inherits the fp64
 * atomics of the solves and agrees to rounding only -- unless spllt_hip_set_reproducible_solve is on: M^-1 is
 * then spllt_hip_solve_repro_dev for every group size and two calls return the same bits and iteration counts.
 * Errors: null pointer, negative count, nnz not the pattern's, ldx / ldy < n, bad method, tol <= 0, nothing
 * factorized yet (refined solve only) -> SPLLT_ERROR_PARAMETER; partitioned handle ->
 * SPLLT_ERROR_UNIMPLEMENTED; no device -> SPLLT_ERROR_HIP; no device memory -> SPLLT_ERROR_ALLOCATION
 * (nothing is kept half-allocated, the factor and every other solve stay usable).  nvec = 0 and nrhs = 0
 * are no-ops that return 0.  Messages: spllt_hip_last_error. */
int spllt_hip_matvec    (void *fkeep, int nnz, const double *val_host, int nvec, const double *x_host, int64_t ldx, double *y_host, int64_t ldy);
int spllt_hip_matvec_dev(void *fkeep, int nnz, const double *val_dev,  int nvec, const double *x_dev,  int64_t ldx, double *y_dev,  int64_t ldy, int pivot_order);
int spllt_hip_solve_refined    (void *fkeep, int nnz, const double *val_host, int nrhs, double *x_host, int64_t ldx, int method, double tol, int max_iter, int *iterations, double *error);
int spllt_hip_solve_refined_dev(void *fkeep, int nnz, const double *val_dev,  int nrhs, double *x_dev,  int64_t ldx, int method, double tol, int max_iter, int *iterations, double *error);
int spllt_hip_release_refine(void *fkeep);   /* operator tables and work vectors back to the pool */
/* ---- low-rank update / downdate of the factor (single GPU) ------------------------------
 * spllt_hip_updown: with L the current factor of P A P^T, the arena afterwards holds the factor of
 * P (A + sign W W^T) P^T, in place and in the same layout (spllt_hip_get_factor), and the inverses of the
 * new diagonal panels are in place: spllt_solve, spllt_hip_solve_dev, spllt_hip_solve_many* and
 * spllt_hip_solve_refined* work on the modified factor, spllt_hip_log_det reflects it.  W: k sparse columns,
 * CSC, 1-based, in the user's variable order (as ptr / row of spllt_analyse), rows strictly increasing
 * inside a column; sign +1 (update) or -1 (downdate).  Several columns equal that many successive rank-1
 * modifications in the order of the columns.
 * Admissible columns: the pattern of L never changes.  With j the smallest pivot position of a column's
 * pattern, every pivot position of the pattern must be a row of the supernode that holds j ("rlist" of
 * spllt_hip_sym_get).  Sufficient, and what a user can reason about: the pattern is a clique of the
 * analysed matrix -- an element contribution, alpha (e_i - e_j) on an existing entry (i, j), alpha e_i.
 * Anything else returns SPLLT_ERROR_PARAMETER and leaves the factor bit for bit untouched: every check
 * happens on the host before anything is enqueued.
 * Work: only the block columns on the elimination-tree paths from the first pivot of each column to the
 * root are read and written, once per pass of 8 columns (spllt_hip_updown_plan lists them).  No atomics:
 * the same calls on two handles whose factors are bit-identical give bit-identical factors.  All work is
 * ordered on spllt_hip_engine_stream and finished when the call returns; a pending factorization is waited
 * for.  A work array of 8 n doubles and a small scratch stay with the handle.
 * Cost (MI355X): the sweep is bound by the chain of dependent operations along the path, not
 * by bytes.  Measured: 80 ms for one column and 166 ms for eight against a 507 ms factorization (n = 2.1 M), but
 * 21 ms and 52 ms against a 23 ms factorization on a matrix (n = 72 k) whose top separators hold 30 % of the
 * factor: where a factorization takes tens of milliseconds, re-factorize instead.
 * State afterwards: a success marks the selected inverse stale (its readers return SPLLT_ERROR_PARAMETER
 * until spllt_hip_selected_inverse runs again); the batch of spllt_hip_factor_batch is independent and
 * untouched; a later spllt_factor behaves as before.  A DOWNDATE THAT MEETS A NON-POSITIVE PIVOT returns
 * SPLLT_ERROR_NOT_POSDEF and leaves the factor INVALID: the solves and readers of the single factor then
 * return SPLLT_ERROR_PARAMETER ("nothing factorized") until the next spllt_factor, which revives the handle.
 * Errors: null pointer, k < 0, a row index outside [1, n], unsorted or duplicate rows in a column, a sign
 * other than +1 / -1, a value of W that is not finite, a column that is not admissible, nothing factorized -> SPLLT_ERROR_PARAMETER;
 * partitioned handle -> SPLLT_ERROR_UNIMPLEMENTED; no device -> SPLLT_ERROR_HIP; no device memory for the
 * work array, the scratch or the staged entries -> SPLLT_ERROR_ALLOCATION (nothing is kept half-allocated,
 * the factor stays usable).  k = 0 and empty columns are no-ops that return 0.  Messages:
 * spllt_hip_last_error. */
int spllt_hip_updown(void *fkeep, int k, const int *wptr, const int *wrow, const double *wval, int sign);
/* host only, needs no device: the block columns the call would visit, ascending (ids as in "bcol_*" of
 * spllt_hip_sym_get); returns their number, or SPLLT_ERROR_PARAMETER when the arrays are malformed or a
 * column is not admissible (bcols may be NULL to query) */
int64_t spllt_hip_updown_plan(void *fkeep, int k, const int *wptr, const int *wrow, int32_t *bcols, int64_t capacity);
/* of the last spllt_hip_updown: block columns visited, entries of L in them, kernel launches, passes */
int spllt_hip_updown_info(void *fkeep, int64_t out[4]);
/* device time of the last spllt_hip_updown, ms: first scatter to last kernel, between two HIP events on the
 * engine stream (without the host's plan and the staging of W) */
int spllt_hip_updown_time(void *fkeep, double *device_ms);
/* ---- sparse right-hand sides and selected outputs (single GPU) -------------------------------
 * spllt_hip_solve_sparse*: X = A^-1 B (job 0), L^-1 P B (job 1) or L^-T of the scattered B (job 2) for k SPARSE
 * columns B, at SELECTED entries.  The forward sweep visits only the block columns on the elimination-tree paths
 * from the nonzeros of B to the root, the backward sweep only those on the paths from the wanted entries to the
 * root (spllt_hip_solve_sparse_plan lists both sets); skipping a block column whose part of the vector is exactly
 * zero removes additions of zero only, so the result is that of the full solve up to the order of the atomic
 * adds.  This is the route to entries of A^-1 outside the pattern of L (unit columns, one wanted entry each), to
 * a few entries of x for a b with a few nonzeros, and, with spllt_hip_gram_sparse, to B^T A^-1 B.
 * B: CSC, 1-based, in the user's variable order, exactly like W of spllt_hip_updown: rows strictly increasing
 * inside a column, empty columns allowed.  Any pattern is legal; the values are not inspected (a NaN propagates
 * through its column).  sel: nsel 1-based user variables in any order, duplicates allowed; sel == NULL or
 * nsel < 0: all n entries.
 * Output: x[q * ldx + t] = the solution of column q at variable sel[t], ldx >= nsel (all entries wanted:
 * x[q * ldx + i] at variable i, ldx >= n); nothing else is written.  Under job 1 and job 2 a wanted variable
 * means what it means to spllt_solve: the vector comes back in user order through the pivot permutation.  A
 * wanted entry that no sweep reaches is an exact 0.0; an empty column gives an exact zero column under jobs 0
 * and 1.
 * Columns are worked on in consecutive groups of 32 (a tail of at most 16: one block of 16, as in
 * spllt_hip_solve_many), each group with its own plan and the blocked fp64-MFMA kernels of solve_many on the
 * shared workspace of 32 n doubles.  Reproducibility, ordering and pickup are those of spllt_hip_solve_many:
 * the strips add with atomics (reproducible to rounding), spllt_hip_set_reproducible_solve has no effect here,
 * all work is ordered on spllt_hip_engine_stream and finished on return, a later factorization or
 * spllt_hip_updown is picked up.  The staged lists of a group and (host entry points) the gathered block stay
 * with the handle and grow on demand; spllt_hip_release_solve_sparse returns them.
 * spllt_hip_gram_sparse: G = B^T A^-1 B = Y^T Y with Y = L^-1 P B, by forward sweeps only; k x k, column-major,
 * both triangles (exactly symmetric), ldg >= k.  One workspace of 32 n doubles per group of columns stays alive
 * until the products are done.
 * Cost (MI355X): the sweeps are bound by dependent launches, one surviving block column
 * per level of a path -- see there for what the restriction gains and where it does not.
 * Errors, all decided on the host before anything is enqueued, x untouched: null fkeep, bptr, x or g; brow or
 * bval null with a non-empty B; k < 0; bptr[0] < 1 or decreasing pointers; a row or sel index outside [1, n];
 * rows not strictly increasing; ldx or ldg too small; a job other than 0, 1, 2; nothing factorized ->
 * SPLLT_ERROR_PARAMETER; partitioned handle -> SPLLT_ERROR_UNIMPLEMENTED; no device -> SPLLT_ERROR_HIP; no
 * device memory -> SPLLT_ERROR_ALLOCATION (nothing of this feature stays allocated; the factor and every other
 * solve stay usable).  A pending factorization is waited for.  k = 0 and nsel = 0 return 0 and do nothing.
 * Messages: spllt_hip_last_error. */
int spllt_hip_solve_sparse    (void *fkeep, int k, const int *bptr, const int *brow, const double *bval,
                               int nsel, const int *sel, double *x_host, int64_t ldx, int job);
int spllt_hip_solve_sparse_dev(void *fkeep, int k, const int *bptr, const int *brow, const double *bval,
                               int nsel, const int *sel, double *x_dev,  int64_t ldx, int job);
int spllt_hip_gram_sparse     (void *fkeep, int k, const int *bptr, const int *brow, const double *bval,
                               double *g_host, int64_t ldg);
/* host only, needs no device and no factor: the block columns the two sweeps would visit for these columns
 * taken as ONE group, ascending (ids as in "bcol_*" of spllt_hip_sym_get).  The forward set is empty under job 2,
 * the backward set under job 1.  counts[0 .. 1] receive the two sizes; either array may be NULL to query.
 * Returns 0 or SPLLT_ERROR_PARAMETER. */
int spllt_hip_solve_sparse_plan(void *fkeep, int k, const int *bptr, const int *brow, int nsel, const int *sel,
                                int job, int32_t *fwd_bcols, int64_t fwd_cap, int32_t *bwd_bcols, int64_t bwd_cap,
                                int64_t counts[2]);
/* of the last sparse solve or gram, summed over its groups and counted from the lists that were uploaded: block
 * columns of the forward sweep, of the backward sweep, doubles of L (sum of nrow * width) in the forward set, in
 * the backward set, kernel launches, workgroups launched by the sweeps */
int spllt_hip_solve_sparse_info(void *fkeep, int64_t out[6]);
int spllt_hip_release_solve_sparse(void *fkeep);   /* staged lists, gathered block, gram workspaces back to the pool */
/* timings of the last factorization, milliseconds */
int spllt_hip_factor_times(void *fkeep, double *submit_ms, double *device_ms, double *h2d_ms,
                           int *launches);
/* ---- sampled outer product on the pattern, device-side readers (single GPU) -----------------
 * What the adjoints of x = A^-1 b and of log det A with respect to the stored values need on the device
 * (the torch front end is spllt_amd/torch_ops.py).  The k-th stored value val[k]
 * stands for BOTH a_ij and a_ji (i >= j, the k-th entry of the analysed CSC-lower pattern in user
 * variables), so
 *
 *     out[k] = alpha * sum_q ( u_q[i] v_q[j] + [i != j] u_q[j] v_q[i] ),   q = 0 .. nvec-1
 *
 * with u = the adjoint solution A^-1 xbar, v = x and alpha = -1 is d loss / d val[k].  Vector q is at
 * u[q*ldu .. q*ldu + n) and v[q*ldv .. q*ldv + n) in the user's variable order (the layout of
 * spllt_hip_solve_many_dev), ldu, ldv >= n; nothing outside those ranges is read and exactly nnz doubles
 * are written.  One gather kernel (spllt_amd/csrc/pattern_outer.hip): no atomics; per entry the sum over
 * q is ONE chain of fma in ascending q (first u_i v_j, then u_j v_i), alpha is applied once at the end, so
 * the same input bits give the same output bits whatever the launch shape.  Needs the analysis only, no
 * factor.  The (row, column) tables are built on first use from the analysed pattern, int32, 0-based user
 * variables, exported as "pattern_row" / "pattern_col" by spllt_hip_program_get and released with the handle.
 * nvec = 0 writes alpha * 0 to every entry.
 *
 * Errors, all decided on the host before the device is touched: a null pointer, nvec < 0, nbatch < 0,
 * ldu < n, ldv < n, ldout < nnz -> SPLLT_ERROR_PARAMETER; a partitioned handle ->
 * SPLLT_ERROR_UNIMPLEMENTED; no device -> SPLLT_ERROR_HIP.  Messages: spllt_hip_last_error.  All work is
 * ordered on spllt_hip_engine_stream and finished when a call returns. */
int spllt_hip_pattern_outer(void *fkeep, int nvec, const double *u_host, int64_t ldu, const double *v_host,
                            int64_t ldv, double alpha, double *out_host);
int spllt_hip_pattern_outer_dev(void *fkeep, int nvec, const double *u_dev, int64_t ldu, const double *v_dev,
                                int64_t ldv, double alpha, double *out_dev);
/* nbatch members in one launch: vector q of member b at u[(b*nvec + q)*ldu ..] (the layout of
 * spllt_hip_solve_batch_dev), out[b*ldout + k], ldout >= nnz.  Member b's row equals the single call on
 * its vectors bit for bit.  Needs no batch factor. */
int spllt_hip_pattern_outer_batch_dev(void *fkeep, int nbatch, int nvec, const double *u_dev, int64_t ldu,
                                      const double *v_dev, int64_t ldv, double alpha, double *out_dev,
                                      int64_t ldout);
/* spllt_hip_inverse_on_pattern / _batch with the output in device memory (nnz doubles / nbatch rows of
 * ldout >= nnz doubles): the same gather launch, the same bits, no copy to the host.  The rows of a failed
 * member are NaN. */
int spllt_hip_inverse_on_pattern_dev(void *fkeep, double *out_dev);
int spllt_hip_inverse_on_pattern_batch_dev(void *fkeep, double *out_dev, int64_t ldout);
/* ---- reverse-mode derivative of the factor -----------------------------------------
 * G is a further arena with the layout of spllt_hip_get_factor.  Seeded, it holds Lbar = d loss / d L on the
 * lower positions of L in pivot order (the strict upper triangle of a diagonal tile is never read).
 * spllt_hip_factor_adjoint sweeps it in place -- the panels of the selected inversion in the same order, three
 * launches per step, no atomics, every sum in a fixed order: the same bits for the same L and Lbar -- into
 * d loss / d (P A P^T)_ij on every stored lower position, a stored lower entry standing for a_ij AND a_ji, and
 * returns the values at the entries of A: gval[k] = d loss / d val[k], nnz doubles in the order of val.
 *
 * _seed: G (+)= alpha sum_q a_q[r] b_q[c] at every lower position (r, c); vector q at a + q * ld, ld >= n.
 * order_flags bit 0: a is in pivot order, bit 1: b is (spllt_hip_white_noise_dev writes pivot order); else a
 * vector is in the user's variable order.  accumulate = 0 overwrites (nvec = 0: zeroes the arena), 1 adds to
 * a seeded arena.  Per entry the sum is one fma chain over q ascending, alpha applied once: a vector's
 * contribution does not depend on nvec or on its place among the others.  The seeds of the uses, all
 * vectors in pivot order, ybar the incoming gradient:  y = L x: + ybar x^T;  y = L^T x: + x ybar^T;
 * y = L^-1 x: - (L^-T ybar) y^T;  y = L^-T x: - y (L^-1 ybar)^T.  The map Lbar -> gval is linear: any number
 * of vectors shares one sweep.
 * _set / _get: the whole arena from / to the host (an arbitrary Lbar; after the sweep the result).
 * spllt_hip_device_factor_adjoint: the arena on the device, null while it is unseeded.
 *
 * States: unseeded (also after spllt_factor, spllt_hip_factor_dev, spllt_hip_updown: stale), seeded, swept.
 * The arena is taken on first use and kept until spllt_hip_release_factor_adjoint or the handle is freed; the
 * program tables and the step scratch are shared with spllt_hip_selected_inverse, whose Z arena is untouched.
 *
 * Errors, decided before anything is enqueued: a null pointer, nvec < 0, ld < n, count < the arena, nothing
 * factorized, accumulate = 1 on an arena that is not seeded, a sweep of an arena that is not freshly seeded
 * (a second sweep included), _get on an unseeded arena -> SPLLT_ERROR_PARAMETER; a partitioned handle ->
 * SPLLT_ERROR_UNIMPLEMENTED; no memory for G -> SPLLT_ERROR_ALLOCATION (nothing is kept half-allocated, the
 * factor and the solves stay usable); a symbolic structure the selected-inversion program cannot be built
 * for -> the flag of spllt_hip_selected_inverse.  All work is ordered on spllt_hip_engine_stream and finished
 * when a call returns. */
int spllt_hip_factor_adjoint_seed_dev(void *fkeep, int nvec, const double *a_dev, const double *b_dev, int64_t ld,
                                      double alpha, int accumulate, int order_flags);
int spllt_hip_factor_adjoint_seed(void *fkeep, int nvec, const double *a_host, const double *b_host, int64_t ld,
                                  double alpha, int accumulate, int order_flags);
int spllt_hip_set_factor_adjoint(void *fkeep, const double *host_arena, int64_t count);
int spllt_hip_get_factor_adjoint(void *fkeep, double *out, int64_t count);
double *spllt_hip_device_factor_adjoint(void *fkeep);
int spllt_hip_factor_adjoint_dev(void *fkeep, double *gval_dev);
int spllt_hip_factor_adjoint(void *fkeep, double *gval_host);
int spllt_hip_release_factor_adjoint(void *fkeep);
/* a counter that every successful change of the factor increments: which = 0 the single factor
 * (spllt_factor, spllt_hip_factor_dev, spllt_hip_updown, the profiling entry points), which = 1 the batch
 * (spllt_hip_factor_batch*).  0 on a fresh handle; needs no device.  A caller that saved state computed
 * from a factor compares the counter to know whether that factor is still the current one. */
int64_t spllt_hip_factor_serial(const void *fkeep, int which);
/* program export for tests: "launches" (int64 x 12 per launch: kind, level,
 * first, count, tile, flops, stream, record, wait0..wait3), "chains" (ChainUnit bytes),
 * "potrf" (PotrfUnit bytes), "units" (UpdUnit bytes), "tiles" (UpdTile bytes),
 * "relpos" (int32), "dinv_size" (int64), "chain_block" (int64), "gather_tiles" / "gather_items"
 * (GatherTile / GatherItem bytes), "scratch_size" (int64); the substitution program:
 * "solve_units" (SolveUnit bytes), "solve_list" (int32), "solve_tiles" (UpdTile bytes),
 * "solve_fwd" / "solve_bwd" (int64 x 4 per launch: kind, level, first, count), "solve_split"
 * (int64 x 2: launches of fwd that belong to the own branches, launches of bwd that belong
 * to the top tree); the selected-inversion program: "selinv_units" (SelinvUnit bytes),
 * "selinv_tiles" (UpdTile bytes: unit, row tile, K slice), "selinv_launches" (int64 x 5 per
 * launch: kind, level, first, count, flops), "selinv_rows" (SelinvRow bytes), "selinv_relpos"
 * (int32), "selinv_diag" (int64 per pivot position: arena offset of its diagonal entry),
 * "selinv_scratch" (int64), "selinv_flops" (double); the program of the batched factorization (the
 * same for every engine flag): "batch_launches", "batch_units", "batch_tiles", "batch_chains",
 * "batch_relpos", "batch_dinv_size" with the layouts of their unprefixed counterparts (and
 * "batch_potrf", empty, "batch_scratch_size", 0); the selected-inversion program of the batch (panels of
 * 64 columns, independent of the handle's panel width): "batch_selinv_units", "batch_selinv_tiles",
 * "batch_selinv_launches", "batch_selinv_rows", "batch_selinv_relpos", "batch_selinv_diag",
 * "batch_selinv_scratch", "batch_selinv_flops", the layouts of the "selinv_*" names; the operator of the
 * refined solves: "matvec_rowptr" (int64), "matvec_col", "matvec_src" (int32); the index stream of the sampled
 * outer product: "pattern_row", "pattern_col" (int32, one per entry of val); "solve_sparse_host_us" (int64):
 * the host microseconds the last spllt_hip_solve_sparse* / spllt_hip_gram_sparse on THIS handle spent, before its
 * first device call, on the plans of its groups, the filtered launches and the arrays to upload (not the upload).
 * Struct layouts: spllt_amd/csrc/schedule.hpp, mirrored as numpy dtypes in
 * spllt_amd/api.py.  Returns the byte length. */
int64_t spllt_hip_program_get(void *fkeep, const char *name, void *buf, int64_t capacity_bytes);
/* per-launch device time (ms) of one profiled factorization; returns #launches */
int spllt_hip_profile(void *fkeep, const double *val, int nnz, float *ms, int capacity);
/* the same for the real multi-stream program: every launch bracketed by two HIP events on
 * the stream it runs on (behind its dependency waits), i.e. its duration beside whatever the
 * other streams run at that moment */
int spllt_hip_profile_in_program(void *fkeep, const double *val, int nnz, float *ms, int capacity);
/* when every event of the real multi-stream program was reached: t_ms[i] = ms after the value
 * scatter at which the event that launch i records completed (-1: the launch records none),
 * t_ms[#launches] = the end of the program.  Nothing is added to the streams (the program's own
 * records, on timing-enabled events).  Returns #launches + 1. */
int spllt_hip_timeline(void *fkeep, const double *val, int nnz, float *t_ms, int capacity);
const char *spllt_hip_last_error(const void *fkeep);
/* flag of the last operation on this handle (0, or an SPLLT error flag): what spllt_wait(void),
 * which has no way to return it, found when the factorization had run */
int spllt_hip_last_flag(const void *fkeep);
const char *spllt_hip_version(void);

/* test hooks: "wedge" marks the HIP runtime as not having returned from a call (what the wait /
 * submission deadlines do), "wedged" reads the mark (1 / 0), "teardown" runs the library's atexit
 * handler now (it must touch nothing once the mark is set); "batch_grid_limit=N": a launch of the batched
 * factorization or solve whose (work items) x (members) exceeds N workgroups is split by member range
 * (N <= 0: back to the hardware limit, (2^32 - 1) / 256 workgroups); "batch_selinv_fused=0" / "=1": the
 * batched selected inversion runs every step as three launches / fuses the small steps (the default);
 * "solve_sparse_poison=1" / "=0": the whole workspace of a sparse solve is filled with NaN before its touched
 * rows are zeroed, so that a sweep that reads a row outside the plan shows up in the result.
 * -1: unknown request. */
int spllt_hip_debug(const char *what);

#ifdef __cplusplus
}
#endif
#endif
