#!/usr/bin/env python3
"""Times the sparse right-hand-side solve (spllt_hip_solve_sparse / spllt_hip_gram_sparse) against the blocked
full solve on the same columns stored densely.

  solve_sparse_bench.py [configs] [--k 32] [--reps 20] [--warmup 3] [--scale 1.0]

configs: comma-separated matgen.CONFIGS keys (default: the bench workload and Poisson3D-128).  B: k unit columns
at the first pivots of distinct leaves of the elimination tree.  In one process, after the warm-ups, alternating:
  (a) solve_many on B stored densely (the unchanged baseline)
  (b) solve_sparse, all entries wanted      (c) solve_sparse, the k entries A^-1[I, I] wanted
  (d) gram(B)                               (e) B^T solve_many(B) formed on the host
Every call returns after its stream has drained.  Median, minimum and maximum of --reps, the host time the call
spends on its plans, filtered launches and the arrays to upload before its first device call
("solve_sparse_host_us" of spllt_hip_program_get), and the figures of spllt_hip_solve_sparse_info.  Needs a GPU: there is no fall-back."""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spllt_amd import api, matgen  # noqa: E402


def stats(ts):
    return {"median_ms": round(float(np.median(ts)) * 1e3, 3), "min_ms": round(min(ts) * 1e3, 3),
            "max_ms": round(max(ts) * 1e3, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("configs", nargs="?", default="nd24k_like,poisson3d_128")
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0)
    args = ap.parse_args()
    if args.reps < 20:
        sys.exit("--reps must be at least 20")
    import torch
    if not torch.cuda.is_available():
        sys.exit("solve_sparse_bench.py needs a GPU")
    for config in args.configs.split(","):
        A, order, cfg = matgen.build_config(config, args.scale)
        if config == "poisson3d_128":
            order = None              # (the built-in nested dissection for this configuration)
        n, ptr, row, val = api.csc_lower_1based(A)
        f = api.Factorization(n, ptr, row, nb=cfg["nb"], nemin=32, prune_tree=False, order=order)
        f.factor(val).wait()
        sptr, sparent, piv = f.sym("sptr"), f.sym("sparent"), f.sym("order")
        var_of = np.empty(n, dtype=np.int64)
        var_of[piv] = np.arange(n)
        leaves = np.setdiff1d(np.arange(len(sparent)), sparent)
        k = min(args.k, len(leaves))
        I = var_of[sptr[leaves[np.linspace(0, len(leaves) - 1, k).astype(np.int64)]]]
        B = sp.csc_matrix((np.ones(k), (I, np.arange(k))), shape=(n, k))
        Bd = np.asfortranarray(B.toarray())
        info, host_us, t = {}, {}, {w: [] for w in "abcde"}
        check = {}
        for it in range(args.warmup + args.reps):
            for which in "abcde":
                t0 = time.perf_counter()
                if which == "a":
                    out = f.solve_many(Bd)
                elif which == "b":
                    out = f.solve_sparse(B)
                elif which == "c":
                    out = f.solve_sparse(B, rows=I)
                elif which == "d":
                    out = f.gram(B)
                else:
                    out = Bd.T @ f.solve_many(Bd)
                dt = time.perf_counter() - t0
                if it >= args.warmup:
                    t[which].append(dt)
                if it == 0:
                    check[which] = out
                    if which in "bcd":
                        info[which] = f.solve_sparse_info()
                        host_us[which] = f.program("solve_sparse_host_us")
        scale = float(np.abs(check["a"]).max())
        err = {"b_vs_a": float(np.abs(check["b"] - check["a"]).max() / scale),
               "c_vs_a": float(np.abs(check["c"] - check["a"][I]).max() / scale),
               "d_vs_e": float(np.abs(check["d"] - check["e"]).max() / np.abs(check["e"]).max())}
        print(json.dumps({"config": config, "n": n, "k": k, "block_columns": int(f.sym_info()["nbcol"]),
                          "arena_doubles": int(f.sym_info()["arena"]),
                          "a_solve_many_dense": stats(t["a"]), "b_solve_sparse_all": stats(t["b"]),
                          "c_solve_sparse_k_entries": stats(t["c"]), "d_gram": stats(t["d"]),
                          "e_host_gram_from_solve_many": stats(t["e"]), "host_plan_filter_us": host_us,
                          "info": info, "max_rel_diff": err}), flush=True)
        f.close()


if __name__ == "__main__":
    main()
