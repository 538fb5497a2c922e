#!/usr/bin/env python3
"""Measurements of the sparse right-hand-side solves of a batch.

  solve_sparse_batch_bench.py [config ...] [--nbatch 4 16 64] [--reps 20] [--warmup 3] [--scale 1.0]
                                                                (default: poisson2d_128 nd24k_like)

Per configuration and nbatch: the members are (1 + b/8) A, B is 32 unit columns on the first pivots of the deepest
leaves (the set-up of solve_sparse_bench.py), shared by all members.  For each of three calls -- all entries wanted,
the 32 entries at B's own rows, gram -- three paths are timed, alternating in one process, host clocks around the
calls (each returns with the stream drained):
  (a) the batch call: solve_sparse_batch / gram_batch;
  (b) the single handle's solve_sparse / gram once per member, summed (ONE handle with the factor resident: the work
      of a member's sweep does not depend on its values);
  (c) solve_many_batch on B stored densely (host vectors: what a caller without this feature passes), for the 32
      entries with the rows picked on the host, for gram with the product B^T X on the host.
Printed per point: median [min, max] of --reps samples after --warmup, in ms; the largest relative difference
between the paths' numbers; spllt_hip_solve_sparse_batch_info and the host time before the first device call.
Needs a GPU: there is no fall-back."""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spllt_amd import api, matgen  # noqa: E402
from updown_bench import deepest_leaves  # noqa: E402


def stats(x):
    return {"median": round(float(np.median(x)), 4), "min": round(float(min(x)), 4), "max": round(float(max(x)), 4)}


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("configs", nargs="*", default=["poisson2d_128", "nd24k_like"])
    ap.add_argument("--nbatch", type=int, nargs="*", default=[4, 16, 64])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0)
    args = ap.parse_args()
    if args.reps < 5:
        sys.exit("--reps must be at least 5")
    import torch
    if not torch.cuda.is_available():
        sys.exit("solve_sparse_batch_bench.py needs a GPU")
    K = 32
    for config in args.configs:
        A, order, cfg = matgen.build_config(config, args.scale)
        A = sp.csc_matrix(A)
        n, ptr, row, val = api.csc_lower_1based(A)
        f = api.Factorization(n, ptr, row, nb=cfg["nb"], nemin=32, prune_tree=False, order=order)
        f.factor(val).wait()
        si = f.sym_info()
        free, total = torch.cuda.mem_get_info()
        var, depth = deepest_leaves(f, K)
        k = len(var)
        B = sp.csc_matrix((np.ones(k), (var, np.arange(k))), shape=(n, k))
        Bd = B.toarray()
        print(f"{config}: n={n} nb={cfg['nb']} arena={si['arena']} doubles, k={k} unit columns at leaves of depth "
              f"{int(depth.min())}..{int(depth.max())}", flush=True)
        for nbatch in args.nbatch:
            need = 8 * (si["arena"] * 1.2 + 3 * 32 * n) * nbatch
            if need > 0.6 * free:
                print(json.dumps({"config": config, "nbatch": nbatch, "skipped": "the members' arenas and workspaces do not fit"}),
                      flush=True)
                continue
            scale = 1.0 + np.arange(nbatch) / 8.0
            assert f.factor_batch(scale[:, None] * val[None, :]) == 0
            dense = np.ascontiguousarray(np.broadcast_to(Bd.T, (nbatch, k, n)))
            paths = {
                "all": (lambda: f.solve_sparse_batch(B),
                        lambda: [f.solve_sparse(B) for _ in range(nbatch)],
                        lambda: f.solve_many_batch(dense).transpose(0, 2, 1)),
                "selected": (lambda: f.solve_sparse_batch(B, rows=var),
                             lambda: [f.solve_sparse(B, rows=var) for _ in range(nbatch)],
                             lambda: f.solve_many_batch(dense).transpose(0, 2, 1)[:, var]),
                "gram": (lambda: f.gram_batch(B),
                         lambda: [f.gram(B) for _ in range(nbatch)],
                         lambda: np.einsum("ik,bij->bkj", Bd, f.solve_many_batch(dense).transpose(0, 2, 1))),
            }
            for what, (batch, single, blocked) in paths.items():
                t = {"batch": [], "single": [], "blocked": []}
                last = {}
                info = host_us = None
                for it in range(args.warmup + args.reps):
                    for name, fn in (("batch", batch), ("single", single), ("blocked", blocked)):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        last[name] = fn()
                        t1 = time.perf_counter()
                        if it >= args.warmup:
                            t[name].append((t1 - t0) * 1e3)
                        if name == "batch":
                            info, host_us = f.solve_sparse_batch_info(), f.program("solve_sparse_batch_host_us")
                got = np.asarray(last["batch"])
                # (the single handle holds member 0's values: A_b = scale_b A, so its numbers divided by scale_b)
                one = np.stack([np.asarray(last["single"][b]) / scale[b] for b in range(nbatch)])
                out = {"config": config, "nbatch": nbatch, "call": what, "k": k,
                       "batch_ms": stats(t["batch"]), "single_sum_ms": stats(t["single"]), "blocked_ms": stats(t["blocked"]),
                       "single_over_batch": round(float(np.median(t["single"])) / float(np.median(t["batch"])), 2),
                       "blocked_over_batch": round(float(np.median(t["blocked"])) / float(np.median(t["batch"])), 2),
                       "rel_diff_batch_single": rel(got, one), "rel_diff_batch_blocked": rel(got, np.asarray(last["blocked"])),
                       "host_us_before_first_device_call": host_us, **info}
                print(json.dumps(out), flush=True)
            f.release_batch()
        f.close()


if __name__ == "__main__":
    main()
