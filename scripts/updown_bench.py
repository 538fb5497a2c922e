#!/usr/bin/env python3
"""Measurements of the low-rank update / downdate of the factor on bench configurations.

  updown_bench.py [config ...] [--reps 9] [--warmup 2] [--scale 1.0]      (default: nd24k_like poisson3d_128)

Per configuration: spllt_hip_updown for k = 1 and k = 8 columns a e_i on the first pivots of the deepest leaves
of the elimination tree (k = 1: the longest path to the root), as update / downdate pairs so that the matrix
stays where it was.  Printed per k: the counts of spllt_hip_updown_info; the device time of the sweep
(spllt_hip_updown_time: HIP events on the engine stream around its kernels, what compares with the device time
of a factorization); the time of the whole call between two events and between two host clocks around it (it
returns with the stream drained; both include the host's plan and the staging of W); bytes per second of the
sweep against 16 B x entries visited (one pass: k <= 8); and the device time of a re-factorization of the same
handle in the same process (spllt_hip_factor_times), the path a caller had to take before.  Warm-ups first, median of --reps.  Needs a
GPU: there is no fall-back."""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spllt_amd import api, matgen  # noqa: E402


def deepest_leaves(f, k):
    """user variables of the first pivots of the k deepest leaves"""
    sptr, sparent, order = f.sym("sptr"), f.sym("sparent"), f.sym("order")
    nn = len(sparent)
    depth = np.zeros(nn + 1, dtype=np.int64)
    for s in range(nn - 1, -1, -1):
        depth[s] = depth[min(int(sparent[s]), nn)] + 1
    leaves = np.array(sorted(set(range(nn)) - set(int(p) for p in sparent)))
    pick = leaves[np.argsort(-depth[leaves], kind="stable")[:k]]
    inv = np.empty(f.n, dtype=np.int64)
    inv[order] = np.arange(f.n)
    return inv[sptr[pick]], depth[pick]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("configs", nargs="*", default=["nd24k_like", "poisson3d_128"])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0)
    args = ap.parse_args()
    if args.reps < 5:
        sys.exit("--reps must be at least 5")
    import torch
    if not torch.cuda.is_available():
        sys.exit("updown_bench.py needs a GPU")
    for config in args.configs:
        A, order, cfg = matgen.build_config(config, args.scale)
        A = sp.csc_matrix(A)
        n, ptr, row, val = api.csc_lower_1based(A)
        f = api.Factorization(n, ptr, row, nb=cfg["nb"], nemin=32, prune_tree=False, order=order)
        dval = torch.tensor(val, device="cuda")
        torch.cuda.synchronize()
        tf = []
        for it in range(args.warmup + 3):
            f.factor_dev(dval.data_ptr()).wait()
            tf.append(f.times()["device_ms"])
        refactor_ms = float(np.median(tf[args.warmup:]))
        si = f.sym_info()
        print(f"{config}: n={n} nb={cfg['nb']} arena={si['arena']} doubles, re-factorization {refactor_ms:.3f} ms on the device",
              flush=True)
        stream = torch.cuda.ExternalStream(f.engine_stream())
        diag = A.diagonal()
        for k in (1, 8):
            var, depth = deepest_leaves(f, k)
            W = sp.csc_matrix((0.5 * np.sqrt(diag[var]), (var, np.arange(len(var)))), shape=(n, len(var)))
            ev_ms, host_ms, dev_ms = [], [], []
            for it in range(args.warmup + args.reps):
                for down in (False, True):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    e0.record(stream)
                    f.update(W, downdate=down)
                    e1.record(stream)
                    e1.synchronize()
                    t1 = time.perf_counter()
                    if it >= args.warmup:
                        ev_ms.append(e0.elapsed_time(e1))
                        host_ms.append((t1 - t0) * 1e3)
                        dev_ms.append(f.updown_device_ms())
            info = f.updown_info()
            med = float(np.median(dev_ms))
            nbytes = 16 * info["entries"] * info["passes"]
            print(json.dumps({"config": config, "k": k, "tree_depth_of_first_leaf": int(depth[0]), **info,
                              "fraction_of_arena": round(info["entries"] / max(1, si["arena"]), 4),
                              "device_ms": round(med, 4), "device_min_ms": round(min(dev_ms), 4),
                              "call_event_ms": round(float(np.median(ev_ms)), 4),
                              "host_ms": round(float(np.median(host_ms)), 4), "bytes": nbytes,
                              "GBps": round(nbytes / med / 1e6, 1), "refactor_device_ms": round(refactor_ms, 3),
                              "refactor_over_update": round(refactor_ms / med, 2)}), flush=True)
        # the factor is where it was, to rounding: one solve as a check of the whole sequence
        b = A @ np.ones(n)
        x = f.solve(b)
        r = b - A @ x
        print(json.dumps({"config": config, "bwd_err_after_all_pairs":
                          float(np.linalg.norm(r) / (np.linalg.norm(b) + abs(A).max() * np.linalg.norm(x)))}), flush=True)
        f.close()


if __name__ == "__main__":
    main()
