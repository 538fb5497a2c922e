#!/usr/bin/env python3
"""Measurements of the low-rank update / downdate of the factors of a batch.

  updown_batch_bench.py [config ...] [--nbatch 4 16 64] [--reps 9] [--warmup 2] [--scale 1.0]
                                                                (default: nd24k_like poisson2d_128)

Per configuration, nbatch and k = 1 / 8: spllt_hip_updown_batch of the columns 0.5 sqrt(a_ii) e_i on the first
pivots of the deepest leaves (the set-up of updown_bench.py; every member gets the same values: the members are
copies of the configuration's matrix), as update / downdate pairs so that the matrices stay where they were.  One
more row per nbatch: leave-one-out, k = 8 with member b non-zero in column b mod 8 only.  Printed per point: the
counts of spllt_hip_updown_batch_info; the device time of the sweep (spllt_hip_updown_batch_time, HIP events
around its kernels) and the host time around the call, medians of --reps after --warmup with the smallest and the
largest sample; and in the same process what a caller had before:
  (a) nbatch single-handle spllt_hip_updown sweeps one after the other: the sum of their spllt_hip_updown_time and
      the host time around the nbatch calls (the same handle, alternating update and downdate);
  (b) spllt_hip_factor_batch_dev of the members (host time around the call: it returns with the stream drained).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("configs", nargs="*", default=["nd24k_like", "poisson2d_128"])
    ap.add_argument("--nbatch", type=int, nargs="*", default=[4, 16, 64])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0)
    args = ap.parse_args()
    if args.reps < 5:
        sys.exit("--reps must be at least 5")
    import torch
    if not torch.cuda.is_available():
        sys.exit("updown_batch_bench.py needs a GPU")
    for config in args.configs:
        A, order, cfg = matgen.build_config(config, args.scale)
        A = sp.csc_matrix(A)
        n, ptr, row, val = api.csc_lower_1based(A)
        f = api.Factorization(n, ptr, row, nb=cfg["nb"], nemin=32, prune_tree=False, order=order)
        dval = torch.tensor(val, device="cuda")
        f.factor_dev(dval.data_ptr()).wait()
        si = f.sym_info()
        free, total = torch.cuda.mem_get_info()
        print(f"{config}: n={n} nb={cfg['nb']} arena={si['arena']} doubles", flush=True)
        diag = A.diagonal()
        for nbatch in args.nbatch:
            need = 8 * (si["arena"] * 1.2 + 8 * n) * nbatch
            if need > 0.6 * free:
                print(json.dumps({"config": config, "nbatch": nbatch, "skipped": "the members' arenas do not fit"}), flush=True)
                continue
            dvals = dval.repeat(nbatch, 1).contiguous()
            torch.cuda.synchronize()
            tb = []
            for it in range(args.warmup + 3):
                t0 = time.perf_counter()
                assert f.factor_batch_dev(dvals.data_ptr(), nbatch) == 0
                tb.append((time.perf_counter() - t0) * 1e3)
            factor_batch_ms = stats(tb[args.warmup:])
            rows = [(1, False), (8, False), (8, True)]
            for k, loo in rows:
                var, depth = deepest_leaves(f, k)
                k = len(var)
                W = sp.csc_matrix((0.5 * np.sqrt(diag[var]), (var, np.arange(k))), shape=(n, k))
                wv = np.tile(W.data, (nbatch, 1))
                if loo:
                    for b in range(nbatch):
                        keep = wv[b, b % k]
                        wv[b] = 0.0
                        wv[b, b % k] = keep
                # (a) the single handle, nbatch sweeps one after the other
                if not loo:
                    seq_dev, seq_host = [], []
                    for it in range(args.warmup + args.reps):
                        for _ in range(2):                 # (as many samples as the batch's update / downdate pairs)
                            torch.cuda.synchronize()
                            acc = 0.0
                            t0 = time.perf_counter()
                            for b in range(nbatch):        # (update, downdate, update, ...: the factor stays put)
                                f.update(W, downdate=b % 2 == 1)
                                acc += f.updown_device_ms()
                            t1 = time.perf_counter()
                            if it >= args.warmup:
                                seq_dev.append(acc)
                                seq_host.append((t1 - t0) * 1e3)
                            if nbatch % 2:                 # (an odd count: undo the last one, outside the clock)
                                f.update(W, downdate=True)
                dev_ms, host_ms = [], []
                for it in range(args.warmup + args.reps):
                    for down in (False, True):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        assert f.update_batch(W, wv, downdate=down) == 0
                        t1 = time.perf_counter()
                        if it >= args.warmup:
                            dev_ms.append(f.updown_batch_device_ms())
                            host_ms.append((t1 - t0) * 1e3)
                info = f.updown_batch_info()
                med = float(np.median(dev_ms))
                nbytes = 16 * info["entries"] * info["passes"] * nbatch
                out = {"config": config, "nbatch": nbatch, "k": k, "leave_one_out": loo,
                       "tree_depth_of_first_leaf": int(depth[0]), **info, "device_ms": stats(dev_ms),
                       "host_ms": stats(host_ms), "GBps_union_path": round(nbytes / med / 1e6, 1),
                       "factor_batch_host_ms": factor_batch_ms,
                       "factor_batch_over_batch_sweep": round(factor_batch_ms["median"] / float(np.median(host_ms)), 2)}
                if not loo:
                    out.update({"sequential_device_ms": stats(seq_dev), "sequential_host_ms": stats(seq_host),
                                "sequential_over_batch_device": round(float(np.median(seq_dev)) / med, 2),
                                "sequential_over_batch_host": round(float(np.median(seq_host)) / float(np.median(host_ms)), 2)})
                print(json.dumps(out), flush=True)
            # the members are where they were, to rounding: one solve as a check of the whole sequence
            b = A @ np.ones(n)
            x = f.solve_batch(np.tile(b, (nbatch, 1)))
            bwd = max(float(np.linalg.norm(b - A @ x[m]) / (np.linalg.norm(b) + abs(A).max() * np.linalg.norm(x[m])))
                      for m in range(nbatch))
            print(json.dumps({"config": config, "nbatch": nbatch, "bwd_err_after_all_pairs": bwd}), flush=True)
            f.release_batch()
            del dvals
        f.close()


if __name__ == "__main__":
    main()
