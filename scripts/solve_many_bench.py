#!/usr/bin/env python3
"""Times the existing device solve (spllt_hip_solve_dev, 4 right-hand sides per sweep) against the
blocked one (spllt_hip_solve_many_dev, 32 per sweep on the fp64 matrix cores) on a bench configuration.

  solve_many_bench.py [config] [--nrhs 4,16,32,128,512] [--reps 5] [--warmup 2] [--scale 1.0]

Both on resident vectors in pivot order, alternating in one process, every timed call between host
synchronisations (both calls return after their stream has drained), warm-ups first, median of --reps.
GB/s on L = bytes of the factor arena read per sweep / time per sweep (old: ceil(nrhs / 4) sweeps, new:
ceil(nrhs / 32)).  Needs a GPU: there is no fall-back."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spllt_amd import api, matgen  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("config", nargs="?", default="nd24k_like")
    ap.add_argument("--nrhs", default="4,16,32,128,512")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0)
    args = ap.parse_args()
    if args.reps < 5:
        sys.exit("--reps must be at least 5")
    import torch
    if not torch.cuda.is_available():
        sys.exit("solve_many_bench.py needs a GPU")
    A, order, cfg = matgen.build_config(args.config, args.scale)
    n, ptr, row, val = api.csc_lower_1based(A)
    f = api.Factorization(n, ptr, row, nb=cfg["nb"], nemin=32, prune_tree=False, order=order)
    f.factor(val).wait()
    arena_bytes = 8 * int(f.sym_info()["arena"])
    piv = f.sym("order")
    print(f"{args.config}: n={n} nb={cfg['nb']} L arena {arena_bytes / 1e9:.3f} GB", flush=True)
    rng = np.random.default_rng(0)
    amax = abs(A).max()
    for nrhs in [int(s) for s in args.nrhs.split(",")]:
        X = rng.standard_normal((n, nrhs))
        B = A @ X
        Bp = np.empty((nrhs, n))
        Bp[:, piv] = B.T
        src = torch.tensor(Bp.ravel(), device="cuda")
        work = torch.empty_like(src)
        t = {"old": [], "new": []}
        err = {}
        for it in range(args.warmup + args.reps):
            for which in ("old", "new"):
                work.copy_(src)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if which == "old":
                    f.solve_dev(work.data_ptr(), nrhs)
                else:
                    f.solve_many_dev(work.data_ptr(), nrhs, pivot_order=True)
                dt = time.perf_counter() - t0
                if it >= args.warmup:
                    t[which].append(dt)
                if it == 0:
                    # scaled backward error of up to 8 of the vectors (evenly spaced, first and last included)
                    cols = np.unique(np.linspace(0, nrhs - 1, min(nrhs, 8)).astype(int))
                    got = work.cpu().numpy().reshape(nrhs, n)[cols][:, piv].T
                    R = B[:, cols] - A @ got
                    err[which] = float((np.linalg.norm(R, axis=0) / (np.linalg.norm(B[:, cols], axis=0) +
                                                                     amax * np.linalg.norm(got, axis=0))).max())
        old, new = float(np.median(t["old"])), float(np.median(t["new"]))
        so, sn = -(-nrhs // 4), -(-nrhs // 32)
        print(json.dumps({"config": args.config, "nrhs": nrhs, "solve_dev_ms": round(old * 1e3, 3),
                          "solve_many_dev_ms": round(new * 1e3, 3), "ratio": round(old / new, 2),
                          "solve_dev_sweeps": so, "solve_many_sweeps": sn,
                          "solve_dev_GBps_on_L": round(2 * arena_bytes * so / old / 1e9, 1),
                          "solve_many_GBps_on_L": round(2 * arena_bytes * sn / new / 1e9, 1),
                          "min_ms": [round(min(t["old"]) * 1e3, 3), round(min(t["new"]) * 1e3, 3)],
                          "max_bwd_err": [err["old"], err["new"]]}), flush=True)
    f.close()


if __name__ == "__main__":
    main()
