#!/usr/bin/env python3
"""Times the existing device solve (spllt_hip_solve_dev, fp64 atomic adds) against the reproducible one
(spllt_hip_solve_repro_dev: strips store, diagonal launches gather in table order) on a bench configuration
or on the mid-size case of the test-suite (nd_like((24, 24, 23), 2), nb 128).

  solve_repro_bench.py [config | mid] [--nrhs 1,4,16,64] [--reps 5] [--warmup 2] [--scale 1.0]

Both on resident vectors in pivot order, alternating in one process, every timed call between host
synchronisations (both calls return after their stream has drained), warm-ups first, median of --reps.
Both paths sweep 4, 2 or 1 vectors at a time; GB/s on L = bytes of the factor arena read per sweep pair /
time.  Also prints rsolve_frows, the longest gather list and the scratch bytes, and checks that two calls of
the reproducible path return the same bits.  Needs a GPU: there is no fall-back."""
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
    ap.add_argument("--nrhs", default="1,4,16,64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0)
    args = ap.parse_args()
    if args.reps < 5:
        sys.exit("--reps must be at least 5")
    import torch
    if not torch.cuda.is_available():
        sys.exit("solve_repro_bench.py needs a GPU")
    if args.config == "mid":
        A, order, nb = matgen.nd_like((24, 24, 23), 2), None, 128
    else:
        A, order, cfg = matgen.build_config(args.config, args.scale)
        nb = cfg["nb"]
    n, ptr, row, val = api.csc_lower_1based(A)
    f = api.Factorization(n, ptr, row, nb=nb, nemin=32, prune_tree=False, order=order)
    f.factor(val).wait()
    arena_bytes = 8 * int(f.sym_info()["arena"])
    piv = f.sym("order")
    frows, bsize = f.program("rsolve_frows"), f.program("rsolve_bsize")
    lens = np.diff(f.program("rsolve_gptr"))
    print(json.dumps({"config": args.config, "n": n, "nb": nb, "L_arena_GB": round(arena_bytes / 1e9, 3),
                      "launches_fwd_bwd": [len(f.program("solve_fwd")), len(f.program("solve_bwd"))],
                      "rsolve_frows": frows, "rsolve_bsize": bsize, "longest_gather_list": int(lens.max()),
                      "mean_gather_list": round(float(lens.mean()), 1),
                      "scratch_bytes": 8 * 4 * max(frows, bsize),
                      "table_bytes": 8 * (2 * len(f.program("rsolve_fslot")) + n + 1 + frows
                                          + len(f.program("rsolve_bslot"))) + 4 * n}), flush=True)
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
        err, first_bits, same_bits = {}, None, True
        for it in range(args.warmup + args.reps):
            for which in ("old", "new"):
                work.copy_(src)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if which == "old":
                    f.solve_dev(work.data_ptr(), nrhs)
                else:
                    f.solve_reproducible_dev(work.data_ptr(), nrhs, pivot_order=True)
                dt = time.perf_counter() - t0
                if it >= args.warmup:
                    t[which].append(dt)
                if it == 0:
                    cols = np.unique(np.linspace(0, nrhs - 1, min(nrhs, 8)).astype(int))
                    got = work.cpu().numpy().reshape(nrhs, n)[cols][:, piv].T
                    R = B[:, cols] - A @ got
                    err[which] = float((np.linalg.norm(R, axis=0) / (np.linalg.norm(B[:, cols], axis=0) +
                                                                     amax * np.linalg.norm(got, axis=0))).max())
                if which == "new" and it < 2:     # (warm-up iterations: the copies back are not timed)
                    bits = work.cpu().numpy()
                    if first_bits is None:
                        first_bits = bits
                    else:
                        same_bits = bool(np.array_equal(bits, first_bits))
        old, new = float(np.median(t["old"])), float(np.median(t["new"]))
        sweeps = nrhs // 4 + (nrhs % 4) // 2 + nrhs % 2
        print(json.dumps({"config": args.config, "nrhs": nrhs, "solve_dev_ms": round(old * 1e3, 3),
                          "solve_repro_dev_ms": round(new * 1e3, 3), "repro_over_dev": round(new / old, 3),
                          "sweeps": sweeps,
                          "solve_dev_GBps_on_L": round(2 * arena_bytes * sweeps / old / 1e9, 1),
                          "solve_repro_GBps_on_L": round(2 * arena_bytes * sweeps / new / 1e9, 1),
                          "min_ms": [round(min(t["old"]) * 1e3, 3), round(min(t["new"]) * 1e3, 3)],
                          "max_bwd_err": [err["old"], err["new"]], "repro_same_bits": same_bits}), flush=True)
    f.close()


if __name__ == "__main__":
    main()
