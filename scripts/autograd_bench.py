#!/usr/bin/env python3
"""Times what a backward pass of the torch front end (spllt_amd.torch_ops) is made of, on the bench workload
(nd24k_like, nb 256) and Poisson3D-128, with 1 and 32 right-hand sides.

  autograd_bench.py [configs] [--nrhs 1,32] [--reps 5] [--warmup 2] [--parts kernel,reader,solve,logdet]

Per configuration and nrhs, alternating in one process, resident tensors, every timed call between host
synchronisations (the library's calls return after their stream has drained), median of --reps after --warmup:
  kernel   pattern_outer_dev alone and solve_many_dev on the same vectors: the two calls of a `solve` backward.
           Bytes of the outer product: 8 per entry for the (row, column) pair, 8 for the output, 4 nvec gathered
           doubles (counted as issued, 32 nvec bytes per entry; the hardware serves the repeats from cache) ->
           achieved GB/s, and the ratio to the solve
  reader   inverse_on_pattern_dev (after one selected_inverse)
  solve    forward + backward of SparseCholesky.solve end to end, factorization included, and with the factor cached
  logdet   forward + backward of SparseCholesky.logdet end to end (factorization, selected inversion, reader)
One JSON line per measurement.  Needs a GPU: there is no fall-back."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spllt_amd import api, matgen  # noqa: E402


def timed(fn, sync, warmup, reps):
    t = []
    for it in range(warmup + reps):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        if it >= warmup:
            t.append(time.perf_counter() - t0)
    return {"ms": round(float(np.median(t)) * 1e3, 3), "min_ms": round(min(t) * 1e3, 3), "max_ms": round(max(t) * 1e3, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("configs", nargs="?", default="nd24k_like,poisson3d_128")
    ap.add_argument("--nrhs", default="1,32")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parts", default="kernel,reader,solve,logdet")
    ap.add_argument("--scale", type=float, default=1.0)
    args = ap.parse_args()
    if args.reps < 3:
        sys.exit("--reps must be at least 3")
    import torch
    if not torch.cuda.is_available():
        sys.exit("autograd_bench.py needs a GPU")
    from spllt_amd.torch_ops import SparseCholesky
    parts = set(args.parts.split(","))
    sync = torch.cuda.synchronize
    for config in args.configs.split(","):
        A, order, cfg = matgen.build_config(config, args.scale)
        if config == "poisson3d_128":
            order = None              # (the built-in nested dissection for this configuration)
        n, ptr, row, val = api.csc_lower_1based(A)
        chol = SparseCholesky((n, ptr, row), nb=cfg["nb"], nemin=32, prune_tree=False, order=order)
        f = chol.f
        nnz = f.nnz
        tv = torch.tensor(val, device="cuda")
        head = {"config": config, "n": n, "nnz": nnz, "nnz_l": int(f.sym_info()["nnz_l"])}
        t0 = time.perf_counter()
        chol.logdet(tv)               # (the first factorization: engine, tables, arena)
        print(json.dumps({**head, "first_factor_and_logdet_s": round(time.perf_counter() - t0, 2)}), flush=True)
        rng = np.random.default_rng(0)
        for nrhs in [int(s) for s in args.nrhs.split(",")]:
            X = torch.tensor(rng.standard_normal((nrhs, n)), device="cuda")
            G = torch.tensor(rng.standard_normal((nrhs, n)), device="cuda")
            if "kernel" in parts:
                out = torch.empty(nnz, dtype=torch.float64, device="cuda")
                work = torch.empty_like(G)

                def outer():
                    f.pattern_outer_dev(G.data_ptr(), X.data_ptr(), nrhs, out.data_ptr(), alpha=-1.0)

                def solve():
                    f.solve_many_dev(work.data_ptr(), nrhs)
                to = timed(outer, sync, args.warmup, args.reps)
                work.copy_(G)
                ts = timed(solve, sync, args.warmup, args.reps)   # (in place on whatever the last call left: same work)
                nbytes = nnz * (16 + 32 * nrhs)
                print(json.dumps({**head, "nrhs": nrhs, "pattern_outer_dev": to, "solve_many_dev": ts,
                                  "outer_over_solve": round(to["ms"] / ts["ms"], 4), "outer_bytes": nbytes,
                                  "outer_GBps": round(nbytes / to["ms"] / 1e6, 1)}), flush=True)
            if "solve" in parts:
                B = X.t()
                Gt = G.t()

                def fwd_bwd(fresh):
                    v = (tv.clone() if fresh else tv).requires_grad_(True)
                    b = B.detach().requires_grad_(True)
                    (chol.solve(v, b) * Gt).sum().backward()
                    v.grad = None
                    v.requires_grad_(False)
                cold = timed(lambda: fwd_bwd(True), sync, args.warmup, args.reps)
                chol.solve(tv, B)
                warm = timed(lambda: fwd_bwd(False), sync, args.warmup, args.reps)
                print(json.dumps({**head, "nrhs": nrhs, "solve_fwd_bwd_with_factorization": cold,
                                  "solve_fwd_bwd_factor_cached": warm}), flush=True)
        if "reader" in parts:
            chol.logdet(tv.clone().requires_grad_(True)).backward()    # (a selected inverse of the current factor)
            out = torch.empty(nnz, dtype=torch.float64, device="cuda")
            tr = timed(lambda: f.inverse_on_pattern_dev(out.data_ptr()), sync, args.warmup, args.reps)
            print(json.dumps({**head, "inverse_on_pattern_dev": tr}), flush=True)
        if "logdet" in parts:
            def ld_fwd_bwd():
                v = tv.clone().requires_grad_(True)
                chol.logdet(v).backward()
            tl = timed(ld_fwd_bwd, sync, 1, max(3, args.reps - 2))
            tf = timed(lambda: f.factor_dev(tv.data_ptr()).wait(), sync, 1, max(3, args.reps - 2))
            chol.invalidate()
            print(json.dumps({**head, "logdet_fwd_bwd_with_factorization": tl, "factor_dev_and_wait": tf}), flush=True)
        chol.close()
        del chol, f


if __name__ == "__main__":
    main()
