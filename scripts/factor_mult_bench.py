#!/usr/bin/env python3
"""Times the factor products (spllt_hip_factor_mult_dev, jobs 0 / 1 / 2) and the samplers (spllt_hip_sample_dev,
both kinds) beside the blocked solve (spllt_hip_solve_many_dev, job 0) and the operator product
(spllt_hip_matvec_dev) on the same resident vectors.

  factor_mult_bench.py [config ...] [--nvec 1,32,128] [--reps 5] [--warmup 2] [--inner 10] [--scale 1.0]

Default configurations: the bench workload (nd24k_like) and poisson3d_128.  Everything on device vectors in user
order, the operations alternating in one process; one timed sample is --inner calls in a row, each of which
returns after its stream has drained (host clock around synchronised work); warm-ups first, median and minimum of
--reps samples, per call.  GB/s on L = bytes of the factor arena read per block of 32 vectors and direction /
time.  Checked at the timed size before timing: factor_mult(job 0) against matvec, and solve_many of the product
against the input.  Needs a GPU: there is no fall-back."""
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
    ap.add_argument("configs", nargs="*", default=["nd24k_like", "poisson3d_128"])
    ap.add_argument("--nvec", default="1,32,128")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--scale", type=float, default=1.0)
    args = ap.parse_args()
    if args.reps < 5:
        sys.exit("--reps must be at least 5")
    import torch
    if not torch.cuda.is_available():
        sys.exit("factor_mult_bench.py needs a GPU")
    for config in args.configs:
        A, order, cfg = matgen.build_config(config, args.scale)
        n, ptr, row, val = api.csc_lower_1based(A)
        f = api.Factorization(n, ptr, row, nb=cfg["nb"], nemin=32, prune_tree=False, order=order)
        f.factor(val).wait()
        arena_bytes = 8 * int(f.sym_info()["arena"])
        frows, bsize = f.program("rsolve_frows"), f.program("rsolve_bsize")
        print(json.dumps({"config": config, "n": n, "nb": cfg["nb"], "arena_GB": round(arena_bytes / 1e9, 3),
                          "rsolve_frows": frows, "rsolve_bsize": bsize,
                          "scratch_MB_32": round(8 * 32 * max(frows, bsize) / 1e6, 1),
                          "workspace_MB_32": round(8 * 32 * n / 1e6, 1),
                          "tiles": int(len(f.program("solve_tiles")))}), flush=True)
        dval = torch.tensor(val, device="cuda")
        gen = torch.Generator(device="cuda").manual_seed(0)
        for nvec in [int(s) for s in args.nvec.split(",")]:
            src = torch.randn((nvec, n), dtype=torch.float64, device="cuda", generator=gen)
            work = torch.empty_like(src)
            out = torch.empty_like(src)
            torch.cuda.synchronize()
            ops = {
                "factor_mult_job0": lambda: f.factor_mult_dev(work.data_ptr(), nvec, job=0),
                "factor_mult_job1": lambda: f.factor_mult_dev(work.data_ptr(), nvec, job=1),
                "factor_mult_job2": lambda: f.factor_mult_dev(work.data_ptr(), nvec, job=2),
                "sample_precision": lambda: f.sample_dev(work.data_ptr(), nvec, seed=1, kind="precision"),
                "sample_covariance": lambda: f.sample_dev(work.data_ptr(), nvec, seed=1, kind="covariance"),
                "solve_many_job0": lambda: f.solve_many_dev(work.data_ptr(), nvec, job=0),
                "matvec": lambda: f.matvec_dev(dval.data_ptr(), len(val), work.data_ptr(), out.data_ptr(), nvec),
            }
            # results at the timed size: L L^T x against A x, and the solve of the product against x
            work.copy_(src)
            torch.cuda.synchronize()
            ops["factor_mult_job0"]()
            prod = work.clone()
            work.copy_(src)
            torch.cuda.synchronize()
            ops["matvec"]()
            scale = float(out.abs().max())
            err_matvec = float((prod - out).abs().max()) / scale
            work.copy_(prod)
            torch.cuda.synchronize()
            ops["solve_many_job0"]()
            err_back = float((work - src).abs().max()) / float(src.abs().max())
            t = {k: [] for k in ops}
            for it in range(args.warmup + args.reps):
                for k, op in ops.items():
                    work.copy_(src)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.inner):
                        op()
                    dt = (time.perf_counter() - t0) / args.inner
                    if it >= args.warmup:
                        t[k].append(dt)
            blocks = -(-nvec // 32)
            rec = {"config": config, "nvec": nvec, "blocks": blocks, "inner": args.inner,
                   "max|LLt x - A x|/max|A x|": err_matvec, "max|solve(LLt x) - x|/max|x|": err_back}
            for k, v in t.items():
                rec[k + "_ms"] = [round(float(np.median(v)) * 1e3, 3), round(min(v) * 1e3, 3)]   # median, minimum
            for k, passes in (("factor_mult_job0", 2), ("factor_mult_job1", 1), ("factor_mult_job2", 1), ("solve_many_job0", 2)):
                rec[k + "_GBps_on_L"] = round(arena_bytes * passes * blocks / float(np.median(t[k])) / 1e9, 1)
            print(json.dumps(rec), flush=True)
        f.close()


if __name__ == "__main__":
    main()
