#!/usr/bin/env python3
"""Times the blocked batch solve (spllt_hip_solve_many_batch_dev) against two yardsticks in the same run:

  batch   spllt_hip_solve_batch_dev on the same batch: the existing way to the same numbers (one vector of one
          member per workgroup, fp64 VALU)
  seq     nbatch calls of spllt_hip_solve_many_dev one after the other on ONE arena (the handle's single factor;
          the time of a solve does not depend on the values)

and the precision kind of spllt_hip_sample_batch_dev with the routing switch off and on.

  solve_many_batch_bench.py [--configs poisson2d_128,nd24k_like] [--nbatch 1,4,16,64] [--nrhs 1,8,32,128]
                            [--jobs 0,2] [--reps 10] [--warmup 2] [--max-gb 24] [--no-sample] [--out FILE]

The method of factor_mult_batch_bench.py: vectors resident in HBM, a host clock around calls that end in a
synchronise, all sides alternating in one process, warm-ups first, median and spread (min .. max) of --reps
windows; a timed window repeats its call until it holds at least 2 ms.  The vectors are restored before every
window; inside a window the solves run in place on their own results (the time of a solve does not depend on the
values).  Members: A_b = (1 + 0.01 b) A / ||A||_1.  At every size the blocked result is checked against
solve_batch_dev (1e-10 of the largest entry: two backward-stable solves of a matrix whose condition number is near
1e4 differ by that much at the most; the figure is in the output).  One JSON line per (config, nbatch, nrhs, job); --out appends the
lines to a file as well.  nd24k_like runs at nbatch 1, 4, 16 (--nbatch is cut by --max-gb and, for that config,
at 16).  Needs a GPU: there is no fall-back."""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spllt_amd import api, matgen  # noqa: E402


def timed(fn, sync, min_s=2e-3):
    """seconds per call: the call repeated inside one window until the window lasts min_s"""
    reps = 1
    while True:
        sync()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        dt = time.perf_counter() - t0
        if dt >= min_s or reps >= 256:
            return dt / reps
        reps = min(256, max(reps * 2, int(reps * 1.2 * min_s / max(dt, 1e-7)) + 1))


def alternate(sides, sync, reps, warmup, before=None):
    """sides: {name: fn}; (median, min, max) seconds per call of every side, the sides taking turns"""
    t = {k: [] for k in sides}
    for it in range(warmup + reps):
        for which, fn in sides.items():
            if before:
                before()
            dt = timed(fn, sync)
            if it >= warmup:
                t[which].append(dt)
    return {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in t.items()}


def ms(t):
    return round(t[0] * 1e3, 4), [round(t[1] * 1e3, 4), round(t[2] * 1e3, 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="poisson2d_128,nd24k_like")
    ap.add_argument("--nbatch", default="1,4,16,64")
    ap.add_argument("--nrhs", default="1,8,32,128")
    ap.add_argument("--jobs", default="0,2")
    ap.add_argument("--nsamp", type=int, default=32)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--max-gb", type=float, default=24.0, help="skip a batch whose storage would exceed this")
    ap.add_argument("--no-sample", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 10:
        sys.exit("--reps must be at least 10")
    import torch
    if not torch.cuda.is_available():
        sys.exit("solve_many_batch_bench.py needs a GPU")
    sync = torch.cuda.synchronize
    out = open(args.out, "a") if args.out else None

    def emit(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    rhs = [int(s) for s in args.nrhs.split(",")]
    jobs = [int(s) for s in args.jobs.split(",")]
    rmax = max(rhs + [args.nsamp])
    for config in args.configs.split(","):
        A, order, cfg = matgen.build_config(config, args.scale)
        A = sp.csc_matrix(A)
        A = A / abs(A).sum(axis=0).max()
        n, ptr, row, val = api.csc_lower_1based(A)
        f = api.Factorization(n, ptr, row, nb=cfg["nb"], nemin=32, prune_tree=False, order=order)
        arena, nnz = int(f.sym_info()["arena"]), f.nnz
        # arena + dinv + values + the vectors, their copy, the workspace of solve_batch and the blocked workspace
        per_member_gb = 8.0 * (arena + f.program("batch_dinv_size") + nnz + (3 * rmax + 32) * n) / 1e9
        cap = 16 if config == "nd24k_like" else 1 << 30
        sizes = [b for b in (int(s) for s in args.nbatch.split(",")) if b * per_member_gb <= args.max_gb and b <= cap]
        emit(f"# {config}: n={n} nnz={nnz} arena={arena} member storage={per_member_gb:.3f} GB sizes={sizes} nrhs={rhs} "
             f"jobs={jobs}")
        if not sizes:
            f.close()
            continue
        f.factor(val).wait()
        nmax = max(sizes)
        dv = torch.tensor(np.stack([(1 + 0.01 * b) * val for b in range(nmax)]).ravel(), device="cuda")
        rng = np.random.default_rng(0)
        for nbatch in sizes:
            assert f.factor_batch_dev(dv.data_ptr(), nbatch) == 0
            for nrhs in rhs:
                src = torch.tensor(rng.standard_normal((nbatch, nrhs, n)), device="cuda")
                work = torch.empty_like(src)
                wp = work.data_ptr()
                for job in jobs:
                    work.copy_(src)
                    sync()
                    f.solve_many_batch_dev(wp, nrhs, job=job)
                    got = work.cpu().numpy()
                    work.copy_(src)
                    sync()
                    f.solve_batch_dev(wp, nrhs, job=job)
                    want = work.cpu().numpy()
                    perr = float(np.abs(got - want).max() / np.abs(want).max())
                    assert perr <= 1e-10, perr
                    info = f.solve_many_batch_info()

                    def blocked():
                        f.solve_many_batch_dev(wp, nrhs, job=job)

                    def batch():
                        f.solve_batch_dev(wp, nrhs, job=job)

                    def seq():
                        for b in range(nbatch):
                            f.solve_many_dev(wp + 8 * b * nrhs * n, nrhs, job=job)
                    t = alternate({"blocked": blocked, "batch": batch, "seq": seq}, sync, args.reps, args.warmup,
                                  before=lambda: work.copy_(src))
                    tb, to, ts = t["blocked"], t["batch"], t["seq"]
                    # bytes a sweep reads at least: the arena once per member and block
                    gbs = 8.0 * arena * nbatch * info["blocks"] * (2 if job == 0 else 1) / tb[0] / 1e9
                    emit(json.dumps({"config": config, "nbatch": nbatch, "nrhs": nrhs, "job": job,
                                     "blocked_ms": ms(tb)[0], "blocked_ms_min_max": ms(tb)[1],
                                     "solve_batch_ms": ms(to)[0], "solve_batch_ms_min_max": ms(to)[1],
                                     "seq_solve_many_ms": ms(ts)[0], "seq_solve_many_ms_min_max": ms(ts)[1],
                                     "vs_solve_batch": round(to[0] / tb[0], 2), "vs_seq": round(ts[0] / tb[0], 2),
                                     "blocked_us_per_vector": round(tb[0] / (nbatch * nrhs) * 1e6, 3),
                                     "blocked_arena_GBs": round(gbs, 1), "launches": info["launches"],
                                     "parity_rel_err": perr}))
                del src, work
            if args.no_sample:
                continue
            ns = args.nsamp
            work = torch.empty((nbatch, ns, n), dtype=torch.float64, device="cuda")
            wp = work.data_ptr()

            def routed(on):
                def fn():
                    f.sample_batch_dev(wp, ns, seed=1, kind="precision")

                def run():
                    before = f.set_batch_blocked_solve(on)
                    try:
                        return timed(fn, sync)
                    finally:
                        f.set_batch_blocked_solve(before)
                return run

            def sseq():
                for b in range(nbatch):
                    f.sample_dev(wp + 8 * b * ns * n, ns, seed=1, kind="precision")
            t = {"off": [], "on": [], "seq": []}
            for it in range(args.warmup + args.reps):
                for which, run in (("off", routed(False)), ("on", routed(True)), ("seq", lambda: timed(sseq, sync))):
                    dt = run()
                    if it >= args.warmup:
                        t[which].append(dt)
            per = 1e6 / (nbatch * ns)
            med = {k: float(np.median(v)) for k, v in t.items()}
            emit(json.dumps({"config": config, "nbatch": nbatch, "what": f"sample precision nsamp {ns}",
                             "off_us_per_sample": round(med["off"] * per, 3),
                             "off_us_per_sample_min_max": [round(min(t["off"]) * per, 3), round(max(t["off"]) * per, 3)],
                             "on_us_per_sample": round(med["on"] * per, 3),
                             "on_us_per_sample_min_max": [round(min(t["on"]) * per, 3), round(max(t["on"]) * per, 3)],
                             "seq_us_per_sample": round(med["seq"] * per, 3),
                             "off_vs_seq": round(med["seq"] / med["off"], 2), "on_vs_seq": round(med["seq"] / med["on"], 2)}))
            del work
        f.release_batch()
        f.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
