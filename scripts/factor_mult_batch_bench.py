#!/usr/bin/env python3
"""Times the batched factor products and samplers (spllt_hip_factor_mult_batch_dev / spllt_hip_sample_batch_dev)
against the same numbers from the handle's single factor: nbatch calls of spllt_hip_factor_mult_dev /
spllt_hip_sample_dev one after the other on ONE arena (the time of a product does not depend on the values).

  factor_mult_batch_bench.py [--configs poisson2d_128,nd24k_like] [--nbatch 1,4,16,64] [--nvec 32] [--reps 10]
                             [--warmup 2] [--max-gb 24] [--member-fast 0|1] [--no-sample]

Vectors resident in HBM, a host clock around calls that end in a synchronise, both sides alternating in one
process, warm-ups first, median and spread (min .. max) of --reps windows; a timed window repeats its call until
it holds well over a millisecond.  Members: A_b = (1 + 0.01 b) A / ||A||_1, so that repeated products stay finite.
At every size member 0's product is checked against A_0 X (1e-12).  One JSON line per (config, nbatch, what).
--member-fast sets SPLLT_BATCH_MULT_MEMBER_FAST: the grid order of the product kernels (0: the member is the slow
axis, the default; 1: the members of one work item are consecutive).  Needs a GPU: there is no fall-back."""
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


def ab(seq, bat, sync, reps, warmup, before=None):
    t = {"seq": [], "bat": []}
    for it in range(warmup + reps):
        for which, fn in (("seq", seq), ("bat", bat)):
            if before:
                before()
            dt = timed(fn, sync)
            if it >= warmup:
                t[which].append(dt)
    return {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="poisson2d_128,nd24k_like")
    ap.add_argument("--nbatch", default="1,4,16,64")
    ap.add_argument("--nvec", type=int, default=32)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--max-gb", type=float, default=24.0, help="skip a batch whose storage would exceed this")
    ap.add_argument("--member-fast", type=int, default=None, help="grid order experiment (SPLLT_BATCH_MULT_MEMBER_FAST)")
    ap.add_argument("--no-sample", action="store_true")
    args = ap.parse_args()
    if args.reps < 10:
        sys.exit("--reps must be at least 10")
    if args.member_fast is not None:
        os.environ["SPLLT_BATCH_MULT_MEMBER_FAST"] = str(args.member_fast)
    import torch
    if not torch.cuda.is_available():
        sys.exit("factor_mult_batch_bench.py needs a GPU")
    sync = torch.cuda.synchronize
    nvec = args.nvec
    for config in args.configs.split(","):
        A, order, cfg = matgen.build_config(config, args.scale)
        A = sp.csc_matrix(A)
        A = A / abs(A).sum(axis=0).max()
        n, ptr, row, val = api.csc_lower_1based(A)
        f = api.Factorization(n, ptr, row, nb=cfg["nb"], nemin=32, prune_tree=False, order=order)
        info = f.sym_info()
        arena, nnz = int(info["arena"]), f.nnz
        stride = max(int(f.program("rsolve_frows")), int(f.program("rsolve_bsize")), 1)
        per_member_gb = 8.0 * (arena + f.program("batch_dinv_size") + nnz + 32 * (3 * n + stride)) / 1e9
        sizes = [b for b in (int(s) for s in args.nbatch.split(",")) if b * per_member_gb <= args.max_gb]
        print(f"# {config}: n={n} nnz={nnz} arena={arena} scratch rows={stride} member storage={per_member_gb:.3f} GB "
              f"tiles={len(f.program('solve_tiles'))} member_fast={os.environ.get('SPLLT_BATCH_MULT_MEMBER_FAST', '0')} "
              f"sizes={sizes}", flush=True)
        if not sizes:
            f.close()
            continue
        f.factor(val).wait()
        nmax = max(sizes)
        dv = torch.tensor(np.stack([(1 + 0.01 * b) * val for b in range(nmax)]).ravel(), device="cuda")
        src = torch.tensor(np.random.default_rng(0).standard_normal((nmax, nvec, n)), device="cuda")
        work = torch.empty_like(src)
        sync()
        wp = work.data_ptr()
        for nbatch in sizes:
            assert f.factor_batch_dev(dv.data_ptr(), nbatch) == 0
            work.copy_(src)
            sync()
            f.factor_mult_batch_dev(wp, nvec, job=0)
            got, want = work[0].cpu().numpy(), (A @ src[0].cpu().numpy().T).T
            perr = float(np.abs(got - want).max() / np.abs(want).max())
            assert perr <= 1e-12, perr
            for job in (1, 0):
                def seq():
                    for b in range(nbatch):
                        f.factor_mult_dev(wp + 8 * b * nvec * n, nvec, job=job)

                def bat():
                    f.factor_mult_batch_dev(wp, nvec, job=job)
                t = ab(seq, bat, sync, args.reps, args.warmup, before=lambda: work.copy_(src))
                ts, tb = t["seq"], t["bat"]
                # bytes one direction reads at least: the arena once per member
                gbs = 8.0 * arena * nbatch * (2 if job == 0 else 1) / tb[0] / 1e9
                print(json.dumps({"config": config, "nbatch": nbatch, "what": f"factor_mult job {job} nvec {nvec}",
                                  "seq_ms": round(ts[0] * 1e3, 4), "seq_ms_min_max": [round(ts[1] * 1e3, 4), round(ts[2] * 1e3, 4)],
                                  "batch_ms": round(tb[0] * 1e3, 4), "batch_ms_min_max": [round(tb[1] * 1e3, 4), round(tb[2] * 1e3, 4)],
                                  "batch_ms_per_member": round(tb[0] / nbatch * 1e3, 4), "ratio": round(ts[0] / tb[0], 2),
                                  "batch_arena_GBs": round(gbs, 1), "parity_rel_err": perr}), flush=True)
            if args.no_sample:
                continue
            for kind in ("covariance", "precision"):
                def sseq():
                    for b in range(nbatch):
                        f.sample_dev(wp + 8 * b * nvec * n, nvec, seed=1, kind=kind)

                def sbat():
                    f.sample_batch_dev(wp, nvec, seed=1, kind=kind)
                t = ab(sseq, sbat, sync, args.reps, args.warmup)
                ts, tb = t["seq"], t["bat"]
                print(json.dumps({"config": config, "nbatch": nbatch, "what": f"sample {kind} nsamp {nvec}",
                                  "seq_us_per_sample": round(ts[0] / (nbatch * nvec) * 1e6, 3),
                                  "batch_us_per_sample": round(tb[0] / (nbatch * nvec) * 1e6, 3),
                                  "batch_us_per_sample_min_max": [round(tb[1] / (nbatch * nvec) * 1e6, 3),
                                                                  round(tb[2] / (nbatch * nvec) * 1e6, 3)],
                                  "ratio": round(ts[0] / tb[0], 2)}), flush=True)
        f.release_batch()
        f.close()


if __name__ == "__main__":
    main()
