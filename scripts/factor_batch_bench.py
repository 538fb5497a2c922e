#!/usr/bin/env python3
"""Times the batched factorization and solve (spllt_hip_factor_batch_dev / spllt_hip_solve_batch_dev)
against the same members factorized / solved one after the other by the handle's existing path
(spllt_hip_factor_dev + spllt_hip_wait with the default engine; spllt_hip_solve_dev).

  factor_batch_bench.py [--problems p2d32,p2d64,p2d128,p2d256,p3d16,p3d24,p3d32] [--nbatch 1,4,16,64,256,1024]
                        [--reps 10] [--warmup 2] [--max-gb 24] [--member-fast 0|1]

Values and vectors resident in HBM, a host clock around calls that end in a synchronise, both sides
alternating in one process, warm-ups first, median of --reps; a timed window repeats its call until it
holds well over a millisecond.  Members: A_b = D_b A D_b, D_b uniform in [0.5, 2] (seed 100 + b).  At
every size one member's factor is checked against the handle's single factorization (1e-12).  One JSON
line per (problem, nbatch): time per member, GFLOP/s from sym_info()["flops"], the launch count, and the
rate over the 78.6 TFLOP/s fp64 matrix peak -- a WHOLE-PROGRAM rate (initialisation, panels, index
traffic and atomics included), not a kernel rate.  nb = 256, nemin = 32.  Needs a GPU: there is no
fall-back."""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spllt_amd import api, matgen  # noqa: E402

PEAK_TFLOPS = 78.6
PROBLEMS = {"p2d32": lambda: matgen.poisson2d(32), "p2d64": lambda: matgen.poisson2d(64),
            "p2d128": lambda: matgen.poisson2d(128), "p2d256": lambda: matgen.poisson2d(256),
            "p3d16": lambda: matgen.poisson3d(16), "p3d24": lambda: matgen.poisson3d(24),
            "p3d32": lambda: matgen.poisson3d(32)}


def member_values(A, b):
    d = np.random.default_rng(100 + b).uniform(0.5, 2.0, A.shape[0])
    D = sp.diags(d)
    return api.csc_lower_1based(sp.csc_matrix(D @ A @ D))[3]


def lower_mask(f):
    """True where the arena holds L (the strict upper triangle of the diagonal tiles is never read)"""
    mask = np.zeros(f.sym_info()["arena"], dtype=bool)
    for off, w, nr in zip(f.sym("bcol_off"), f.sym("bcol_width"), f.sym("bcol_nrow")):
        m = np.ones((int(nr), int(w)), dtype=bool)
        m[:w, :w] = np.tril(m[:w, :w])
        mask[int(off):int(off) + int(nr) * int(w)] = m.ravel()
    return mask


def timed(fn, sync, min_s=2e-3):
    """seconds per call: the call repeated inside one window until the window lasts min_s"""
    reps = 1
    while True:
        sync()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        dt = time.perf_counter() - t0
        if dt >= min_s or reps >= 4096:
            return dt / reps
        reps = min(4096, max(reps * 2, int(reps * 1.2 * min_s / max(dt, 1e-7)) + 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", default="p2d32,p2d64,p2d128,p2d256,p3d16,p3d24,p3d32")
    ap.add_argument("--nbatch", default="1,4,16,64,256,1024")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--max-gb", type=float, default=24.0, help="skip a batch whose storage would exceed this")
    ap.add_argument("--member-fast", type=int, default=None, help="grid mapping experiment (SPLLT_BATCH_MEMBER_FAST)")
    ap.add_argument("--no-solve", action="store_true")
    args = ap.parse_args()
    if args.reps < 10:
        sys.exit("--reps must be at least 10")
    if args.member_fast is not None:
        os.environ["SPLLT_BATCH_MEMBER_FAST"] = str(args.member_fast)
    import torch
    if not torch.cuda.is_available():
        sys.exit("factor_batch_bench.py needs a GPU")
    sync = torch.cuda.synchronize
    for pname in args.problems.split(","):
        A = sp.csc_matrix(PROBLEMS[pname]())
        n, ptr, row, val = api.csc_lower_1based(A)
        f = api.Factorization(n, ptr, row, nb=256, nemin=32)
        info = f.sym_info()
        flops, arena, nnz = float(info["flops"]), int(info["arena"]), f.nnz
        mask = None
        piv = f.sym("order")
        per_member_gb = 8.0 * (arena + f.program("batch_dinv_size") + nnz + 2 * n) / 1e9
        sizes = [b for b in (int(s) for s in args.nbatch.split(",")) if b * per_member_gb <= args.max_gb]
        if not sizes:
            print(f"# {pname}: skipped, one member needs {per_member_gb:.3f} GB and --max-gb is {args.max_gb}", flush=True)
            f.close()
            continue
        nmax = max(sizes)
        vals = np.stack([member_values(A, b) for b in range(min(nmax, 64))])
        vals = vals[np.arange(nmax) % len(vals)]          # (beyond 64 the members repeat: the values only feed the timing)
        dv = torch.tensor(vals.ravel(), device="cuda")
        rhs = np.random.default_rng(0).standard_normal((nmax, n))
        sync()
        base = dv.data_ptr()
        print(f"# {pname}: n={n} nnz={nnz} arena={arena} flops={flops:.3e} single-program launches="
              f"{len(f.program('launches'))} batch-program launches={int((f.program('batch_launches')[:, 3] > 0).sum()) + 1}",
              flush=True)
        for nbatch in sizes:
            def seq():
                for b in range(nbatch):
                    f.factor_dev(base + 8 * b * nnz).wait()

            def bat():
                rc = f.factor_batch_dev(base, nbatch)
                assert rc == 0, rc
            t = {"seq": [], "bat": []}
            for it in range(args.warmup + args.reps):
                for which, fn in (("seq", seq), ("bat", bat)):
                    dt = timed(fn, sync)
                    if it >= args.warmup:
                        t[which].append(dt)
            # parity of one member against the single factorization (the last sequential one: nbatch - 1)
            if mask is None:
                mask = lower_mask(f)
            got, ref = f.get_factor_batch(nbatch - 1), f.get_factor()
            perr = float(np.abs(got - ref)[mask].max() / np.abs(ref[mask]).max())
            assert perr <= 1e-12, perr
            ts, tb = float(np.median(t["seq"])), float(np.median(t["bat"]))
            rec = {"problem": pname, "nbatch": nbatch, "what": "factor",
                   "seq_ms_per_member": round(ts / nbatch * 1e3, 4), "batch_ms_per_member": round(tb / nbatch * 1e3, 4),
                   "batch_ms": round(tb * 1e3, 3), "ratio": round(ts / tb, 2),
                   "seq_GFLOPs": round(flops * nbatch / ts / 1e9, 1), "batch_GFLOPs": round(flops * nbatch / tb / 1e9, 1),
                   "batch_share_of_fp64_mfma_peak_whole_program": round(flops * nbatch / tb / (PEAK_TFLOPS * 1e12), 4),
                   "batch_launches": f.batch_launches(), "parity_rel_err": perr}
            print(json.dumps(rec), flush=True)
            if args.no_solve:
                continue
            # solve, nrhs = 1, pivot order on both sides
            src = torch.tensor(rhs[:nbatch].ravel(), device="cuda")
            work = torch.empty_like(src)
            sync()
            wp = work.data_ptr()

            def sseq():      # (the handle's single factor is member nbatch - 1: the time does not depend on the values)
                for b in range(nbatch):
                    f.solve_dev(wp + 8 * b * n, 1)

            def sbat():
                f.solve_batch_dev(wp, 1, pivot_order=True)
            t = {"seq": [], "bat": []}
            for it in range(args.warmup + args.reps):
                for which, fn in (("seq", sseq), ("bat", sbat)):
                    work.copy_(src)
                    dt = timed(fn, sync)
                    if it >= args.warmup:
                        t[which].append(dt)
            ts, tb = float(np.median(t["seq"])), float(np.median(t["bat"]))
            print(json.dumps({"problem": pname, "nbatch": nbatch, "what": "solve nrhs=1",
                              "seq_ms_per_member": round(ts / nbatch * 1e3, 4),
                              "batch_ms_per_member": round(tb / nbatch * 1e3, 4), "batch_ms": round(tb * 1e3, 3),
                              "ratio": round(ts / tb, 2)}), flush=True)
        f.close()


if __name__ == "__main__":
    main()
