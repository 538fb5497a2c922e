#!/usr/bin/env python3
"""Measurements of the refined solves on a bench configuration or on the mid-size case
of the test-suite.

  refine_bench.py [config | mid] [--reps 5] [--warmup 2] [--scale 1.0] [--parts spmv,overhead,stale]

  spmv      spllt_hip_matvec_dev in pivot order for 1, 4 and 32 resident vectors: time and achieved bytes/s,
            bytes counted from shapes (per chunk of 8 vectors the row pointers, col, src and the gathered
            values once, plus the vectors read and written)
  overhead  spllt_hip_solve_refined_dev with the factorized values (0 iterations) against the plain
            spllt_hip_solve_dev / spllt_hip_solve_many_dev of the same build, 1, 4 and 32 vectors
  stale     values perturbed as A = S A0 S, S = diag(1 + eps u), eps = 0.02 and 0.3, 1 and 32 right-hand sides:
            (a) spllt_hip_factor_dev + wait + solve with the new values against (b) spllt_hip_solve_refined_dev
            (PCG, tol 1e-14) with the factor of A0; iteration counts and host-recomputed backward errors

Everything resident; the variants of a comparison alternate in one process; every timed call lies between host
synchronisations (the calls return after their stream has drained); warm-ups first, median of --reps.  Needs a
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

HBM_BOUND = 6.3e12   # achievable HBM bytes/s of one MI355X (8 TB/s peak)


def timed(fn, before, reps, warmup):
    import torch
    t = []
    for it in range(warmup + reps):
        before()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if it >= warmup:
            t.append(time.perf_counter() - t0)
    return t


def alternating(variants, reps, warmup):
    """variants: name -> (before, fn); one round runs every variant once"""
    import torch
    t = {k: [] for k in variants}
    for it in range(warmup + reps):
        for k, (before, fn) in variants.items():
            before()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if it >= warmup:
                t[k].append(time.perf_counter() - t0)
    return {k: float(np.median(v)) for k, v in t.items()}


def bwd(A, amax, x, b):
    r = b - A @ x
    return float((np.linalg.norm(r, axis=0) / (np.linalg.norm(b, axis=0) + amax * np.linalg.norm(x, axis=0))).max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("config", nargs="?", default="nd24k_like")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--parts", default="spmv,overhead,stale")
    args = ap.parse_args()
    if args.reps < 5:
        sys.exit("--reps must be at least 5")
    import torch
    if not torch.cuda.is_available():
        sys.exit("refine_bench.py needs a GPU")
    if args.config == "mid":
        A0, order, nb = matgen.nd_like((24, 24, 23), 2), None, 128
    else:
        A0, order, cfg = matgen.build_config(args.config, args.scale)
        nb = cfg["nb"]
    A0 = sp.csc_matrix(A0)
    n, ptr, row, val0 = api.csc_lower_1based(A0)
    f = api.Factorization(n, ptr, row, nb=nb, nemin=32, prune_tree=False, order=order)
    f.factor(val0).wait()
    nnz = len(val0)
    piv = f.sym("order")
    rowptr, col, src = f.matvec_tables()
    ent = int(rowptr[-1])
    lens = np.diff(rowptr)
    print(f"{args.config}: n={n} nb={nb} nnz={nnz} operator entries={ent} row length min/median/max="
          f"{int(lens.min())}/{int(np.median(lens))}/{int(lens.max())}", flush=True)
    rng = np.random.default_rng(0)
    dval0 = torch.tensor(val0, device="cuda")
    parts = args.parts.split(",")

    if "spmv" in parts:
        for nvec in (1, 4, 32):
            X = torch.tensor(rng.standard_normal(nvec * n), device="cuda")
            Y = torch.empty_like(X)
            t = timed(lambda: f.matvec_dev(dval0.data_ptr(), nnz, X.data_ptr(), Y.data_ptr(), nvec, pivot_order=True),
                      lambda: None, args.reps, args.warmup)
            chunks = -(-nvec // 8)
            nbytes = chunks * (ent * (4 + 4 + 8) + (n + 1) * 8 + n * 4) + nvec * n * 16
            med = float(np.median(t))
            print(json.dumps({"part": "spmv", "nvec": nvec, "ms": round(med * 1e3, 4), "min_ms": round(min(t) * 1e3, 4),
                              "bytes": nbytes, "GBps": round(nbytes / med / 1e9, 1),
                              "fraction_of_hbm_bound": round(nbytes / med / HBM_BOUND, 3)}), flush=True)

    if "overhead" in parts:
        for nrhs in (1, 4, 32):
            B = np.asfortranarray(A0 @ rng.standard_normal((n, nrhs)))
            Bp = np.empty((nrhs, n))
            Bp[:, piv] = B.T
            src_u = torch.tensor(B.T.ravel(), device="cuda")
            src_p = torch.tensor(Bp.ravel(), device="cuda")
            work = torch.empty_like(src_u)
            res = {}

            def plain():
                if nrhs <= 4:
                    f.solve_dev(work.data_ptr(), nrhs)
                else:
                    f.solve_many_dev(work.data_ptr(), nrhs, pivot_order=True)

            def refined():
                res["r"] = f.solve_refined_dev(dval0.data_ptr(), nnz, work.data_ptr(), nrhs, method="pcg", tol=1e-14)

            t = alternating({"plain": (lambda: work.copy_(src_p), plain), "refined": (lambda: work.copy_(src_u), refined)},
                            args.reps, args.warmup)
            rc, it, err = res["r"]
            print(json.dumps({"part": "overhead", "nrhs": nrhs, "plain_ms": round(t["plain"] * 1e3, 3),
                              "refined_ms": round(t["refined"] * 1e3, 3),
                              "difference_ms": round((t["refined"] - t["plain"]) * 1e3, 3),
                              "ratio": round(t["refined"] / t["plain"], 3), "status": rc, "iterations": int(it.max()),
                              "max_error": float(err.max())}), flush=True)

    if "stale" in parts:
        for eps in (0.02, 0.3):
            s = 1.0 + eps * rng.random(n)
            A = sp.csc_matrix(sp.diags(s) @ A0 @ sp.diags(s))
            val = api.csc_lower_1based(A)[3]
            amax = abs(A).max()
            dval = torch.tensor(val, device="cuda")
            for nrhs in (1, 32):
                B = np.asfortranarray(A @ rng.standard_normal((n, nrhs)))
                src_u = torch.tensor(B.T.ravel(), device="cuda")
                work = torch.empty_like(src_u)
                res = {}

                def refactor():
                    f.factor_dev(dval.data_ptr()).wait()
                    f.solve_many_dev(work.data_ptr(), nrhs)

                def restore():
                    work.copy_(src_u)
                    f.factor_dev(dval0.data_ptr()).wait()     # the stale factor is that of A0

                def stale():
                    res["r"] = f.solve_refined_dev(dval.data_ptr(), nnz, work.data_ptr(), nrhs, method="pcg", tol=1e-14,
                                                   max_iter=100)

                t = alternating({"refactor": (lambda: work.copy_(src_u), refactor), "stale": (restore, stale)},
                                args.reps, args.warmup)
                # the solutions of one more, untimed, call each
                work.copy_(src_u)
                refactor()
                res["xa"] = work.cpu().numpy().reshape(nrhs, n).T
                restore()
                stale()
                res["xb"] = work.cpu().numpy().reshape(nrhs, n).T
                rc, it, err = res["r"]
                print(json.dumps({"part": "stale", "eps": eps, "nrhs": nrhs,
                                  "factor_wait_solve_ms": round(t["refactor"] * 1e3, 3),
                                  "pcg_stale_factor_ms": round(t["stale"] * 1e3, 3),
                                  "ratio_refactor_over_pcg": round(t["refactor"] / t["stale"], 3), "status": rc,
                                  "iterations_min_max": [int(it.min()), int(it.max())],
                                  "reported_error": float(err.max()),
                                  "host_bwd_err": [bwd(A, amax, res["xa"], B), bwd(A, amax, res["xb"], B)]}), flush=True)
    f.close()


if __name__ == "__main__":
    main()
