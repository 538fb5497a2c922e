#!/usr/bin/env python3
"""Times the product and the refined solves of a batch (include/spllt_hip_batch_refine.h).  Per (config, nbatch,
vectors per member), one JSON line each:

  spmv      spllt_hip_matvec_batch_dev alone (pivot order): time, and GB/s from bytes derived from the shapes -- per
            member the values gathered once per entry of the full pattern and x, y once per vector; the index
            streams (col, src: 8 bytes per entry) counted ONCE for the batch
  ask       spllt_hip_solve_refined_batch_dev with the values that were factorized (eps = 0, PCG, tol 1e-14: no
            iteration) against the plain spllt_hip_solve_batch_dev / spllt_hip_solve_many_batch_dev: the cost of asking
  moved     eps = 0.02 and 0.3: PCG on the stale batch factor to 1e-14, against spllt_hip_factor_batch_dev with the
            new values plus a plain solve, and against nbatch sequential spllt_hip_solve_refined_dev on the single
            handle (those three entry points are what the parent commit has: this change touches none of their
            kernels); the iteration counts
  mixed     member 0 at eps = 0.3, the others at eps = 0, against the all-eps-0 batch and against member 0 ALONE in
            a batch of one: what the converged members cost by riding along
  route     eps = 0.02 with M^-1 forced to spllt_hip_solve_batch_dev (SPLLT_BRF_BLOCKED_MIN=1000000) and to the
            blocked solve (=1): the crossover behind BRF_BLOCKED_MIN.  (--threshold N runs every OTHER measurement
            with SPLLT_BRF_BLOCKED_MIN=N; the first recorded runs used 8, the value before the crossover was
            measured)

  refine_batch_bench.py [--configs poisson2d_128,nd24k_like] [--nbatch 4,16,64] [--nvec 1,2,4,8,32] [--reps 5]
                        [--max-gb 40] [--out FILE]

Members: S_b A0 S_b, S_b = diag(1 + eps u_b), factorized as A0.  Vectors resident in HBM and restored before every
call; a host clock around calls that end in a synchronise; the sides alternate; median and (min, max) of --reps
calls after one warm-up.  Needs a GPU: there is no fall-back."""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spllt_amd import api, matgen  # noqa: E402

TOL, MAX_ITER = 1e-14, 60


def alternate(sides, sync, reps, before):
    t = {k: [] for k in sides}
    for it in range(reps + 1):
        for which, fn in sides.items():
            before()
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            if it:
                t[which].append(time.perf_counter() - t0)
    return {k: [round(float(np.median(v)) * 1e3, 3), round(min(v) * 1e3, 3), round(max(v) * 1e3, 3)] for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="poisson2d_128,nd24k_like")
    ap.add_argument("--nbatch", default="4,16,64")
    ap.add_argument("--nvec", default="1,2,4,8,32")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--max-gb", type=float, default=40.0, help="skip a batch whose storage would exceed this")
    ap.add_argument("--out", default=None)
    ap.add_argument("--threshold", type=int, default=None, help="SPLLT_BRF_BLOCKED_MIN outside the route measurement")
    args = ap.parse_args()
    if args.threshold:
        os.environ["SPLLT_BRF_BLOCKED_MIN"] = str(args.threshold)
    import torch
    if not torch.cuda.is_available():
        sys.exit("refine_batch_bench.py needs a GPU")
    sync = torch.cuda.synchronize
    out = open(args.out, "a") if args.out else None

    def emit(obj):
        line = obj if isinstance(obj, str) else json.dumps(obj)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    nvecs = [int(s) for s in args.nvec.split(",")]
    for config in args.configs.split(","):
        A, order, cfg = matgen.build_config(config, args.scale)
        A0 = sp.csc_matrix(A)
        A0 = A0 / abs(A0).sum(axis=0).max()
        n, ptr, row, val0 = api.csc_lower_1based(A0)
        f = api.Factorization(n, ptr, row, nb=cfg["nb"], nemin=32, prune_tree=False, order=order)
        nnz, arena = f.nnz, int(f.sym_info()["arena"])
        nnz_full = int(f.matvec_tables()[0][-1])
        col_of = np.repeat(np.arange(n), np.diff(ptr))
        row_of = np.asarray(row[:nnz]) - 1
        # arena + values + six work arrays, the vectors and their copy at 32 per member
        per_member_gb = 8.0 * (arena + 2 * nnz + 8 * 32 * n) / 1e9
        sizes = [b for b in (int(s) for s in args.nbatch.split(",")) if b * per_member_gb <= args.max_gb]
        emit(f"# {config}: n={n} nnz={nnz} entries of the full pattern={nnz_full} arena={arena} member storage="
             f"{per_member_gb:.3f} GB sizes={sizes} nvec={nvecs}")
        f.factor(val0).wait()
        rng = np.random.default_rng(0)

        def moved(eps, b):
            s = 1.0 + eps * np.random.default_rng(1000 + b).random(n)
            return val0 * s[row_of] * s[col_of]

        for nbatch in sizes:
            dv0 = torch.tensor(np.stack([val0] * nbatch).ravel(), device="cuda")
            dvals = {eps: torch.tensor(np.stack([moved(eps, b) for b in range(nbatch)]).ravel(), device="cuda")
                     for eps in (0.02, 0.3)}
            dmixed = torch.tensor(np.stack([moved(0.3, 0)] + [val0] * (nbatch - 1)).ravel(), device="cuda")
            for nvec in nvecs:
                src = torch.tensor(rng.standard_normal((nbatch, nvec, n)), device="cuda")
                work, ybuf = torch.empty_like(src), torch.empty_like(src)
                wp = work.data_ptr()
                restore = lambda: work.copy_(src)   # noqa: E731
                base = {"config": config, "nbatch": nbatch, "nvec": nvec}
                # 1. the product alone
                t = alternate({"spmv": lambda: f.matvec_batch_dev(dv0.data_ptr(), nbatch, wp, ybuf.data_ptr(), nvec, pivot_order=True)},
                              sync, args.reps, restore)
                nbytes = nbatch * (8.0 * nnz_full + 16.0 * nvec * n) + 8.0 * nnz_full
                emit(dict(base, what="spmv", ms=t["spmv"], bytes=nbytes, GBs=round(nbytes / t["spmv"][0] / 1e6, 1)))
                # 2. the cost of asking
                assert f.factor_batch_dev(dv0.data_ptr(), nbatch) == 0
                st = {}

                def refined(dv, key):
                    def fn():
                        st[key] = f.solve_refined_batch_dev(dv.data_ptr(), wp, nvec, method="pcg", tol=TOL, max_iter=MAX_ITER)
                    return fn
                t = alternate({"refined": refined(dv0, "ask"), "solve_batch": lambda: f.solve_batch_dev(wp, nvec),
                               "solve_many_batch": lambda: f.solve_many_batch_dev(wp, nvec)}, sync, args.reps, restore)
                assert st["ask"][0] == 0 and int(st["ask"][1].max()) == 0
                emit(dict(base, what="ask", refined_ms=t["refined"], solve_batch_ms=t["solve_batch"],
                          solve_many_batch_ms=t["solve_many_batch"], launches=f.solve_refined_batch_info()["launches"]))
                # 3. moved values
                for eps, dv in dvals.items():
                    def refactor():
                        assert f.factor_batch_dev(dv.data_ptr(), nbatch) == 0
                        (f.solve_many_batch_dev if nvec >= 8 else f.solve_batch_dev)(wp, nvec)

                    def seq():
                        for b in range(nbatch):
                            f.solve_refined_dev(dv.data_ptr() + 8 * b * nnz, nnz, wp + 8 * b * nvec * n, nvec, method="pcg",
                                                tol=TOL, max_iter=MAX_ITER)
                    t = alternate({"refined": refined(dv, eps), "seq_single": seq}, sync, args.reps, restore)
                    t.update(alternate({"factor_and_solve": refactor}, sync, args.reps, restore))
                    assert f.factor_batch_dev(dv0.data_ptr(), nbatch) == 0     # (the stale factors again)
                    rc, it, err = st[eps]
                    emit(dict(base, what="moved", eps=eps, status=rc, iterations=[int(it.min()), int(it.max())],
                              max_error=float(err.max()), refined_ms=t["refined"], factor_and_solve_ms=t["factor_and_solve"],
                              seq_single_refined_ms=t["seq_single"]))
                # 4. one member iterates, the others ride along
                t = alternate({"mixed": refined(dmixed, "mixed"), "all_eps0": refined(dv0, "ask")}, sync, args.reps, restore)
                rc, it, err = st["mixed"]
                assert f.factor_batch_dev(dv0.data_ptr(), 1) == 0
                t.update(alternate({"alone": refined(dmixed, "alone")}, sync, args.reps, restore))
                assert f.factor_batch_dev(dv0.data_ptr(), nbatch) == 0
                emit(dict(base, what="mixed", status=rc, iterations_member0=[int(it[0].min()), int(it[0].max())],
                          iterations_others=int(it[1:].max()) if nbatch > 1 else 0, mixed_ms=t["mixed"],
                          all_eps0_ms=t["all_eps0"], member0_alone_ms=t["alone"]))
                # 5. the two routes of M^-1
                t = {}
                for route, env in (("solve_batch", "1000000"), ("blocked", "1")):
                    os.environ["SPLLT_BRF_BLOCKED_MIN"] = env
                    t.update(alternate({route: refined(dvals[0.02], route)}, sync, args.reps, restore))
                if args.threshold:
                    os.environ["SPLLT_BRF_BLOCKED_MIN"] = str(args.threshold)
                else:
                    del os.environ["SPLLT_BRF_BLOCKED_MIN"]
                emit(dict(base, what="route", eps=0.02, iterations=int(st["blocked"][1].max()), via_solve_batch_ms=t["solve_batch"],
                          via_blocked_ms=t["blocked"], blocked_over_solve_batch=round(t["blocked"][0] / t["solve_batch"][0], 3)))
                del src, work, ybuf
            del dv0, dvals, dmixed
        f.release_batch()
        f.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
