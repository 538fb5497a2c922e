#!/usr/bin/env python3
"""Times the factor adjoint of a batch (include/spllt_hip_batch_adjoint.h) and its yardsticks in the same run:

  seed32      spllt_hip_factor_adjoint_seed_batch_dev with 32 vectors per member
  fused       one re-seed with ONE vector per member (a sweep wants freshly seeded arenas) + the sweep and its
              reader, fused steps on (spllt_hip_debug "batch_fadj_fused=1")
  unfused     the same with every step in its three-launch form ("batch_fadj_fused=0")
  reseed      the re-seed with one vector alone: what the two lines above contain besides the sweep
  selinv      spllt_hip_selected_inverse_batch on the same batch: the same program, the inversion's kernels
  seq         nbatch times (seed of 32 vectors + sweep + reader) of the single handle one after the other on ONE
              arena: what a caller had before this family (the time does not depend on the values)

  factor_adjoint_batch_bench.py [--configs poisson2d_128,nd24k_like] [--nbatch 1,4,16,64] [--reps 10] [--warmup 2]
                                [--max-gb 24] [--out FILE]

The method of selinv_batch_bench.py / solve_many_batch_bench.py: everything resident in HBM, a host clock around
calls that end in a synchronise, all sides alternating in one process, warm-ups first, median and spread (min ..
max) of --reps windows; a timed window repeats its call until it holds at least 2 ms.  Members: A_b = (1 + 0.01 b)
A / ||A||_1.  At every size the fused and the unfused sweep are compared (relative difference on the pattern, in
the output) before anything is timed.  One JSON line per (config, nbatch); --out appends the lines to a file as
well.  --nbatch is cut by --max-gb (three arenas and the step scratch per member: nd24k_like, 5.07 GB per member,
runs at 1 and 4 members under the default 24 GB) and, for nd24k_like, at 16.  Needs a GPU: there is no fall-back."""
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


def ms(t):
    return round(t[0] * 1e3, 4), [round(t[1] * 1e3, 4), round(t[2] * 1e3, 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="poisson2d_128,nd24k_like")
    ap.add_argument("--nbatch", default="1,4,16,64")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--max-gb", type=float, default=24.0, help="skip a batch whose storage would exceed this")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 10:
        sys.exit("--reps must be at least 10")
    import torch
    if not torch.cuda.is_available():
        sys.exit("factor_adjoint_batch_bench.py needs a GPU")
    sync = torch.cuda.synchronize
    out = open(args.out, "a") if args.out else None
    nvec = 32

    def emit(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    def hook(on):
        assert api._lib.load().spllt_hip_debug(b"batch_fadj_fused=1" if on else b"batch_fadj_fused=0") == 0

    for config in args.configs.split(","):
        A, order, cfg = matgen.build_config(config, args.scale)
        A = sp.csc_matrix(A)
        A = A / abs(A).sum(axis=0).max()
        n, ptr, row, val = api.csc_lower_1based(A)
        f = api.Factorization(n, ptr, row, nb=cfg["nb"], nemin=32, prune_tree=False, order=order)
        arena, nnz = int(f.sym_info()["arena"]), f.nnz
        scratch = int(f.program("batch_selinv_scratch"))
        # L, G and Z arenas, dinv, step scratch, values and gradients, the seed vectors
        per_member_gb = 8.0 * (3 * arena + f.program("batch_dinv_size") + scratch + 2 * nnz + 2 * nvec * n) / 1e9
        cap = 16 if config == "nd24k_like" else 1 << 30
        sizes = [b for b in (int(s) for s in args.nbatch.split(",")) if b * per_member_gb <= args.max_gb and b <= cap]
        emit(f"# {config}: n={n} nnz={nnz} arena={arena} member storage={per_member_gb:.3f} GB sizes={sizes}")
        if not sizes:
            f.close()
            continue
        f.factor(val).wait()
        nmax = max(sizes)
        dv = torch.tensor(np.stack([(1 + 0.01 * b) * val for b in range(nmax)]).ravel(), device="cuda")
        rng = np.random.default_rng(0)
        for nbatch in sizes:
            assert f.factor_batch_dev(dv.data_ptr(), nbatch) == 0
            a = torch.tensor(rng.standard_normal((nbatch, nvec, n)), device="cuda")
            b = torch.tensor(rng.standard_normal((nbatch, nvec, n)), device="cuda")
            a1, b1 = a[:, :1].contiguous(), b[:, :1].contiguous()
            g = torch.empty((nbatch, nnz), dtype=torch.float64, device="cuda")
            g1 = torch.empty(nnz, dtype=torch.float64, device="cuda")
            sync()
            ap_, bp_, a1p, b1p, gp, g1p = (t.data_ptr() for t in (a, b, a1, b1, g, g1))

            def seed32():
                f.factor_adjoint_seed_batch_dev(ap_, bp_, nvec)

            def reseed():
                f.factor_adjoint_seed_batch_dev(a1p, b1p, 1)

            def sweep():
                reseed()
                f.factor_adjoint_batch_dev(gp)

            def form(on):
                def fn():
                    hook(on)
                    try:
                        return timed(sweep, sync)
                    finally:
                        hook(False)
                return fn

            def selinv():
                f.selected_inverse_batch()

            def seq():
                for m in range(nbatch):
                    f.factor_adjoint_seed_dev(ap_ + 8 * m * nvec * n, bp_ + 8 * m * nvec * n, nvec)
                    f.factor_adjoint_dev(g1p)

            # the two forms give the same gradient
            res = {}
            for on in (True, False):
                hook(on)
                seed32()
                f.factor_adjoint_batch_dev(gp)
                res[on] = (g.cpu().numpy().copy(), f.batch_adjoint_launches())
            hook(False)
            diff = float(np.abs(res[True][0] - res[False][0]).max() / np.abs(res[False][0]).max())
            assert diff <= 1e-12, diff
            t = {k: [] for k in ("seed32", "reseed", "fused", "unfused", "selinv", "seq")}
            runs = {"seed32": lambda: timed(seed32, sync), "reseed": lambda: timed(reseed, sync), "fused": form(True),
                    "unfused": form(False), "selinv": lambda: timed(selinv, sync), "seq": lambda: timed(seq, sync)}
            for it in range(args.warmup + args.reps):
                for which, run in runs.items():
                    dt = run()
                    if it >= args.warmup:
                        t[which].append(dt)
            st = {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in t.items()}
            line = {"config": config, "nbatch": nbatch, "nvec": nvec, "launches_fused": res[True][1],
                    "launches_unfused": res[False][1], "fused_vs_unfused_rel_diff": diff}
            for k, v in st.items():
                line[k + "_ms"], line[k + "_ms_min_max"] = ms(v)
            sw_f, sw_u = st["fused"][0] - st["reseed"][0], st["unfused"][0] - st["reseed"][0]
            line["sweep_fused_ms"], line["sweep_unfused_ms"] = round(sw_f * 1e3, 4), round(sw_u * 1e3, 4)
            line["unfused_over_fused"] = round(st["unfused"][0] / st["fused"][0], 3)
            line["seq_over_batch"] = round(st["seq"][0] / (st["seed32"][0] + sw_f), 2)
            emit(json.dumps(line))
            del a, b, g
        f.release_batch()
        f.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
