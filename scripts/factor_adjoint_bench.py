"""Time the reverse-mode derivative of the factor (spllt_hip_factor_adjoint) on a named configuration: factor
once, then per sample a seed of 32 device vectors (spllt_hip_factor_adjoint_seed_dev), the sweep with its reader
(spllt_hip_factor_adjoint_dev) and, in the same process, spllt_hip_selected_inverse and the reader alone
(spllt_hip_inverse_on_pattern_dev: the same gather kernel on the other arena), each between device
synchronisations.  Prints one JSON line.

    python scripts/factor_adjoint_bench.py [--config nd24k_like] [--steps 5] [--warmup 2]
"""
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
    ap.add_argument("--config", default="nd24k_like")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nemin", type=int, default=32)
    ap.add_argument("--nvec", type=int, default=32)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "factor_adjoint_bench needs a HIP device"
    A, order, cfg = matgen.build_config(args.config, args.scale)
    n, ptr, row, val = api.csc_lower_1based(A)
    f = api.Factorization(n, ptr, row, nb=cfg["nb"], nemin=args.nemin, prune_tree=False, order=order)
    f.factor(val).wait()
    gen = torch.Generator(device="cuda").manual_seed(1)
    a = torch.randn((args.nvec, n), dtype=torch.float64, device="cuda", generator=gen)
    b = torch.randn((args.nvec, n), dtype=torch.float64, device="cuda", generator=gen)
    gval = torch.empty(f.nnz, dtype=torch.float64, device="cuda")
    pat = torch.empty(f.nnz, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()

    def timed(call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()                              # every call ends in a synchronisation of the engine's stream
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    seed = lambda: f.factor_adjoint_seed_dev(a.data_ptr(), b.data_ptr(), args.nvec, ld=n, alpha=0.5)  # noqa: E731
    sweep = lambda: f.factor_adjoint_dev(gval.data_ptr())                                            # noqa: E731
    ms = {"seed": [], "sweep_and_reader": [], "selected_inverse": [], "reader": []}
    for it in range(args.warmup + args.steps):
        t = {"seed": timed(seed), "sweep_and_reader": timed(sweep), "selected_inverse": timed(f.selected_inverse),
             "reader": timed(lambda: f.inverse_on_pattern_dev(pat.data_ptr()))}
        if it >= args.warmup:
            for k, v in t.items():
                ms[k].append(v)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    # the seed of log det A against (2 - delta) (A^-1) from the selected inverse, on the entries of A
    check = None
    if f.sym_info()["arena"] <= 3e8:
        L = f.get_factor()
        lbar = np.zeros_like(L)
        d = f.program("selinv_diag")
        lbar[d] = 2.0 / L[d]
        f.set_factor_adjoint(lbar)
        g = f.factor_adjoint()
        prow, pcol = f.pattern_tables()
        want = np.where(prow == pcol, 1.0, 2.0) * f.inverse_on_pattern()
        check = float(np.abs(g - want).max() / np.abs(want).max())
    sweep_ms = med["sweep_and_reader"] - med["reader"]
    flops = f.program("selinv_flops")
    print(json.dumps({
        "metric": "factor adjoint time", "config": args.config, "n": n, "nnz": int(f.nnz),
        "arena_GB": round(f.sym_info()["arena"] * 8 / 1e9, 3), "nvec": args.nvec,
        "seed_ms": round(med["seed"], 3), "sweep_and_reader_ms": round(med["sweep_and_reader"], 3),
        "reader_ms": round(med["reader"], 3), "sweep_ms": round(sweep_ms, 3),
        "selected_inverse_ms": round(med["selected_inverse"], 3),
        "sweep_to_selected_inverse": round(sweep_ms / med["selected_inverse"], 3),
        "ms_all": {k: [round(x, 3) for x in v] for k, v in ms.items()},
        "selinv_useful_flops": flops, "launches": int(len(f.program("selinv_launches"))),
        "logdet_seed_rel_err_on_pattern": check}))
    f.close()


if __name__ == "__main__":
    main()
