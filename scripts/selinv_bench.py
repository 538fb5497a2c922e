"""Time the selected inversion (spllt_hip_selected_inverse) on a named configuration: factor once,
warm up, then time selected_inverse() between device synchronisations.  Prints one JSON line.

    python scripts/selinv_bench.py [--config nd24k_like] [--steps 5] [--warmup 2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from spllt_amd import api, matgen  # noqa: E402

PEAK_FP64_MFMA = 78.6   # TFLOP/s, MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="nd24k_like")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nemin", type=int, default=32)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "selinv_bench needs a HIP device"
    A, order, cfg = matgen.build_config(args.config, args.scale)
    n, ptr, row, val = api.csc_lower_1based(A)
    f = api.Factorization(n, ptr, row, nb=cfg["nb"], nemin=args.nemin, prune_tree=False, order=order)
    f.factor(val).wait()
    factor_ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        f.factor(val).wait()
        factor_ms.append((time.perf_counter() - t0) * 1e3)
    for _ in range(args.warmup):
        f.selected_inverse()
    ms = []
    for _ in range(args.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f.selected_inverse()            # ends in a synchronisation of the engine's stream
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    b = np.zeros(n)
    b[0] = 1.0
    f.solve(b)
    t0 = time.perf_counter()
    f.solve(b)
    solve_ms = (time.perf_counter() - t0) * 1e3
    flops = f.program("selinv_flops")
    med = float(np.median(ms))
    tf = flops / (med * 1e-3) / 1e12
    fmed = float(np.median(factor_ms))
    print(json.dumps({
        "metric": "selected inversion time", "config": args.config, "n": n, "ms": round(med, 3),
        "ms_all": [round(v, 3) for v in ms], "useful_flops": flops, "tflops": round(tf, 3),
        "frac_of_fp64_mfma_peak": round(tf / PEAK_FP64_MFMA, 4), "factor_ms": round(fmed, 3),
        "ratio_to_factor": round(med / fmed, 3), "factor_flops_sym": float(f.sym_info()["flops"]),
        "one_solve_ms": round(solve_ms, 3), "n_solves_s_extrapolated": round(n * solve_ms * 1e-3, 1),
        "launches": int(len(f.program("selinv_launches")))}))
    f.close()


if __name__ == "__main__":
    main()
