#!/usr/bin/env python3
"""Times the hard linear constraints (include/spllt_hip_constrain.h) beside the same operations composed from the
calls a user had before plus torch.matmul / torch.linalg on the device.

  constrain_bench.py [config ...] [--k 1,8,64] [--nvec 1,32,128] [--reps 5] [--warmup 2] [--inner 10] [--no-var]

Default configurations: the bench workload (nd24k_like) and poisson3d_128.  Method of factor_mult_bench.py: device
vectors in user order, the operations alternating in one process; one timed sample is --inner calls in a row, each of
which returns after its stream has drained (host clock around synchronised work; where a library call follows torch
operations on the same vectors the composition synchronises in between, as a caller has to); warm-ups first, median
and minimum of --reps samples, per call.  Two yardsticks beside every number of ours:

  torch    set: W = solve_many_dev(C), S = C W^T, torch.linalg.cholesky, solve_triangular; constrain: r = C X^T - e,
           solve_triangular, X -= t^T U^T; solve / sample: solve_many_dev / sample_dev in front of that; variances:
           inverse_diag() minus (U * U).sum on the device
  traffic  the model (3 nvec + 2 k) 8 n bytes of one constrain (X read by the product, read and written by the
           correction, C and U read once), as achieved GB/s

Checked at the timed size before timing: ours against the torch composition.  Needs a GPU: there is no fall-back."""
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
    ap.add_argument("--k", default="1,8,64")
    ap.add_argument("--nvec", default="1,32,128")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--no-var", action="store_true", help="skip inverse_diag_constrained (no selected inversion)")
    args = ap.parse_args()
    if args.reps < 5:
        sys.exit("--reps must be at least 5")
    import torch
    if not torch.cuda.is_available():
        sys.exit("constrain_bench.py needs a GPU")

    def timed(ops, reset):
        t = {name: [] for name in ops}
        for it in range(args.warmup + args.reps):
            for name, op in ops.items():
                reset()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.inner):
                    op()
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) / args.inner
                if it >= args.warmup:
                    t[name].append(dt)
        return {name: [round(float(np.median(v)) * 1e3, 4), round(min(v) * 1e3, 4)] for name, v in t.items()}   # median, minimum

    for config in args.configs:
        A, order, cfg = matgen.build_config(config, args.scale)
        n, ptr, row, val = api.csc_lower_1based(A)
        f = api.Factorization(n, ptr, row, nb=cfg["nb"], nemin=32, prune_tree=False, order=order)
        f.factor(val).wait()
        have_var = not args.no_var
        if have_var:
            f.selected_inverse()
        print(json.dumps({"config": config, "n": n, "nb": cfg["nb"], "arena_GB": round(8 * int(f.sym_info()["arena"]) / 1e9, 3)}),
              flush=True)
        gen = torch.Generator(device="cuda").manual_seed(0)
        for k in [int(s) for s in args.k.split(",")]:
            Ct = torch.randn((k, n), dtype=torch.float64, device="cuda", generator=gen)
            Ct[0] = 1.0
            e = torch.randn(k, dtype=torch.float64, device="cuda", generator=gen)
            st = {}

            def torch_set():
                W = Ct.clone()
                torch.cuda.synchronize()          # (the library works on its own stream)
                f.solve_many_dev(W.data_ptr(), k)
                S = Ct @ W.t()
                st["G"] = torch.linalg.cholesky(S)
                st["Ut"] = torch.linalg.solve_triangular(st["G"], W, upper=False)     # (k, n) = U^T

            def torch_correct(X):
                r = Ct @ X.t() - e[:, None]
                t = torch.linalg.solve_triangular(st["G"], r, upper=False)
                X -= t.t() @ st["Ut"]

            def torch_var():
                d = torch.as_tensor(f.inverse_diag(), device="cuda") - (st["Ut"] * st["Ut"]).sum(0)
                return d.cpu().numpy()

            torch_set()
            f.set_constraints_dev(Ct.data_ptr(), k)
            info = f.constraints_info()
            rec = {"config": config, "k": k, "device_MB": round(info["device_bytes"] / 1e6, 1),
                   "min_relative_pivot": info["min_relative_pivot"],
                   "log_det_s_vs_torch": abs(info["log_det_s"] - 2.0 * float(torch.log(torch.diagonal(st["G"])).sum()))}
            ops = {"set_constraints": lambda: f.set_constraints_dev(Ct.data_ptr(), k), "set_constraints_torch": torch_set}
            if have_var:
                v = f.inverse_diag_constrained()
                rec["max|var - torch|/max|var|"] = float(np.abs(v - torch_var()).max() / np.abs(v).max())
                ops["inverse_diag_constrained"] = f.inverse_diag_constrained
                ops["inverse_diag_constrained_torch"] = torch_var
            for name, tm in timed(ops, lambda: None).items():
                rec[name + "_ms"] = tm
            print(json.dumps(rec), flush=True)
            for nvec in [int(s) for s in args.nvec.split(",")]:
                src = torch.randn((nvec, n), dtype=torch.float64, device="cuda", generator=gen)
                work = torch.empty_like(src)
                ep = e.data_ptr()

                def then_correct(first):
                    first()
                    torch_correct(work)
                    torch.cuda.synchronize()      # (the next library call reads what torch has enqueued)

                ops = {
                    "constrain": lambda: f.constrain_dev(work.data_ptr(), nvec, e_dev_ptr=ep),
                    "constrain_torch": lambda: torch_correct(work),
                    "solve_constrained": lambda: f.constrain_dev(work.data_ptr(), nvec, e_dev_ptr=ep, entry="solve_constrained"),
                    "solve_constrained_torch": lambda: then_correct(lambda: f.solve_many_dev(work.data_ptr(), nvec)),
                    "sample_constrained": lambda: f.sample_constrained_dev(work.data_ptr(), nvec, seed=1, e_dev_ptr=ep),
                    "sample_constrained_torch": lambda: then_correct(lambda: f.sample_dev(work.data_ptr(), nvec, seed=1)),
                    "solve_many_job0": lambda: f.solve_many_dev(work.data_ptr(), nvec),
                }
                # results at the timed size: ours against the composition, and the constraint itself
                work.copy_(src)
                torch.cuda.synchronize()
                ops["constrain"]()
                ours = work.clone()
                work.copy_(src)
                ops["constrain_torch"]()
                scale = float(work.abs().max())
                rec = {"config": config, "k": k, "nvec": nvec, "inner": args.inner,
                       "max|ours - torch|/max|x|": float((ours - work).abs().max()) / scale,
                       "max|C x - e|": float((Ct @ ours.t() - e[:, None]).abs().max())}
                tm = timed(ops, lambda: work.copy_(src))
                for name, v in tm.items():
                    rec[name + "_ms"] = v
                model = (3 * nvec + 2 * k) * 8 * n
                rec["constrain_model_MB"] = round(model / 1e6, 1)
                rec["constrain_GBps"] = round(model / (tm["constrain"][0] * 1e-3) / 1e9, 1)
                rec["constrain_torch_GBps"] = round(model / (tm["constrain_torch"][0] * 1e-3) / 1e9, 1)
                print(json.dumps(rec), flush=True)
        f.close()


if __name__ == "__main__":
    main()
