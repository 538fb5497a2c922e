#!/usr/bin/env python3
"""Times the batched selected inversion (spllt_hip_selected_inverse_batch) with the fused small-step
kernel on and off, against the same work as single-handle inversions one after the other
(spllt_hip_selected_inverse, nbatch calls on a factor of the same pattern), with the batched
factorization of the same members beside it.

  selinv_batch_bench.py [--problems poisson2d_128,nd_like_24] [--nbatch 1,8,64,256] [--reps 5] [--warmup 2]
                        [--max-gb 24] [--out profiles/selinv_batch]

A host clock around calls that end in a synchronise, the three inversions alternating in one process,
warm-ups first, median of --reps.  Members: A_b = D_b A D_b, D_b uniform in [0.5, 2] (seed 100 + b).  At
every size one member's Z is checked against the single-handle inverse of the same member (2e-11: each is
within 1e-11 of the dense inverse by the test-suite's bar) and the fused form against the unfused one
(1e-13).  One JSON line per (problem, nbatch), also appended to <out>/<problem>.jsonl.  nb = 256,
nemin = 32 (BASELINE config 1 for poisson2d_128).  Needs a GPU: there is no fall-back."""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spllt_amd import api, matgen  # noqa: E402

PROBLEMS = {"poisson2d_128": lambda: matgen.poisson2d(128), "nd_like_24": lambda: matgen.nd_like((24, 24, 23), 3),
            "poisson2d_40": lambda: matgen.poisson2d(40)}


def member_values(A, b):
    d = np.random.default_rng(100 + b).uniform(0.5, 2.0, A.shape[0])
    D = sp.diags(d)
    return api.csc_lower_1based(sp.csc_matrix(D @ A @ D))[3]


def lower_mask(f):
    mask = np.zeros(f.sym_info()["arena"], dtype=bool)
    for off, w, nr in zip(f.sym("bcol_off"), f.sym("bcol_width"), f.sym("bcol_nrow")):
        m = np.ones((int(nr), int(w)), dtype=bool)
        m[:w, :w] = np.tril(m[:w, :w])
        mask[int(off):int(off) + int(nr) * int(w)] = m.ravel()
    return mask


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", default="poisson2d_128,nd_like_24")
    ap.add_argument("--nbatch", default="1,8,64,256")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--max-gb", type=float, default=24.0, help="skip a batch whose storage would exceed this")
    ap.add_argument("--out", default=os.path.join("profiles", "selinv_batch"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("selinv_batch_bench.py needs a GPU")
    sync = torch.cuda.synchronize
    os.makedirs(args.out, exist_ok=True)
    for pname in args.problems.split(","):
        A = sp.csc_matrix(PROBLEMS[pname]())
        n, ptr, row, val = api.csc_lower_1based(A)
        f = api.Factorization(n, ptr, row, nb=256, nemin=32)
        info = f.sym_info()
        arena, nnz = int(info["arena"]), f.nnz
        units, launches = f.program("batch_selinv_units"), f.program("batch_selinv_launches")
        steps = int((launches[:, 0] == 2).sum())
        fusable = 0
        for kind, _, first, count, _ in launches:
            if kind == 2 and count > 0:
                u = units[first:first + count]
                fusable += int((u["nR"] <= 64).all() and (u["nsplit"] <= 1).all())
        per_member_gb = 8.0 * (2 * arena + f.program("batch_dinv_size") + f.program("batch_selinv_scratch") + nnz) / 1e9
        sizes = [b for b in (int(s) for s in args.nbatch.split(",")) if b * per_member_gb <= args.max_gb]
        print(f"# {pname}: n={n} nnz={nnz} arena={arena} selinv steps={steps} (fusable {fusable}) "
              f"selinv flops={f.program('batch_selinv_flops'):.3e} per member {per_member_gb:.4f} GB", flush=True)
        if not sizes:
            f.close()
            continue
        nmax = max(sizes)
        vals = np.stack([member_values(A, b) for b in range(min(nmax, 64))])
        vals = vals[np.arange(nmax) % len(vals)]          # (beyond 64 the members repeat: the values only feed the timing)
        dv = torch.tensor(vals.ravel(), device="cuda")
        sync()
        mask = lower_mask(f)
        f.factor(vals[0]).wait()                          # the single-handle factor: member 0
        f.selected_inverse()
        Zsingle = f.get_inverse().copy()
        log = open(os.path.join(args.out, pname + ".jsonl"), "a")
        for nbatch in sizes:
            def fac():
                assert f.factor_batch_dev(dv.data_ptr(), nbatch) == 0

            def seq():
                for _ in range(nbatch):
                    f.selected_inverse()

            def bat():
                assert f.selected_inverse_batch() == 0

            def hook(on):
                assert f.lib.spllt_hip_debug(b"batch_selinv_fused=1" if on else b"batch_selinv_fused=0") == 0
            fac()
            t = {"factor": [], "seq": [], "fused": [], "unfused": []}
            nl = {}
            for it in range(args.warmup + args.reps):
                for which in ("factor", "seq", "fused", "unfused"):
                    if which in ("fused", "unfused"):
                        hook(which == "fused")
                    fn = {"factor": fac, "seq": seq}.get(which, bat)
                    sync()
                    t0 = time.perf_counter()
                    fn()
                    dt = time.perf_counter() - t0
                    if which in ("fused", "unfused"):
                        nl[which] = f.batch_selinv_launches()
                    if which == "factor":
                        bat()                             # (the factorization made Z stale: keep the pairs alike)
                    if it >= args.warmup:
                        t[which].append(dt)
            hook(False)
            bat()
            Zu = f.get_inverse_batch(0).copy()
            hook(True)
            bat()
            Zf = f.get_inverse_batch(0)
            scale = np.abs(Zsingle[mask]).max()
            e_single = float(np.abs(Zf - Zsingle)[mask].max() / scale)
            e_forms = float(np.abs(Zf - Zu)[mask].max() / scale)
            assert e_single <= 2e-11 and e_forms <= 1e-13, (e_single, e_forms)
            med = {k: float(np.median(v)) for k, v in t.items()}
            rec = {"problem": pname, "nbatch": nbatch,
                   "factor_batch_ms": round(med["factor"] * 1e3, 3),
                   "seq_ms": round(med["seq"] * 1e3, 3), "fused_ms": round(med["fused"] * 1e3, 3),
                   "unfused_ms": round(med["unfused"] * 1e3, 3),
                   "seq_ms_per_member": round(med["seq"] / nbatch * 1e3, 4),
                   "fused_ms_per_member": round(med["fused"] / nbatch * 1e3, 4),
                   "unfused_ms_per_member": round(med["unfused"] / nbatch * 1e3, 4),
                   "seq_over_fused": round(med["seq"] / med["fused"], 2),
                   "unfused_over_fused": round(med["unfused"] / med["fused"], 3),
                   "launches_fused": nl["fused"], "launches_unfused": nl["unfused"],
                   "launches_seq": nbatch * int((f.program("selinv_launches")[:, 3] > 0).sum()),
                   "raw_ms": {k: [round(x * 1e3, 3) for x in v] for k, v in t.items()},
                   "rel_err_vs_single": e_single, "rel_err_fused_vs_unfused": e_forms}
            line = json.dumps(rec)
            print(line, flush=True)
            log.write(line + "\n")
            log.flush()
        log.close()
        f.close()


if __name__ == "__main__":
    main()
