#!/usr/bin/env python3
"""Times the bit-reproducible batch (spllt_hip_set_batch_reproducible) against the default
batch of the same build, switch off and on taking turns in one process:

  factor         spllt_hip_factor_batch_dev: the deterministic program (buffered products + ordered gathers) against
                 the default one (atomic scatter)
  solve<nrhs>    spllt_hip_solve_many_batch_dev, job 0, 8 and 32 right-hand sides per member: stored strips + ordered
                 gathers against atomic strips
  constraints    spllt_hip_set_constraints_batch_dev with k rows: W_b by the blocked solve either way, so the same
                 difference seen through the constrained family

  batch_repro_bench.py [--configs poisson2d_128:4,poisson2d_128:16,poisson2d_128:64,nd24k_like:4] [--nrhs 8,32]
                       [--k 8] [--samples 5] [--calls 10] [--scale 1.0] [--out FILE]

Method: values and vectors resident in HBM, a host clock around --calls calls that end in a synchronise, one warm-up
sample per side first, then --samples samples per side, the sides alternating; median and spread (min .. max) per
call.  Members: A_b = (1 + 0.01 b) A / ||A||_1.  With the switch on the factors are those of the deterministic program
(the batch is factorized again after every flip, outside the timed windows, except where the factorization itself
is timed).  At every size the reproducible results are checked against the default ones (1e-10 of the largest entry)
and for bit-equality between two runs.  One JSON line per (config, nbatch, what); --out appends the lines to a file as
well.  Needs a GPU: there is no fall-back."""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spllt_amd import api, matgen  # noqa: E402


def sample(fn, sync, calls):
    """seconds per call of one sample of `calls` calls"""
    sync()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    sync()
    return (time.perf_counter() - t0) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="poisson2d_128:4,poisson2d_128:16,poisson2d_128:64,nd24k_like:4")
    ap.add_argument("--nrhs", default="8,32")
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("batch_repro_bench.py needs a GPU")
    sync = torch.cuda.synchronize
    out = open(args.out, "a") if args.out else None

    def emit(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    rhs = [int(s) for s in args.nrhs.split(",")]
    built = {}
    for item in args.configs.split(","):
        config, nbatch = item.split(":")
        nbatch = int(nbatch)
        if config not in built:
            A, order, cfg = matgen.build_config(config, args.scale)
            A = sp.csc_matrix(A)
            A = A / abs(A).sum(axis=0).max()
            n, ptr, row, val = api.csc_lower_1based(A)
            built[config] = (api.Factorization(n, ptr, row, nb=cfg["nb"], nemin=32, prune_tree=False, order=order), val)
        f, val = built[config]
        n = f.n
        dv = torch.tensor(np.stack([(1 + 0.01 * b) * val for b in range(nbatch)]).ravel(), device="cuda")
        rng = np.random.default_rng(0)
        Crows = torch.tensor(rng.standard_normal((args.k, n)), device="cuda")
        emit(f"# {config}: n={n} nnz={f.nnz} arena={int(f.sym_info()['arena'])} nbatch={nbatch} "
             f"factor scratch per member={f.program('batch_det_scratch_size')} doubles, sweep slots="
             f"{max(f.program('batch_rsolve_frows'), f.program('batch_rsolve_bsize'))}")

        def switch(on):
            f.set_batch_reproducible(on)
            assert f.factor_batch_dev(dv.data_ptr(), nbatch) == 0

        def measure(what, fn, prepare=lambda: None, extra=None):
            """fn timed with the switch off and on in turns; prepare() runs before every sample, untimed"""
            t = {False: [], True: []}
            for it in range(1 + args.samples):
                for on in (False, True):
                    switch(on)
                    prepare()
                    dt = sample(fn, sync, args.calls)
                    if it > 0:
                        t[on].append(dt)
            med = {on: float(np.median(v)) for on, v in t.items()}
            line = {"config": config, "nbatch": nbatch, "what": what,
                    "off_ms": round(med[False] * 1e3, 4),
                    "off_ms_min_max": [round(min(t[False]) * 1e3, 4), round(max(t[False]) * 1e3, 4)],
                    "on_ms": round(med[True] * 1e3, 4),
                    "on_ms_min_max": [round(min(t[True]) * 1e3, 4), round(max(t[True]) * 1e3, 4)],
                    "on_over_off": round(med[True] / med[False], 3)}
            line.update(extra or {})
            emit(json.dumps(line))

        # parity and repeatability of the factors
        switch(False)
        ld0 = f.log_det_batch()
        switch(True)
        ld1, a1 = f.log_det_batch(), f.get_factor_batch(nbatch - 1)
        switch(True)
        assert f.log_det_batch().tobytes() == ld1.tobytes() and f.get_factor_batch(nbatch - 1).tobytes() == a1.tobytes()
        assert np.abs(ld1 - ld0).max() <= 1e-10 * np.abs(ld0).max()
        info = f.batch_repro_info()
        measure("factor", lambda: f.factor_batch_dev(dv.data_ptr(), nbatch),
                extra={"launches_on": info["factor_launches"], "factor_scratch_bytes": info["factor_scratch_bytes"]})
        for nrhs in rhs:
            src = torch.tensor(rng.standard_normal((nbatch, nrhs, n)), device="cuda")
            work = torch.empty_like(src)
            res = {}
            for on in (False, True, True):
                switch(on)
                work.copy_(src)
                sync()
                f.solve_many_batch_dev(work.data_ptr(), nrhs, job=0)
                got = work.cpu().numpy()
                if on in res:
                    assert res[on].tobytes() == got.tobytes(), "the reproducible sweep did not repeat"
                res[on] = got
            perr = float(np.abs(res[True] - res[False]).max() / np.abs(res[False]).max())
            assert perr <= 1e-10, perr
            measure(f"solve{nrhs}", lambda: f.solve_many_batch_dev(work.data_ptr(), nrhs, job=0),
                    prepare=lambda: work.copy_(src),
                    extra={"parity_rel_err": perr, "sweep_scratch_bytes": f.batch_repro_info()["sweep_scratch_bytes"]})
            del src, work
        measure(f"constraints k={args.k}", lambda: f.set_constraints_batch_dev(Crows.data_ptr(), args.k))
        f.set_constraints_batch(None)
        f.set_batch_reproducible(False)
        f.release_batch()
    for f, _ in built.values():
        f.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
