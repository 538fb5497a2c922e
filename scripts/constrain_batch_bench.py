#!/usr/bin/env python3
"""Times the hard linear constraints of a batch (include/spllt_hip_constrain_batch.h) against the same work done by
sequential calls on the single handle.  Per (config, nbatch, k, vectors per member), one JSON line:

  build     spllt_hip_set_constraints_batch_dev: C into every member's slot, the blocked batch solve of k columns
            per member, three launches -- all members in every launch
  correct   spllt_hip_constrain_batch_dev on resident vectors: three launches per pass of 32 vectors per member
  solve     spllt_hip_solve_constrained_batch_dev: the blocked batch solve, then the correction
  seq_*     what a user does without this family: per member spllt_hip_factor_dev + wait (not timed: the batch side's
            spllt_hip_factor_batch_dev is not timed either), then spllt_hip_set_constraints_dev (seq_build) and
            spllt_hip_constrain_dev (seq_correct) or spllt_hip_solve_constrained_dev (seq_solve) on that member's
            vectors.  The single handle holds ONE factor, so the sequential side has to factorize between members;
            only the calls named here are inside its clock, summed over the members.

  constrain_batch_bench.py [--configs poisson2d_128,nd24k_like] [--nbatch 4,16,64] [--k 1,8,64] [--nvec 1,32]
                           [--reps 5] [--max-gb 40] [--out FILE]

nd24k_like runs nbatch 4 and 16 only.  Members: A0 scaled by 1 + b / nbatch.  Vectors resident in HBM and restored
before every call; a host clock around calls that end in a synchronise; median and (min, max) of --reps calls after
one warm-up call of each kind.  Needs a GPU: there is no fall-back."""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spllt_amd import api, matgen  # noqa: E402


def chunks_of(n):
    """the chunks of n positions the partial sums are stored by (cn_chunk in constrain.hip)"""
    per = -(-n // 256)
    chunk = max(64, 64 * -(-per // 64))
    return -(-n // chunk)


def stats(v):
    return [round(float(np.median(v)) * 1e3, 3), round(min(v) * 1e3, 3), round(max(v) * 1e3, 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="poisson2d_128,nd24k_like")
    ap.add_argument("--nbatch", default="4,16,64")
    ap.add_argument("--k", default="1,8,64")
    ap.add_argument("--nvec", default="1,32")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--max-gb", type=float, default=40.0, help="skip a batch whose storage would exceed this")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("constrain_batch_bench.py needs a GPU")
    sync = torch.cuda.synchronize
    out = open(args.out, "a") if args.out else None

    def emit(obj):
        line = obj if isinstance(obj, str) else json.dumps(obj)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    def timed(fn, before, reps):
        t = []
        for it in range(reps + 1):
            before()
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            if it:
                t.append(time.perf_counter() - t0)
        return t

    ks = [int(s) for s in args.k.split(",")]
    nvecs = [int(s) for s in args.nvec.split(",")]
    for config in args.configs.split(","):
        A, order, cfg = matgen.build_config(config, args.scale)
        A0 = sp.csc_matrix(A)
        A0 = A0 / abs(A0).sum(axis=0).max()
        n, ptr, row, val0 = api.csc_lower_1based(A0)
        f = api.Factorization(n, ptr, row, nb=cfg["nb"], nemin=32, prune_tree=False, order=order)
        nnz, arena = f.nnz, int(f.sym_info()["arena"])
        nchunks = chunks_of(n)
        # arena + values + U at k = 64 + the partial sums + the vectors and their copy at 32 per member
        per_member_gb = 8.0 * (arena + nnz + 64 * n + nchunks * 4096 + 2 * 32 * n + 32 * n) / 1e9
        cap = 16 if config == "nd24k_like" else 1 << 30
        sizes = [b for b in (int(s) for s in args.nbatch.split(",")) if b <= cap and b * per_member_gb <= args.max_gb]
        emit(f"# {config}: n={n} nnz={nnz} arena={arena} chunks={nchunks} member storage={per_member_gb:.3f} GB "
             f"sizes={sizes} k={ks} nvec={nvecs} reps={args.reps}")
        rng = np.random.default_rng(0)
        for nbatch in sizes:
            scales = 1.0 + np.arange(nbatch) / nbatch
            dvals = torch.tensor((scales[:, None] * val0[None, :]).ravel(), device="cuda")
            assert f.factor_batch_dev(dvals.data_ptr(), nbatch) == 0
            for k in ks:
                Crows = rng.standard_normal((k, n))
                Crows[0] = 1.0
                dC = torch.tensor(Crows, device="cuda")
                nothing = lambda: None   # noqa: E731
                t_build = timed(lambda: f.set_constraints_batch_dev(dC.data_ptr(), k), nothing, args.reps)
                # sequential: per member factor (outside the clock), then set_constraints_dev (inside)
                t_seq_build = np.zeros(args.reps)
                for b in range(nbatch):
                    f.factor_dev(dvals.data_ptr() + 8 * b * nnz)
                    f.wait()
                    t_seq_build += np.array(timed(lambda: f.set_constraints_dev(dC.data_ptr(), k), nothing, args.reps))
                emit(dict(config=config, nbatch=nbatch, k=k, what="build", batch_ms=stats(t_build),
                          seq_ms=stats(list(t_seq_build)), seq_over_batch=round(float(np.median(t_seq_build) / np.median(t_build)), 3),
                          launches=f.constraints_batch_info()["launches"]))
                for nvec in nvecs:
                    src = torch.tensor(rng.standard_normal((nbatch, nvec, n)), device="cuda")
                    work = torch.empty_like(src)
                    wp = work.data_ptr()
                    restore = lambda: work.copy_(src)   # noqa: E731
                    res = {}
                    for what, entry in (("correct", "constrain"), ("solve", "solve_constrained")):
                        res[what] = timed(lambda: f.constrain_batch_dev(wp, nvec, entry=entry), restore, args.reps)
                    launches = f.constraints_batch_info()["launches"]
                    seq = {"correct": np.zeros(args.reps), "solve": np.zeros(args.reps)}
                    for b in range(nbatch):
                        f.factor_dev(dvals.data_ptr() + 8 * b * nnz)
                        f.wait()
                        f.constrain_dev(wp, nvec)      # (picks the new factor up: the rebuild stays outside the clock)
                        for what, entry in (("correct", "constrain"), ("solve", "solve_constrained")):
                            seq[what] += np.array(timed(lambda: f.constrain_dev(wp + 8 * b * nvec * n, nvec, entry=entry),
                                                        restore, args.reps))
                    for what in ("correct", "solve"):
                        emit(dict(config=config, nbatch=nbatch, k=k, nvec=nvec, what=what, batch_ms=stats(res[what]),
                                  seq_ms=stats(list(seq[what])),
                                  seq_over_batch=round(float(np.median(seq[what]) / np.median(res[what])), 3),
                                  launches_per_pass=launches))
                    del src, work
                f.release_constraints()
                f.release_constraints_batch()
            del dvals
        f.release_batch()
        f.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
