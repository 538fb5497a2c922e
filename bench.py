#!/usr/bin/env python3
"""Headline benchmark: factorize GFLOP/s (fp64) of the MI355X engine.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

One "step" = one complete numerical factorization (spllt_factor -> spllt_wait,
reference timing window drivers/spllt_omp.F90:185-192) of the workload, with
`val` already resident in HBM and L left device-resident.  GFLOP/s = F_sym / t
with F_sym the reference's own symbolic flop count
(src/spllt_analyse_mod.F90:1007-1023).  Prints ONE JSON line on rank 0.

A plain single-GPU run sets up, warms up, times the K steps and prints the line
(`roofline` and `cpu_baseline` null).  --full adds everything else: drop-in
variant, accuracy check against the CPU oracle, roofline and per-launch profile,
timeline, CPU baseline, DGEMM reference, two handles in flight, the small and the
other BASELINE configurations.  --dump-outputs DIR writes the factor of the last
timed step (a fixed sample of it) as DIR/L.npy.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
# cpu_baseline leg: idle OpenMP workers sleep instead of spinning (a spinning team of 16 on
# a 16-CPU cgroup quota gets the whole process throttled; seen once as 19 s instead of 1.1 s)
os.environ.setdefault("OMP_WAIT_POLICY", "PASSIVE")

FP64_MFMA_PEAK_TFLOPS = 78.6  # MI355X vendor fp64 matrix peak (dense); see DESIGN.md


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--config", default="nd24k_like", help="matgen.CONFIGS key")
    ap.add_argument("--scale", type=float, default=1.0, help="shrink every grid edge (debug)")
    ap.add_argument("--mm", default=None, help="MatrixMarket file to use instead of the stand-in")
    ap.add_argument("--rb", default=None, help="Rutherford-Boeing file (values = 3 conditioning, like the reference drivers)")
    ap.add_argument("--no-extra-configs", action="store_true",
                    help="skip the other BASELINE configurations reported under detail.configs")
    ap.add_argument("--ordering", default="geometric", choices=["geometric", "builtin"])
    ap.add_argument("--nb", type=int, default=None)
    ap.add_argument("--panel", type=int, default=None)
    ap.add_argument("--nemin", type=int, default=32, help="supernode amalgamation threshold (reference default 32)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-threads", type=int, default=0)
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--profile-out", default=None, help="write the per-launch timing table here (needs --full)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline: check, roofline, CPU baseline and the other configurations")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write the factor computed by the last timed step to DIR/L.npy (single GPU)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.profile_out and not args.full:
        ap.error("--profile-out needs --full (the per-launch table is part of the profile)")
    return args


# entries of L that --dump-outputs writes at most: 32 MiB of float64
DUMP_ENTRIES = 1 << 22


def dump_outputs(out_dir, f):
    """What a caller of the timed path receives: the factor L (the whole arena, float64).  An arena
    of more than DUMP_ENTRIES entries is sampled at fixed positions (seed 0, sorted), so the same
    arguments dump the same entries on every run and every build."""
    os.makedirs(out_dir, exist_ok=True)
    L = f.get_factor()
    if L.size > DUMP_ENTRIES:
        L = L[np.sort(np.random.default_rng(0).integers(0, L.size, DUMP_ENTRIES))]
    np.save(os.path.join(out_dir, "L.npy"), np.ascontiguousarray(L, dtype=np.float64))


def build_workload(args):
    from spllt_amd import api, matgen
    if args.mm:
        A = matgen.make_diag_dominant(matgen.read_mtx(args.mm))
        order, cfg = None, dict(nb=args.nb or 256, gen="mtx:" + os.path.basename(args.mm))
        name = "mtx:" + os.path.basename(args.mm)
    elif args.rb:
        A = matgen.read_rb(args.rb, values=3)
        order, cfg = None, dict(nb=args.nb or 256, gen="rb:" + os.path.basename(args.rb))
        name = "rb:" + os.path.basename(args.rb)
    else:
        A, order, cfg = matgen.build_config(args.config, args.scale)
        name = args.config + ("" if args.scale == 1.0 else f"@{args.scale}")
        if args.ordering == "builtin":
            order = None
    nb = args.nb or cfg["nb"]
    n, ptr, row, val = api.csc_lower_1based(A)
    return A, n, ptr, row, val, order, nb, name, cfg


# (the 128-tile is the LDS-DMA kernel unless SPLLT_UPD_DMA=0 selects the register-staged one)
UPDATE_KERNELS = {128: "k_update<128, 16, 4, 2>" if os.environ.get("SPLLT_UPD_DMA") == "0" else "k_update_dma128",
                  64: "k_update<64, 16, 2, 2>", 32: "k_update<32, 32, 2, 2>"}


def roofline_from_profile(f, val):
    """Dominant kernel = the k_update<T,...> instantiation (fp64 MFMA GEMM with
    direct / scatter / TRSM epilogue) with the largest total time.  achieved =
    algorithmic flops of all its launches / the sum of their durations, measured live with
    HIP events on the stream each launch runs on.  Two figures:
      frac        the launches inside the real multi-stream program (beside the panel chains and
                  the other update streams): what the program gets
      frac_alone  the same launches serialized on one stream: the kernel alone on the chip"""
    # two passes, per-launch minimum: a single pass occasionally shows one launch
    # stalled by tens of ms (host/driver hiccup between its two event records)
    ms = np.minimum(f.profile(val), f.profile(val))
    ms_prog = np.minimum(f.profile(val, in_program=True), f.profile(val, in_program=True))
    L = f.program("launches")
    kinds, tiles, flops = L[:, 0], L[:, 4], L[:, 5].astype(np.float64)
    table = {"chain_ms": float(ms[kinds == 4].sum()), "chain_launches": int((kinds == 4).sum()),
             "chain_ms_in_program": float(ms_prog[kinds == 4].sum()),
             "total_ms": float(ms.sum()), "total_gflop": float(flops.sum()) / 1e9}
    per = {}
    for T in UPDATE_KERNELS:
        sel = (kinds == 1) & (tiles == T) & (L[:, 3] > 0)
        per[T] = (float(ms[sel].sum()), float(flops[sel].sum()), int(sel.sum()), float(ms_prog[sel].sum()))
        table[f"update{T}_ms"], table[f"update{T}_gflop"], table[f"update{T}_launches"] = (
            per[T][0], per[T][1] / 1e9, per[T][2])
        table[f"update{T}_tflops"] = round(per[T][1] / per[T][0] / 1e9, 2) if per[T][0] > 0 else 0.0
        table[f"update{T}_tflops_in_program"] = round(per[T][1] / per[T][3] / 1e9, 2) if per[T][3] > 0 else 0.0
    T = max(per, key=lambda t: per[t][0])
    t_s, fl, nl, t_prog = per[T][0] * 1e-3, per[T][1], per[T][2], per[T][3] * 1e-3
    ach = fl / t_s / 1e12 if t_s > 0 else 0.0
    ach_prog = fl / t_prog / 1e12 if t_prog > 0 else 0.0
    # achieved / frac: INSIDE the program (what the factorization gets from the kernel: every launch
    # bracketed by two events on its own stream, beside whatever runs on the other streams);
    # achieved_alone / frac_alone: the same launches serialized, the kernel alone on the chip
    roof = {"bound": "mfma", "kernel": UPDATE_KERNELS[T], "achieved": round(ach_prog, 3),
            "peak": FP64_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
            "frac": round(ach_prog / FP64_MFMA_PEAK_TFLOPS, 4),
            "achieved_alone": round(ach, 3),
            "frac_alone": round(ach / FP64_MFMA_PEAK_TFLOPS, 4), "traffic": None,
            "launches": nl, "avg_launch_ms": round(per[T][3] / max(nl, 1), 4),
            "avg_launch_ms_alone": round(per[T][0] / max(nl, 1), 4)}
    return roof, table, ms


PROFILE_DIRS = {"nd24k_like": "nd24k", "poisson3d_128": "p3d128", "serena_like": "serena", "flan_like": "flan"}


def attach_pmc(roof, workload):
    """HBM traffic and matrix-pipe utilisation of the dominant kernel come from separate
    rocprofv3 --pmc passes (scripts/gpu_profile.sh: FETCH_SIZE / WRITE_SIZE / MFMA busy cannot
    be read from inside this process); the committed per-launch summary of the SAME command is
    quoted when it was taken on this very workload."""
    try:
        path = os.path.join(ROOT, "profiles", "r04", PROFILE_DIRS[workload], "summary.json")
        with open(path) as fh:
            pmc = json.load(fh)
        k = pmc.get("kernels", {}).get(roof["kernel"])
        if pmc.get("workload") == workload and k:
            roof["traffic"] = round(k["hbm_bytes_per_launch"])
            roof["traffic_unit"] = ("bytes per launch (rocprofv3 PMC: 2*FETCH_SIZE + WRITE_SIZE, "
                                    f"profiles/r04/{PROFILE_DIRS[workload]}/summary.json)")
            roof["algorithmic_bytes_per_launch"] = round(k["algorithmic_bytes_per_launch"])
            if k.get("mfma_util_percent") is not None:
                roof["mfma_util_percent"] = round(k["mfma_util_percent"], 1)
    except (OSError, ValueError, KeyError):
        pass


def run_extra_config(cfg_name, steps=2):
    """One of the other BASELINE.json configurations with the same engine, reported under
    detail.configs (never as `value`): resident GFLOP/s, accuracy, dominant-kernel rate."""
    import torch
    from spllt_amd import api, matgen
    A, order, cfg = matgen.build_config(cfg_name, 1.0)
    if cfg_name == "poisson3d_128":
        order = None            # built-in nested dissection for config 3
    n, ptr, row, val = api.csc_lower_1based(A)
    f = api.Factorization(n, ptr, row, nb=cfg["nb"], nemin=32, prune_tree=False, order=order)
    si = f.sym_info()
    flops = float(si["flops"])
    dval = torch.tensor(val, device="cuda")
    torch.cuda.synchronize()
    f.factor_dev(dval.data_ptr()).wait()
    t0 = time.perf_counter()
    for _ in range(steps):
        f.factor_dev(dval.data_ptr()).wait()
    t = (time.perf_counter() - t0) / steps
    b = A @ np.ones(n)
    x = f.solve(b)
    r = b - A @ x
    roof, table, _ = roofline_from_profile(f, val)
    out = {"workload": cfg_name, "n": n, "nb": cfg["nb"], "nnz_L": int(si["nnz_l"]), "flops_sym": flops,
           "ms_per_step": round(t * 1e3, 2), "gflops": round(flops / t / 1e9, 1),
           "resid_2norm_rel": float(np.linalg.norm(r) / np.linalg.norm(b)),
           "bwd_err": float(np.linalg.norm(r) / (np.linalg.norm(b) + abs(A).max() * np.linalg.norm(x))),
           "dominant_kernel": roof["kernel"], "dominant_tflops": roof["achieved"],
           "dominant_frac": roof["frac"], "dominant_frac_alone": roof["frac_alone"],
           # the whole step against the same peak (the in-program figure of a kernel that runs on two
           # streams at once counts the time of BOTH launches: it reads low while the chip is full)
           "step_frac": round(flops / t / 1e12 / FP64_MFMA_PEAK_TFLOPS, 4)}
    f.close()
    del dval
    torch.cuda.empty_cache()
    return out


def run_small_config(label, A, nb, nemin, steps=30):
    """A small problem (BASELINE config 1, the smoke size), where the host's submission is as long as
    the device's work: wall / host-submit / device time per factorization with eager launches and
    with the two HIP-graph replays (engine flag bits 17 / 15 / 16) -- what decides the default of
    row f1 per problem size (reported under detail.small_configs, never as `value`)."""
    import torch
    from spllt_amd import api
    n, ptr, row, val = api.csc_lower_1based(A)
    dval = torch.tensor(val, device="cuda")
    out = {"workload": label, "n": n, "nb": nb}
    for mode, flag in (("default", 0), ("eager", 131072), ("graph_chain", 32768), ("graph_dag", 65536)):
        f = api.Factorization(n, ptr, row, nb=nb, nemin=nemin, prune_tree=False, engine_flags=flag)
        # (the chip needs ~100 ms of load to reach its clocks, profiles/r03/sustain_probe.txt: the first
        # mode measured is not to pay for that)
        for _ in range(300 if mode == "default" else 20):
            f.factor_dev(dval.data_ptr()).wait()
        torch.cuda.synchronize()
        sub, dev = [], []
        t0 = time.perf_counter()
        for _ in range(steps):
            f.factor_dev(dval.data_ptr()).wait()
            tm = f.times()
            sub.append(tm.get("submit_ms", 0.0))
            dev.append(tm.get("device_ms", 0.0))
        t = (time.perf_counter() - t0) / steps
        if mode == "default":
            si = f.sym_info()
            b = A @ np.ones(n)
            x = f.solve(b)
            out.update(flops_sym=float(si["flops"]), launches=int(len(f.program("launches"))),
                       bwd_err=float(np.linalg.norm(b - A @ x) / (np.linalg.norm(b) + abs(A).max() * np.linalg.norm(x))))
        out[mode] = {"wall_ms": round(t * 1e3, 4), "host_submit_ms": round(float(np.mean(sub)), 4),
                     "device_ms": round(float(np.mean(dev)), 4)}
        f.close()
    return out


def host_cores(cap=16):
    """cores this process may really use: affinity mask and cgroup CPU quota"""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(quota) // int(period)))
    except (OSError, ValueError):
        pass
    return max(1, min(n, cap))


def cpu_baseline(f, val, flops, threads):
    """The oracle (CPU restatement on MKL + OpenMP tasks with the reference's
    dependency tokens) on the SAME workload, timed on this host's cores."""
    from oracle import pyoracle
    try:
        o = pyoracle.OracleFactor.from_factorization(f, variant="mkl")
        blas = "mkl"
    except Exception:
        o = pyoracle.OracleFactor.from_factorization(f, variant="plain")
        blas, threads = "plain-c", 1
    dt, rc = None, 0
    for _ in range(2):   # best of two: the first run also pays the page faults of the arena
        t0 = time.time()
        rc = o.factorize(val, threads)
        dt = min(dt, time.time() - t0) if dt is not None else time.time() - t0
    out = {"value": round(flops / dt / 1e9, 2), "unit": "GFLOP/s", "cores": threads,
           "kind": "port", "seconds": round(dt, 3), "blas": blas, "rc": rc}
    if threads > 1:
        # t_cpu_seq beside t_cpu_omp (the reference drivers' window,
        # drivers/spllt_omp.F90:185-192): the same oracle, one thread, one run
        t0 = time.time()
        rc1 = o.factorize(val, 1)
        dt1 = time.time() - t0
        out["seq_seconds"] = round(dt1, 3)
        out["seq_value"] = round(flops / dt1 / 1e9, 2)
        out["seq_rc"] = rc1
        o.factorize(val, threads)     # (the check below reads the parallel run's factor)
    return o, out


def main():
    args = parse()
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1 and args.dump_outputs:
        sys.exit("bench.py: --dump-outputs needs a single-GPU run")
    import torch
    import torch.distributed as dist
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # rehearsal on a one-GPU box: SPLLT_DIST_BACKEND=gloo SPLLT_SINGLE_DEVICE=1
        # puts every rank on device 0 and reduces through gloo
        backend = os.environ.get("SPLLT_DIST_BACKEND", "nccl")
        dev = 0 if os.environ.get("SPLLT_SINGLE_DEVICE") else local_rank
        torch.cuda.set_device(dev)
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", dev))
        else:
            dist.init_process_group(backend)
    else:
        torch.cuda.set_device(0)
    from spllt_amd import api
    A, n, ptr, row, val, order, nb, name, cfg = build_workload(args)

    if world > 1:
        from spllt_amd import multigpu
        def roofline_of(f1, v):
            roof1, _, _ = roofline_from_profile(f1, v)
            attach_pmc(roof1, name)
            return roof1
        out = multigpu.bench_distributed(args, A, n, ptr, row, val, order, nb, name, rank, world,
                                         roofline_fn=roofline_of)
        if rank == 0:
            print(json.dumps(out))
        dist.barrier()
        dist.destroy_process_group()
        return

    t0 = time.time()
    f = api.Factorization(n, ptr, row, nb=nb, nemin=args.nemin, prune_tree=False, order=order,
                          panel_width=args.panel,
                          engine_flags=int(os.environ.get("SPLLT_ENGINE_FLAGS", "0")))
    t_analyse = time.time() - t0
    si = f.sym_info()
    flops = float(si["flops"])
    dval = torch.tensor(val, device="cuda")
    torch.cuda.synchronize()

    for _ in range(args.warmup):
        f.factor_dev(dval.data_ptr()).wait()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    dev_ms, sub_ms = [], []
    for _ in range(args.steps):
        f.factor_dev(dval.data_ptr()).wait()
        dev_ms.append(f.times()["device_ms"])
        sub_ms.append(f.times()["submit_ms"])
    torch.cuda.synchronize()
    t_total = time.perf_counter() - t0
    ms_per_step = t_total / args.steps * 1e3
    value = flops / (t_total / args.steps) / 1e9

    if args.dump_outputs:
        dump_outputs(args.dump_outputs, f)
    out = {
        "metric": "factorize GFLOP/s (fp64)", "value": round(value, 2), "unit": "GFLOP/s",
        "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(ms_per_step, 3), "higher_is_better": True, "scaling": "strong",
        "vs_baseline": None, "dtype": "f64", "data": "synthetic",
        "config": {"workload": name, "stand_in_for": "SuiteSparse ND/nd24k" if "nd24k" in name else None,
                   "n": n, "nnz_lower": int(si["nnz_a"]), "nb": nb, "nnz_L": int(si["nnz_l"]),
                   "flops_sym": flops, "nnodes": int(si["nnodes"]), "ordering": si["ordering"] + ("/geometric-nd" if order is not None else ""),
                   "parallelism": "1 GPU, level-batched stream DAG (chain / bulk / far streams, zone pipeline)"},
        "roofline": None, "cpu_baseline": None,
        "detail": {"device_ms_per_step": round(float(np.mean(dev_ms)), 3),
                   "host_submit_ms_per_step": round(float(np.mean(sub_ms)), 3), "analyse_s": round(t_analyse, 2),
                   "launches": f.times()["launches"],
                   "engine_flags": int(os.environ.get("SPLLT_ENGINE_FLAGS", "0")), "nemin": args.nemin},
    }
    if args.full:
        out["roofline"], out["cpu_baseline"], more = full_measurements(args, A, n, ptr, row, val, order, nb, name,
                                                                       f, dval, flops, value)
        out["detail"].update(more)
    print(json.dumps(out))


def full_measurements(args, A, n, ptr, row, val, order, nb, name, f, dval, flops, value):
    """--full: everything beside the headline, measured after the timed steps with the same handle
    (closed here before the other configurations run).  Returns the line's `roofline` and
    `cpu_baseline` and what it adds to `detail`."""
    import torch
    from spllt_amd import api

    # drop-in variant (H2D of val + D2H of L), reported separately, never `value`
    t0 = time.perf_counter()
    f.factor(val).wait()
    t_h2d = time.perf_counter() - t0
    t0 = time.perf_counter()
    L = f.get_factor()
    t_d2h = time.perf_counter() - t0
    t0 = time.perf_counter()
    f.get_factor(out=L)          # the same destination again: without the page faults of a fresh array
    t_d2h_warm = time.perf_counter() - t0

    check = {}
    t_solve = None
    if not args.no_check:
        b = A @ np.ones(n)
        f.solve(b)  # builds the device solve tables
        t0 = time.perf_counter()
        x = f.solve(b)
        t_solve = time.perf_counter() - t0
        r = b - A @ x
        check = {"resid_2norm_rel": float(np.linalg.norm(r) / np.linalg.norm(b)),
                 "bwd_err": float(np.linalg.norm(r) / (np.linalg.norm(b) + abs(A).max() * np.linalg.norm(x)))}

    roof, table, ms = roofline_from_profile(f, val)
    attach_pmc(roof, name)
    roof["step_frac"] = round(value / 1e3 / FP64_MFMA_PEAK_TFLOPS, 4)     # the whole step against the same peak
    # the real program on the clock (spllt_hip_timeline: its own events, nothing added to the
    # streams): ms after the value scatter at which the last event of each tree level completed
    level_done = None
    try:
        Lh = f.program("launches")
        runs = np.array([f.timeline(val) for _ in range(3)])
        tl = runs[int(np.argmin(runs[:, -1]))]
        level_done = {"program_end_ms": round(float(tl[-1]), 3),
                      "level_done_ms": [round(float(max(tl[i] for i in range(len(Lh)) if Lh[i][1] == k and tl[i] >= 0)), 3)
                                        for k in sorted(set(int(v) for v in Lh[:, 1]) - {-1})
                                        if any(Lh[i][1] == k and tl[i] >= 0 for i in range(len(Lh)))]}
    except Exception as e:   # noqa: BLE001 - a diagnostic, never a reason to lose the line
        level_done = {"error": repr(e)[:200]}
    if args.profile_out:
        Lh = f.program("launches")
        units, tiles = f.program("units"), f.program("tiles")
        bc_off = f.sym("bcol_off")

        def category(l):
            if l[0] != 1:
                return {0: "potrf", 4: "chain", 5: "winv", 6: "gather", 7: "panel", 8: "chain", 9: "trsm"}.get(int(l[0]), "other")
            if l[3] == 0:
                return "marker"
            u = units[int(tiles[int(l[2])]["unit"])]
            if u["mode"] == 2:
                return "trsm"        # rows below a panel / sub-tile: (left-looking update +) solve via Winv
            if u["mode"] == 1:
                return "between"
            if bc_off[int(u["src_bcol0"])] == u["d_off"]:
                return "inpanel"     # left-looking update of the next panel inside the block column
            # block column c -> c+1 (chain stream) / its remainder (side stream) / c -> c+2.. (bulk)
            return {0: "next", 3: "next_rest", 1: "trailing"}.get(int(l[6]), "update")
        with open(args.profile_out, "w") as fh:
            fh.write("idx kind level count tile gflop ms category\n")
            for i, (l, m) in enumerate(zip(Lh, ms)):
                fh.write(f"{i} {l[0]} {l[1]} {l[3]} {l[4]} {l[5] / 1e9:.4f} {m:.4f} {category(l)}\n")

    cpu = None
    if not args.no_cpu_baseline:
        threads = args.cpu_threads or host_cores()
        o, cpu = cpu_baseline(f, val, flops, threads)
        cpu["sample"] = f"full workload ({name}, {flops / 1e9:.0f} GFLOP), best of two factorizations"
        if not args.no_check:
            ref = o.arena()
            check["max_relerr_L_vs_cpu"] = float(np.abs(L - ref).max() / np.abs(ref).max())
            # the same system solved with the CPU oracle's factor, beside the GPU's
            xc = o.solve(b)
            rc_ = b - A @ xc
            check["resid_2norm_rel_cpu_oracle"] = float(np.linalg.norm(rc_) / np.linalg.norm(b))
            check["bwd_err_cpu_oracle"] = float(np.linalg.norm(rc_) / (np.linalg.norm(b) + abs(A).max() * np.linalg.norm(xc)))
            check["tolerance"] = ("pass iff bwd_err = ||r||/(||b|| + max|a_ij| ||x||) <= 1e-14 (reference "
                                  "src/utils_mod.F90:462-467) and max|L - L_cpu|/max|L_cpu| <= 1e-12.  The plain "
                                  "||r||/||b|| is ~1e-13 on this stand-in for BOTH factors: b = A*1 is a near-"
                                  "cancelling row sum (||A|| ||x|| / ||b|| ~ 7e2), so eps * that ratio is the floor")

    nlaunch = f.times()["launches"]
    # reference point for roofline.frac: the tuned library's DGEMM on the update kernel's operand
    # shapes (C -= A B^T, M = N = 8192) -- what an fp64 GEMM sustains on this box at these K
    dgemm_ref = None
    if not args.no_extra_configs:
        try:
            dgemm_ref = {"what": "rocBLAS DGEMM through torch.addmm, C(8192 x 8192) -= A(8192 x K) B(8192 x K)^T, sustained TFLOP/s"}
            for K in (256, 1024):
                Am = torch.randn(8192, K, dtype=torch.float64, device="cuda")
                Bm = torch.randn(8192, K, dtype=torch.float64, device="cuda")
                Cm = torch.zeros(8192, 8192, dtype=torch.float64, device="cuda")
                # sustained: ~150 ms of back-to-back calls first -- single calls between
                # synchronisations read 15-20 % low (the chip needs ~100 ms of continuous load to
                # reach its clocks, scripts/sustain_probe.hip) -- then the average of a timed train
                est_ms = 2.0 * 8192 * 8192 * K / 40e12 * 1e3
                for it in range(int(150.0 / est_ms) + 1):
                    torch.addmm(Cm, Am, Bm.t(), beta=1.0, alpha=-1.0, out=Cm)
                nrep = int(60.0 / est_ms) + 3
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for it in range(nrep):
                    torch.addmm(Cm, Am, Bm.t(), beta=1.0, alpha=-1.0, out=Cm)
                e1.record()
                torch.cuda.synchronize()
                best = e0.elapsed_time(e1) / nrep
                dgemm_ref[f"K{K}"] = round(2.0 * 8192 * 8192 * K / best / 1e9, 2)
            del Am, Bm, Cm
        except Exception as e:   # noqa: BLE001 - a reference point, never a reason to lose the line
            dgemm_ref = {"error": repr(e)[:200]}
    extra, small = [], []
    # Throughput of a STREAM of factorizations of one pattern (a time-stepping caller: analyse once,
    # factorize many): two handles on the same pattern, the next factorization submitted while the
    # previous one is in its latency-bound top levels.  Reported beside `value`, never as `value`
    # (the metric is one factorization at a time, like the reference's driver).
    two_handles = None
    if not args.no_extra_configs:
        try:
            f2 = api.Factorization(n, ptr, row, nb=nb, nemin=args.nemin, prune_tree=False, order=order,
                                   panel_width=args.panel, engine_flags=int(os.environ.get("SPLLT_ENGINE_FLAGS", "0")))
            f2.factor_dev(dval.data_ptr()).wait()
            f.factor_dev(dval.data_ptr()).wait()
            torch.cuda.synchronize()
            reps = max(2, args.steps // 2)
            t0 = time.perf_counter()
            for _ in range(reps):
                f.factor_dev(dval.data_ptr())
                f2.factor_dev(dval.data_ptr())
                f.wait()
                f2.wait()
            torch.cuda.synchronize()
            t2 = (time.perf_counter() - t0) / (2 * reps)
            two_handles = {"ms_per_factorization": round(t2 * 1e3, 3), "gflops": round(flops / t2 / 1e9, 1),
                           "note": "two handles of the same pattern in flight; informational, not the metric"}
            f2.close()
            del f2
        except Exception as e:   # noqa: BLE001 - a diagnostic, never a reason to lose the line
            two_handles = {"error": repr(e)[:200]}
    if not args.no_extra_configs and not args.mm and not args.rb and args.scale == 1.0:
        f.close()
        del dval
        torch.cuda.empty_cache()
        from spllt_amd import matgen as _mg
        for label, Am_, nb_, nemin_ in (("poisson2d_128 (BASELINE config 1)", _mg.poisson2d(128), 256, 32),
                                        ("poisson2d_48 (smoke size)", _mg.poisson2d(48), 32, 16)):
            try:
                small.append(run_small_config(label, Am_, nb_, nemin_))
            except Exception as e:   # noqa: BLE001 - a diagnostic, never a reason to lose the line
                small.append({"workload": label, "error": repr(e)[:200]})
        # (flan_like = BASELINE config 4 on one GPU: 32.7 GB of factor, ~0.8 s per factorization)
        for other in ("poisson3d_128", "serena_like") + (() if os.environ.get("SPLLT_NO_FLAN") else ("flan_like",)):
            if other != args.config:
                extra.append(run_extra_config(other))

    detail = {"dropin_factor_s": round(t_h2d, 4), "L_d2h_s": round(t_d2h, 4), "L_d2h_warm_s": round(t_d2h_warm, 4),
              "L_d2h_warm_GBps": round(L.nbytes / max(t_d2h_warm, 1e-9) / 1e9, 2),
              "device_solve_s": None if t_solve is None else round(t_solve, 5),
              "launches": nlaunch, "kernel_table": table, "timeline": level_done, "check": check,
              "dgemm_reference": dgemm_ref, "two_handles_in_flight": two_handles, "configs": extra,
              "small_configs": small}
    return roof, cpu, detail


if __name__ == "__main__":
    main()
