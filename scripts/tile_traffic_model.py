#!/usr/bin/env python3
"""Fabric traffic of the update launches as the tile order decides it, from the program tables alone
(CPU only: Factorization.program + sym, no device):

    python scripts/tile_traffic_model.py [--config nd24k_like] [--xcd-order 2]

The model: workgroup b of a launch runs on XCD b % 8; every XCD fetches each distinct operand strip
of its tiles ONCE per launch -- the A strip of a tile is (unit, ti), the B strip (unit, tj), each
rows x K x 8 bytes; the destination costs 16 B per entry for a plain read-modify-write and 8 B per
entry for atomic, TRSM and BUFFER units.  "algorithmic" is every distinct strip once per launch.
The model describes one-round launches (every tile of the launch resident at the same time); for
the large launches, whose over-fetch comes from L2 capacity across rounds, it is a lower bound.

Per launch category and tile size it prints the algorithmic operand bytes, the modelled operand
bytes, the destination bytes, (modelled + C) / (algorithmic + C), and the worst per-launch XCD work
balance (max over the XCDs of sum K of its tiles / mean; launches of >= 256 tiles).  "small" marks
the launches that SPLLT_XCD_ORDER=1 leaves in plain order (32-tiles, and fewer than 1280 64-tiles).
"""
import argparse
import contextlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NXCD = 8
L_GEMM = 1
MODE_DIRECT, MODE_SCATTER, MODE_TRSM, MODE_BUFFER = 0, 1, 2, 3
BALANCE_MIN_TILES = 256


@contextlib.contextmanager
def xcd_order_env(value):
    """SPLLT_XCD_ORDER = value inside the block (None: untouched).  The library reads it whenever it
    builds a program, and a handle without an engine builds its program at every program() call."""
    old = os.environ.get("SPLLT_XCD_ORDER")
    if value is not None:
        os.environ["SPLLT_XCD_ORDER"] = str(value)
    try:
        yield
    finally:
        if value is not None:
            if old is None:
                del os.environ["SPLLT_XCD_ORDER"]
            else:
                os.environ["SPLLT_XCD_ORDER"] = old


def config_factorization(config, engine_flags=0):
    """The bench workload's handle for a matgen.CONFIGS key"""
    from spllt_amd import api, matgen
    A, order, cfg = matgen.build_config(config, 1.0)
    n, ptr, row, _ = api.csc_lower_1based(A)
    return api.Factorization(n, ptr, row, nb=cfg["nb"], nemin=32, prune_tree=False, order=order,
                             engine_flags=engine_flags)


def program_tables(f, xcd_order=None):
    """The tables the model needs, of f's program under SPLLT_XCD_ORDER = xcd_order"""
    with xcd_order_env(xcd_order):
        return dict(launches=f.program("launches"), units=f.program("units"), tiles=f.program("tiles"),
                    bcol_off=f.sym("bcol_off"), bcol_width=f.sym("bcol_width"))


def unit_k(units, bcol_width):
    """K extent of every update unit"""
    csum = np.concatenate([[0], np.cumsum(bcol_width.astype(np.int64))])
    b0 = units["src_bcol0"].astype(np.int64)
    multi = csum[np.minimum(b0 + units["nseg"], len(bcol_width))] - csum[b0]
    single = np.where(units["klen"] >= 0, units["klen"], bcol_width[b0])
    return np.where(units["nseg"] == 1, single, multi).astype(np.int64)


def launch_category(launch, units, tiles, bcol_off):
    u = units[int(tiles[int(launch[2])]["unit"])]
    if u["mode"] == MODE_TRSM:
        return "trsm"
    if u["mode"] in (MODE_SCATTER, MODE_BUFFER):
        return "inter-node"
    if bcol_off[int(u["src_bcol0"])] == u["d_off"]:
        return "in-panel"
    return {0: "c->c+1", 3: "c->c+1 rest", 1: "trailing"}.get(int(launch[6]), "update")


def launch_traffic(tl, T, units, K):
    """Model of ONE launch: tl = its tiles in launch order, T = its tile edge.  Returns a dict of
    alg (algorithmic operand bytes), model (operand bytes, one fetch per XCD), c (destination
    bytes), balance (max XCD sum K / mean), work (sum K per XCD)."""
    uid = tl["unit"].astype(np.int64)
    ti, tj = tl["ti"].astype(np.int64), tl["tj"].astype(np.int64)
    u = units[uid]
    M, N, k = u["M"].astype(np.int64), u["N"].astype(np.int64), K[uid]
    rows = np.minimum(T, M - ti * T)
    cols = np.minimum(T, N - tj * T)
    xcd = np.arange(len(tl)) % NXCD
    a_bytes, b_bytes = rows * k * 8, cols * k * 8

    def distinct(where, strip, val):    # bytes of the distinct (where, unit, strip) triples; strip < 2^15
        _, idx = np.unique(((where * len(units) + uid) << 16) | strip, return_index=True)
        return int(val[idx].sum())
    alg = distinct(0, ti, a_bytes) + distinct(0, tj, b_bytes)
    model = distinct(xcd, ti, a_bytes) + distinct(xcd, tj, b_bytes)
    # destination entries of a tile: those with src_r0 + i >= src_c0 + j where the unit is cut at the diagonal
    cut = (u["lower"] != 0) & (u["mode"] != MODE_TRSM) & ((u["mode"] != MODE_DIRECT) | (u["src_r0"] == u["src_c0"]))
    i0, i1 = ti * T, ti * T + rows
    d = (u["src_c0"] - u["src_r0"]).astype(np.int64)
    j = (tj * T)[:, None] + np.arange(T)[None, :]
    below = np.clip(i1[:, None] - np.maximum(i0[:, None], j + d[:, None]), 0, None)
    below = np.where(np.arange(T)[None, :] < cols[:, None], below, 0).sum(axis=1)
    entries = np.where(cut, below, rows * cols)
    per_entry = np.where((u["mode"] != MODE_DIRECT) | (u["atomic"] != 0), 8, 16)
    work = np.bincount(xcd, weights=k, minlength=NXCD)
    return dict(alg=alg, model=model, c=int((entries * per_entry).sum()),
                balance=float(work.max() / work.mean()) if work.sum() > 0 else 1.0, work=work)


def was_unordered(T, count):
    """launches that SPLLT_XCD_ORDER=1 leaves in plain order"""
    return T == 32 or (T == 64 and count < 8 * 160)


def launches(t, small_only=False):
    """One record per update launch (L_GEMM with tiles) of the program tables t, in program order;
    small_only: only the launches that SPLLT_XCD_ORDER=1 leaves in plain order."""
    L, units, tiles = t["launches"], t["units"], t["tiles"]
    bcol_off, K = t["bcol_off"], unit_k(units, t["bcol_width"])
    out = []
    for idx, l in enumerate(L):
        if int(l[0]) != L_GEMM or int(l[3]) <= 0:
            continue
        first, count, T = int(l[2]), int(l[3]), int(l[4])
        if small_only and not was_unordered(T, count):
            continue
        rec = launch_traffic(tiles[first:first + count], T, units, K)
        rec.update(index=idx, first=first, count=count, tile=T, cat=launch_category(l, units, tiles, bcol_off),
                   small=was_unordered(T, count))
        out.append(rec)
    return out


def summarize(recs):
    """rows of the printed table: (category, tile, small) groups, then the sum over the small ones"""
    def row(name, g):
        alg, model, c = (sum(r[k] for r in g) for k in ("alg", "model", "c"))
        big = [r["balance"] for r in g if r["count"] >= BALANCE_MIN_TILES]
        return dict(group=name, launches=len(g), tiles=sum(r["count"] for r in g), alg=alg, model=model, c=c,
                    ratio=(model + c) / (alg + c) if alg + c else 1.0, balance=max(big) if big else None)
    keys = sorted({(r["cat"], r["tile"], r["small"]) for r in recs}, key=lambda k: (not k[2], k[0], k[1]))
    rows = [row(f"{c}, {t}-tile{', small' if s else ''}", [r for r in recs if (r["cat"], r["tile"], r["small"]) == (c, t, s)])
            for c, t, s in keys]
    rows.append(row("all small update launches", [r for r in recs if r["small"] and r["cat"] != "trsm"]))
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="nd24k_like", help="matgen.CONFIGS key")
    ap.add_argument("--xcd-order", type=int, default=None, help="SPLLT_XCD_ORDER of the program (default: the library's)")
    a = ap.parse_args()
    f = config_factorization(a.config)
    rows = summarize(launches(program_tables(f, a.xcd_order)))
    f.close()
    print(f"# {a.config}, SPLLT_XCD_ORDER={'default' if a.xcd_order is None else a.xcd_order}: "
          "bytes per factorization, one fetch of a strip per XCD per launch")
    print(f"{'launches':42s} {'n':>4s} {'tiles':>8s} {'alg GB':>8s} {'model GB':>9s} {'C GB':>7s} {'(m+C)/(a+C)':>11s} {'balance':>8s}")
    for r in rows:
        bal = f"{r['balance']:8.3f}" if r["balance"] is not None else f"{'-':>8s}"
        print(f"{r['group']:42s} {r['launches']:4d} {r['tiles']:8d} {r['alg'] / 1e9:8.3f} {r['model'] / 1e9:9.3f} "
              f"{r['c'] / 1e9:7.3f} {r['ratio']:11.3f} {bal}")


if __name__ == "__main__":
    main()
