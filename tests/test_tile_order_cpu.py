"""The XCD-aware tile order of the update launches (schedule.cpp emit_gemm, SPLLT_XCD_ORDER), on
program tables only: the order is a permutation inside every launch, it changes nothing else of the
program, it never costs modelled fabric bytes (scripts/tile_traffic_model.py: one fetch of an operand
strip per XCD per launch), it keeps the XCDs even in work, and the tables still reproduce the oracle."""
import importlib.util
import os

import numpy as np
import pytest

from emulate import emulate_program
from helpers import dense_arena, lower_mask, make_case, oracle_factor, rel_err
from spllt_amd import matgen

_spec = importlib.util.spec_from_file_location(
    "tile_traffic_model", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                       "scripts", "tile_traffic_model.py"))
model = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(model)

PLAIN, NEW = 0, 2
L_GEMM, MODE_TRSM = 1, 2


def small_case(**kw):
    """7-point Poisson on 12^3, nb 64, nemin 4: the smallest of the grids tried (10^3 .. 14^3, Poisson
    and box stencils) that has every launch shape of test_case_has_the_launch_shapes AND launches of
    at least 256 tiles, so that the balance bound is checked on something."""
    return make_case(matgen.poisson3d(12), nb=64, nemin=4, **kw)


def tables(f, order):
    return model.program_tables(f, order)


def update_launches(t):
    """(launch row, its tiles) of every update launch the new order may touch"""
    for l in t["launches"]:
        if int(l[0]) != L_GEMM or int(l[3]) <= 0:
            continue
        tl = t["tiles"][int(l[2]):int(l[2]) + int(l[3])]
        if t["units"][int(tl[0]["unit"])]["mode"] == MODE_TRSM:
            continue
        yield l, tl


@pytest.fixture(scope="module")
def case():
    """(handle, values, tables in plain order, tables in the new order), built once; the multi-stream
    program, as the function-scoped rule of conftest.py selects it for every test"""
    f, val = small_case()
    with pytest.MonkeyPatch.context() as mp:
        if "SPLLT_CHAIN_GRAPH_SERIAL" not in os.environ:
            mp.setenv("SPLLT_CHAIN_GRAPH_SERIAL", "0")
        t0, t2 = tables(f, PLAIN), tables(f, NEW)
    yield f, val, t0, t2
    f.close()


def test_case_has_the_launch_shapes(case):
    f, val, t0, t2 = case
    K = model.unit_k(t2["units"], t2["bcol_width"])
    two_k = ragged = non8 = tiny = big = 0
    for l, tl in update_launches(t2):
        us = np.unique(tl["unit"])
        if int(l[4]) == 32 and len(np.unique(K[us])) >= 2:
            two_k += 1
        for u in us:
            mine = tl[tl["unit"] == u]
            if len(np.unique(mine["tj"])) >= 2 and len(np.unique(mine["ti"])) % 8:
                ragged += 1
        non8 += int(l[3]) % 8 != 0
        tiny += int(l[3]) < 8
        big += int(l[3]) >= model.BALANCE_MIN_TILES
    assert two_k >= 1      # a 32-tile launch with units of different K
    assert ragged >= 1     # a unit of >= 2 tile columns whose tile-row count is no multiple of 8
    assert non8 >= 1       # a launch whose tile count is no multiple of 8
    assert tiny >= 1       # a launch of fewer than 8 tiles
    assert big >= 1        # a launch the balance bound applies to


def test_order_is_a_permutation_inside_every_launch(case):
    f, val, t0, t2 = case
    assert np.array_equal(t0["launches"], t2["launches"])     # boundaries, flops, streams, waits, records
    assert np.array_equal(t0["units"], t2["units"])
    assert len(t0["tiles"]) == len(t2["tiles"])
    moved = 0
    for l in t0["launches"]:
        a = t0["tiles"][int(l[2]):int(l[2]) + int(l[3])] if int(l[0]) == L_GEMM else t0["tiles"][0:0]
        b = t2["tiles"][int(l[2]):int(l[2]) + int(l[3])] if int(l[0]) == L_GEMM else t2["tiles"][0:0]
        key = ("unit", "ti", "tj")
        assert np.array_equal(np.sort(a, order=key), np.sort(b, order=key))
        moved += int((a != b).sum())
    assert moved > 0                                           # the new order did something
    # whatever is not an update launch's range of the tile table is untouched
    touched = np.zeros(len(t0["tiles"]), dtype=bool)
    for l, tl in update_launches(t0):
        touched[int(l[2]):int(l[2]) + int(l[3])] = True
    assert np.array_equal(t0["tiles"][~touched], t2["tiles"][~touched])


def test_switch_is_read_per_program(case, monkeypatch):
    """one handle, one process: every value of the switch gives its own program; 1 orders only the
    launches of many rounds, which this case does not have"""
    f, val, t0, t2 = case
    monkeypatch.setenv("SPLLT_XCD_ORDER", "1")
    assert np.array_equal(f.program("tiles"), t0["tiles"])
    monkeypatch.setenv("SPLLT_XCD_ORDER", "2")
    assert np.array_equal(f.program("tiles"), t2["tiles"])
    monkeypatch.delenv("SPLLT_XCD_ORDER")
    assert np.array_equal(f.program("tiles"), t2["tiles"])     # the default is the new order


def test_modelled_bytes_and_balance(case):
    f, val, t0, t2 = case
    K = model.unit_k(t2["units"], t2["bcol_width"])
    n = 0
    for (l0, a), (l2, b) in zip(update_launches(t0), update_launches(t2)):
        if np.array_equal(a, b):
            continue
        n += 1
        T = int(l0[4])
        plain, new = model.launch_traffic(a, T, t0["units"], K), model.launch_traffic(b, T, t2["units"], K)
        assert new["alg"] == plain["alg"] and new["c"] == plain["c"]
        assert new["model"] <= plain["model"], (l0, new["model"], plain["model"])
        if int(l0[3]) >= model.BALANCE_MIN_TILES:
            assert new["balance"] <= 1.05, (l0, new["balance"])
    assert n > 0


def test_heaviest_first_on_every_xcd(case):
    f, val, t0, t2 = case
    K = model.unit_k(t2["units"], t2["bcol_width"])
    for l, tl in update_launches(t2):
        for r in range(model.NXCD):
            k = K[tl["unit"][r::model.NXCD]]
            assert (np.diff(k) <= 0).all()


def test_new_order_reproduces_oracle(monkeypatch):
    monkeypatch.setenv("SPLLT_XCD_ORDER", str(NEW))
    A = matgen.poisson3d(12)
    f, val = make_case(A, nb=64, nemin=4)
    got = emulate_program(f, val)
    o, rc = oracle_factor(f, val)
    assert rc == 0
    mask = lower_mask(f)
    assert rel_err(got, o.arena(), mask) < 1e-13
    assert rel_err(got, dense_arena(f, A), mask) < 1e-13
    assert np.all(got[~mask] == 0.0)
    f.close()


def test_bench_workload_modelled_traffic():
    """nd24k_like: (operands + C) / (algorithmic operands + C) of the launches the round-3 order left
    plain, 2.30 before (scripts/tile_traffic_model.py --xcd-order 1); contiguous equal-work shares
    reach 1.08 overall and 1.28 in the worst category"""
    f = model.config_factorization("nd24k_like")
    recs = [r for r in model.launches(tables(f, NEW), small_only=True) if r["cat"] != "trsm"]
    f.close()
    ratio = lambda g: (sum(r["model"] + r["c"] for r in g)) / (sum(r["alg"] + r["c"] for r in g))   # noqa: E731
    assert len(recs) > 200
    assert ratio(recs) <= 1.15
    for cat, T in sorted({(r["cat"], r["tile"]) for r in recs}):
        g = [r for r in recs if (r["cat"], r["tile"]) == (cat, T)]
        assert ratio(g) <= 1.35, (cat, T, ratio(g))
    for r in recs:
        if r["count"] >= model.BALANCE_MIN_TILES:
            assert r["balance"] <= 1.05, (r["cat"], r["tile"], r["count"], r["balance"])
