"""CPU tests of the reproducible solve: the interface exists in every layer, the "rsolve_*" tables
interpreted in numpy solve the system and keep their invariants, the test matrices really have the two
conflicts the tables resolve, and the argument errors that are decided before any device work."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from helpers import dense_arena, make_case
from solve_repro_emulate import emulate_solve_repro, tables
from spllt_amd import _lib, api, matgen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (name, generator, nb, nemin): the cases of the GPU tests
CASES = [
    ("p2d12-nb8", lambda: matgen.poisson2d(12), 8, 4),
    ("p2d40-nb16", lambda: matgen.poisson2d(40), 16, 16),
    ("box11-nb64", lambda: matgen.nd_like((11, 10, 9), 2), 64, 16),
    ("p3d14-nb384", lambda: matgen.poisson3d(14), 384, 16),
    ("box12-nb512", lambda: matgen.nd_like((10, 12, 12), 3), 512, 16),
]
NAMES = [c[0] for c in CASES]


@functools.lru_cache(maxsize=None)
def _case(name):
    _, gen, nb, nemin = next(c for c in CASES if c[0] == name)
    f, _val = make_case(gen(), nb=nb, nemin=nemin)
    prog = {k: f.program(k) for k in ("solve_units", "solve_list", "solve_tiles", "solve_fwd", "solve_bwd")}
    return f, prog, tables(f)


def test_interface_exists_in_every_layer():
    lib = _lib.load()
    names = ("spllt_hip_solve_repro", "spllt_hip_solve_repro_dev", "spllt_hip_set_reproducible_solve",
             "spllt_hip_release_solve_repro")
    for name in names:
        assert hasattr(lib, name), name
        assert name in _lib.HIP_SYMBOLS
    header = open(os.path.join(ROOT, "include", "spllt_hip.h")).read()
    assert re.search(r"int\s+spllt_hip_solve_repro\(void \*fkeep, int nrhs, double \*x_host, int64_t ldx, int job\);", header)
    assert re.search(r"int\s+spllt_hip_solve_repro_dev\(void \*fkeep, int nrhs, double \*x_dev, int64_t ldx, int job,\s*"
                     r"int pivot_order\);", header)
    assert re.search(r"int\s+spllt_hip_set_reproducible_solve\(void \*fkeep, int on\);", header)
    assert re.search(r"int\s+spllt_hip_release_solve_repro\(void \*fkeep\);", header)
    for m in ("solve_reproducible", "solve_reproducible_dev", "set_reproducible_solve", "release_solve_repro"):
        assert callable(getattr(api.Factorization, m)), m
    assert lib.spllt_hip_solve_repro.argtypes[3] is C.c_int64 and lib.spllt_hip_solve_repro_dev.argtypes[3] is C.c_int64


GENS = [lambda: matgen.nd_like((8, 7, 7), 2), lambda: matgen.poisson2d(24),
        lambda: sp.block_diag([matgen.poisson2d(6), matgen.poisson2d(5)]).tocsc()]


@pytest.mark.parametrize("gen", GENS)
@pytest.mark.parametrize("nb,pw", [(16, 8), (48, 16), (200, 64)])
def test_tables_interpreted_in_numpy_equal_the_dense_solve(gen, nb, pw):
    A = gen()
    f, val = make_case(A, nb=nb, nemin=8, panel_width=pw)
    L = dense_arena(f, A)
    n = f.n
    X = np.random.default_rng(0).standard_normal((n, 3))
    B = A @ X
    pos = f.sym("order")
    Y = np.zeros((3, n))
    Y[:, pos] = B.T
    emulate_solve_repro(f, L, Y)
    assert np.isfinite(Y).all()          # (the scratch starts as NaN: every slot read was written first)
    np.testing.assert_allclose(Y[:, pos].T, X, rtol=0, atol=1e-9)
    Y2 = np.zeros((3, n))
    Y2[:, pos] = B.T
    emulate_solve_repro(f, L, Y2, job=1)
    emulate_solve_repro(f, L, Y2, job=2)
    np.testing.assert_allclose(Y2, Y, rtol=1e-12, atol=1e-12)


def _launch_of(launches, kind, nitems):
    """index of the launch of `kind` that holds item i of its table, for every i < nitems"""
    out = np.full(nitems, -1)
    for li, (k, _lev, first, count) in enumerate(launches):
        if k == kind:
            out[first:first + count] = li
    return out


@pytest.mark.parametrize("name", NAMES)
def test_table_invariants(name):
    f, prog, t = _case(name)
    units, lst, tiles, fwd = prog["solve_units"], prog["solve_list"], prog["solve_tiles"], prog["solve_fwd"]
    rlist = f.sym("rlist")
    n, nbc = f.n, len(units)
    fslot, gptr, gsrc = t["fslot"], t["gptr"], t["gsrc"]
    below = units["nrow"].astype(np.int64) - units["w"]
    assert t["frows"] == int(below.sum())
    assert len(fslot) == nbc and len(gptr) == n + 1 and gptr[0] == 0 and gptr[-1] == t["frows"]
    assert np.array_equal(fslot, np.concatenate([[0], np.cumsum(below)[:-1]]))
    assert np.array_equal(np.sort(gsrc), np.arange(t["frows"]))
    # every source slot of p is the product for a row of its block column that IS p; sources ascend
    # (a block column without rows below shares its fslot with the next one: side="right" picks the one with rows)
    src_bcol = np.searchsorted(fslot, gsrc, side="right") - 1
    assert (below[src_bcol] > 0).all()
    u = units[src_bcol]
    row = u["w"] + (gsrc - fslot[src_bcol])
    assert (row < u["nrow"]).all()
    want = np.repeat(np.arange(n), np.diff(gptr))
    assert np.array_equal(rlist[u["idx_off"] + row], want)
    for p in range(n):
        assert (np.diff(src_bcol[gptr[p]:gptr[p + 1]]) > 0).all()
    # the strip launch that writes a slot precedes the diagonal launch that reads it
    strip_launch = _launch_of(fwd, 1, len(tiles))
    diag_launch = _launch_of(fwd, 0, len(lst))
    launch_of_bcol_diag = np.full(nbc, -1)
    launch_of_bcol_diag[lst] = diag_launch
    assert (launch_of_bcol_diag >= 0).all()
    tile_of = {(int(tl["unit"]), int(tl["ti"])): i for i, tl in enumerate(tiles)}
    reader_bcol = np.searchsorted(units["gcol0"], want, side="right") - 1
    assert ((units["gcol0"][reader_bcol] <= want) & (want < units["gcol0"][reader_bcol] + units["w"][reader_bcol])).all()
    writer = np.array([strip_launch[tile_of[(int(b), int((r - units["w"][b]) // 64))]] for b, r in zip(src_bcol, row)])
    assert (writer >= 0).all() and (writer < launch_of_bcol_diag[reader_bcol]).all()
    # backward: disjoint ranges inside bsize, strips of a block column consecutive from bfirst
    bslot, bfirst = t["bslot"], t["bfirst"]
    assert len(bslot) == len(tiles)
    lo = bslot
    hi = bslot + units["w"][tiles["unit"]]
    o = np.argsort(lo)
    assert lo.min(initial=0) >= 0 and hi.max(initial=0) <= t["bsize"]
    assert (hi[o][:-1] <= lo[o][1:]).all()
    for i, tl in enumerate(tiles):
        b = int(tl["unit"])
        assert bslot[i] == bfirst[b] + int(tl["ti"]) * int(units["w"][b])
    assert ((bfirst == -1) == (below == 0)).all()


@pytest.mark.parametrize("name", NAMES)
def test_every_case_has_the_hazard(name):
    f, prog, t = _case(name)
    units, tiles, fwd = prog["solve_units"], prog["solve_tiles"], prog["solve_fwd"]
    rlist = f.sym("rlist")
    most = 0
    for kind, _lev, first, count in fwd:
        if kind != 1:
            continue
        hits = {}
        for tl in tiles[first:first + count]:
            u = units[int(tl["unit"])]
            r0 = int(u["w"]) + int(tl["ti"]) * 64
            r1 = min(r0 + 64, int(u["nrow"]))
            for p in rlist[int(u["idx_off"]) + r0:int(u["idx_off"]) + r1]:
                hits.setdefault(int(p), set()).add(int(tl["unit"]))
        most = max([most] + [len(v) for v in hits.values()])
    assert most >= 2, "no row is hit by two block columns of one forward launch"
    strips = np.bincount(tiles["unit"], minlength=len(units)).max()
    if name != "p2d12-nb8":
        assert strips >= 2, "no block column has two strips"


def test_argument_errors_on_an_analysed_handle():
    f, val = make_case(matgen.poisson2d(8), nb=8, nemin=4)
    n = f.n
    x = np.ones(3 * (n + 2))
    call, call_dev = f.lib.spllt_hip_solve_repro, f.lib.spllt_hip_solve_repro_dev
    cases = [(-1, api._dp(x), n, 0, "nrhs"), (3, api._dp(x), n - 1, 0, "ldx"), (3, api._dp(x), n, 3, "job"),
             (3, api._dp(x), n, -1, "job"), (3, None, n, 0, "null")]
    for nrhs, ptr, ldx, job, word in cases:
        assert call(f.fkeep, nrhs, ptr, ldx, job) == -10
        assert word in f.last_error(), f.last_error()
    addr = x.ctypes.data
    for nrhs, ptr, ldx, job, word in [(-1, addr, n, 0, "nrhs"), (3, addr, n - 1, 0, "ldx"), (3, addr, n, 7, "job"),
                                      (3, None, n, 0, "null")]:
        assert call_dev(f.fkeep, nrhs, ptr, ldx, job, 0) == -10
        assert word in f.last_error(), f.last_error()
    assert call(f.fkeep, 3, api._dp(x), n + 2, 0) == -10
    assert "factorized" in f.last_error()
    assert call(f.fkeep, 0, api._dp(x), n, 0) == -10
    assert (x == 1.0).all()
    assert call(None, 3, api._dp(x), n, 0) == -10
    # the switch lives on the handle and needs no device
    assert f.lib.spllt_hip_set_reproducible_solve(f.fkeep, 1) == 0
    assert f.lib.spllt_hip_set_reproducible_solve(f.fkeep, 1) == 1
    assert f.set_reproducible_solve(False) is True and f.set_reproducible_solve(False) is False
    assert f.lib.spllt_hip_set_reproducible_solve(None, 1) == -10
    assert f.lib.spllt_hip_release_solve_repro(f.fkeep) == 0
    f.close()
