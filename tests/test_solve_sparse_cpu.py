"""CPU tests of the sparse right-hand-side solve (spllt_hip_solve_sparse*, spllt_hip_gram_sparse): the interface
exists in every layer; the argument errors are decided before any device work; the plan of the library equals a
brute-force reach computed here from the row lists; the substitution program restricted to that plan, run by a
numpy interpreter on a dense factor from a vector that is NaN outside the touched rows, agrees with a dense
solve at the wanted entries; dropping a block column from the plan breaks it; Y^T Y over the touched rows is
B^T A^-1 B."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import scipy.linalg as sl
import scipy.sparse as sp

from helpers import dense_arena, make_case, sym_tables
from solve_sparse_emulate import bcol_of, brute_reach, emulate_solve_sparse, touched_rows
from spllt_amd import _lib, api, matgen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("spllt_hip_solve_sparse", "spllt_hip_solve_sparse_dev", "spllt_hip_gram_sparse",
         "spllt_hip_solve_sparse_plan", "spllt_hip_solve_sparse_info", "spllt_hip_release_solve_sparse")
CASES = {
    "p2d12": (lambda: matgen.poisson2d(12), dict(nb=16, nemin=4)),
    "box5": (lambda: matgen.nd_like((5, 5, 4), 1), dict(nb=16)),      # nodes of several block columns
}


def test_interface_exists_in_every_layer():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "spllt_hip.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _lib.HIP_SYMBOLS, name
        assert re.search(r"int\s+%s\s*\(void \*fkeep" % name, header), name
    assert re.search(r"int spllt_hip_solve_sparse_plan\(void \*fkeep, int k, const int \*bptr, const int \*brow, int nsel, "
                     r"const int \*sel,\s*int job, int32_t \*fwd_bcols, int64_t fwd_cap, int32_t \*bwd_bcols, "
                     r"int64_t bwd_cap,\s*int64_t counts\[2\]\);", header)
    for meth in ("solve_sparse", "gram", "inverse_block", "solve_sparse_plan", "solve_sparse_info",
                 "release_solve_sparse"):
        assert callable(getattr(api.Factorization, meth)), meth
    assert lib.spllt_hip_solve_sparse.argtypes[8] is C.c_int64 and lib.spllt_hip_gram_sparse.argtypes[6] is C.c_int64
    assert "inverse_block" in api.Factorization.inverse_entries.__doc__


@functools.lru_cache(maxsize=None)
def _case(name):
    gen, kw = CASES[name]
    A = gen()
    f, val = make_case(A, **kw)
    t = sym_tables(f)
    var_of = np.empty(f.n, dtype=np.int64)
    var_of[t["order"]] = np.arange(f.n)
    return A, f, t, var_of, dense_arena(f, A)


def _columns(n, var_of, cols, seed=0):
    """cols: per column the pivot positions of its nonzeros -> scipy CSC in user order, random values"""
    rng = np.random.default_rng(seed)
    rows = [var_of[p] for c in cols for p in c]
    cidx = [q for q, c in enumerate(cols) for _ in c]
    return sp.csc_matrix((rng.uniform(0.5, 1.5, len(rows)) * rng.choice([-1.0, 1.0], len(rows)), (rows, cidx)),
                         shape=(n, len(cols)))


def _inputs(name, t, nb):
    """the pivot positions the columns of the issue's list start from"""
    n = int(t["sptr"][-1])
    nn = len(t["sparent"])
    leaves = sorted(set(range(nn)) - set(int(p) for p in t["sparent"]))     # nobody's parent
    leaf_a, leaf_b = leaves[0], leaves[-1]
    assert leaf_a != leaf_b
    multi = [s for s in range(nn) if t["node_bcol0"][s + 1] - t["node_bcol0"][s] >= 2]
    if name == "box5":
        assert multi, "box5 must have a node of several block columns"
    mid = None
    if multi:
        b = int(t["node_bcol0"][multi[0]]) + 1
        mid = int(t["sptr"][multi[0]]) + int(t["bcol_r0"][b]) + int(t["bcol_width"][b]) // 2
        assert bcol_of(t, nb, mid) == b and int(t["bcol_width"][b]) // 2 > 0
    return dict(leaf=int(t["sptr"][leaf_a]), other_leaf=int(t["sptr"][leaf_b]), last=n - 1, mid=mid)


@pytest.mark.parametrize("name", list(CASES))
def test_plan_against_brute_force(name):
    A, f, t, var_of, _ = _case(name)
    n, nb, nbc = f.n, f.options.nb, len(t["bcol_off"])
    inp = _inputs(name, t, nb)
    col_sets = {
        "leaf": [[inp["leaf"]]],
        "last": [[inp["last"]]],
        "two_branches": [[inp["leaf"], inp["other_leaf"]]],
        "empty": [[]],
        "five": [[inp["leaf"]], [], [inp["other_leaf"], inp["last"]], [inp["leaf"] + 1], [inp["last"]]],
    }
    if inp["mid"] is not None:
        col_sets["mid"] = [[inp["mid"]]]
    wanted_sets = {
        "one": [inp["leaf"]],
        "other_branch": [inp["other_leaf"], inp["other_leaf"] + 1],
        "duplicates": [inp["leaf"], inp["last"], inp["leaf"]],
        "all": None,
    }
    for cname, cols in col_sets.items():
        B = _columns(n, var_of, cols)
        starts = [p for c in cols for p in c]
        want_f = brute_reach(t, nb, starts)
        for wname, wanted in wanted_sets.items():
            rows = None if wanted is None else var_of[wanted]
            want_b = np.arange(nbc) if wanted is None else brute_reach(t, nb, wanted)
            for job in (0, 1, 2):
                fwd, bwd = f.solve_sparse_plan(B, rows=rows, job=job)
                assert np.array_equal(fwd, want_f if job != 2 else []), (cname, wname, job)
                assert np.array_equal(bwd, want_b if job != 1 else []), (cname, wname, job)
        if cname in ("leaf", "two_branches", "mid", "five"):
            assert 0 < len(want_f) < nbc, (cname, len(want_f), nbc)     # the restriction is real
        if cname == "last":
            assert list(want_f) == [nbc - 1]
        if cname == "empty":
            assert len(want_f) == 0
    print(name, "block columns", nbc, "reach of a leaf", len(brute_reach(t, nb, [inp["leaf"]])))


def _dense(A, t):
    n = A.shape[0]
    P = np.empty(n, dtype=np.int64)
    P[t["order"]] = np.arange(n)
    Ad = A.toarray()
    return Ad, sl.cholesky(Ad[np.ix_(P, P)], lower=True)


def _run_filtered(f, t, arena, B, wanted, job, fwd, bwd, touched=None):
    """the interpreter on a vector that is NaN outside the touched rows; returns (values at the wanted positions
    (nwanted x k), the vector, the touched mask)"""
    n, k = B.shape
    order = t["order"]
    if touched is None:
        touched = touched_rows(t, fwd, bwd, wanted)
    y = np.full((k, n), np.nan)
    y[:, touched] = 0.0
    Bc = B.tocoo()
    for r, c, v in zip(Bc.row, Bc.col, Bc.data):
        if touched[order[r]]:
            y[c, order[r]] = v
    emulate_solve_sparse(f, arena, y, fwd, bwd, job)
    return y[:, wanted].T, y, touched


@pytest.mark.parametrize("job", [0, 1, 2])
@pytest.mark.parametrize("name", list(CASES))
def test_filtered_program_is_sufficient(name, job):
    A, f, t, var_of, arena = _case(name)
    n, nb = f.n, f.options.nb
    inp = _inputs(name, t, nb)
    Ad, Ld = _dense(A, t)
    order = t["order"]
    cols = [[inp["leaf"]], [inp["other_leaf"], inp["last"]], [], [inp["leaf"] + 1, inp["other_leaf"]]]
    if inp["mid"] is not None:
        cols.append([inp["mid"]])
    B = _columns(n, var_of, cols, seed=1)
    Bp = np.zeros((n, len(cols)))
    Bp[order] = B.toarray()
    full = {0: lambda: np.linalg.solve(Ad, B.toarray())[var_of],             # by pivot position
            1: lambda: sl.solve_triangular(Ld, Bp, lower=True),
            2: lambda: sl.solve_triangular(Ld, Bp, lower=True, trans="T")}[job]()
    for wanted in ([inp["leaf"]], [inp["other_leaf"], inp["last"], inp["other_leaf"]], [inp["last"] - 1, 3],
                   list(range(n))):
        rows = None if len(wanted) == n else var_of[wanted]
        fwd, bwd = f.solve_sparse_plan(B, rows=rows, job=job)
        got, y, touched = _run_filtered(f, t, arena, B, wanted, job, fwd, bwd)
        ref = full[wanted]
        if job == 2:
            # entries of B outside the closure of the wanted rows are not scattered: they cannot reach them
            keep = touched[:, None] * np.ones((1, len(cols)))
            ref = sl.solve_triangular(Ld, Bp * keep, lower=True, trans="T")[wanted]
            np.testing.assert_allclose(ref, full[wanted], rtol=0, atol=1e-13 * np.abs(full).max())
        err = np.abs(got - ref).max()
        print(name, job, len(wanted), "fwd", len(fwd), "bwd", len(bwd), "err / max|x|", err / np.abs(full).max())
        assert np.isfinite(got).all()
        assert err <= 1e-12 * np.abs(full).max()
        assert np.isnan(y[:, ~touched]).all()            # nothing outside the touched rows was written either
        if job != 2:
            assert (got[:, 2] == 0.0).all()              # the empty column: exact zeros


@pytest.mark.parametrize("name", list(CASES))
def test_dropping_a_block_column_breaks_it(name):
    A, f, t, var_of, arena = _case(name)
    n, nb = f.n, f.options.nb
    inp = _inputs(name, t, nb)
    Ad, _ = _dense(A, t)
    B = _columns(n, var_of, [[inp["leaf"]], [inp["other_leaf"]]], seed=2)
    wanted = [inp["leaf"], inp["other_leaf"]]
    ref = np.linalg.solve(Ad, B.toarray())[var_of[wanted]]
    fwd, bwd = f.solve_sparse_plan(B, rows=var_of[wanted], job=0)
    bar = 1e-12 * np.abs(np.linalg.solve(Ad, B.toarray())).max()
    touched = touched_rows(t, fwd, bwd, wanted)
    got, _, _ = _run_filtered(f, t, arena, B, wanted, 0, fwd, bwd, touched)
    assert np.abs(got - ref).max() <= bar
    for which, drop in (("fwd", fwd[0]), ("fwd", fwd[-1]), ("bwd", bwd[len(bwd) // 2]), ("bwd", bwd[0])):
        f2 = [b for b in fwd if which != "fwd" or b != drop]
        b2 = [b for b in bwd if which != "bwd" or b != drop]
        got, _, _ = _run_filtered(f, t, arena, B, wanted, 0, f2, b2, touched)
        assert not np.abs(got - ref).max() <= bar, (which, drop)


@pytest.mark.parametrize("name", list(CASES))
def test_gram_recurrence(name):
    A, f, t, var_of, arena = _case(name)
    n, nb = f.n, f.options.nb
    inp = _inputs(name, t, nb)
    Ad, _ = _dense(A, t)
    cols = [[inp["leaf"]], [inp["other_leaf"], inp["last"]], [], [inp["leaf"] + 1, inp["other_leaf"]], [inp["last"]]]
    B = _columns(n, var_of, cols, seed=3)
    fwd, bwd = f.solve_sparse_plan(B, rows=[], job=1)
    assert len(bwd) == 0 and len(fwd) < len(t["bcol_off"])
    _, y, touched = _run_filtered(f, t, arena, B, [], 1, fwd, bwd)
    Y = y[:, touched]
    G = Y @ Y.T
    ref = B.toarray().T @ np.linalg.solve(Ad, B.toarray())
    print(name, "touched rows", int(touched.sum()), "err / max|G|", np.abs(G - ref).max() / np.abs(ref).max())
    assert np.abs(G - ref).max() <= 1e-11 * np.abs(ref).max()
    assert (G[2] == 0.0).all() and (G[:, 2] == 0.0).all()


def test_argument_errors_on_an_analysed_handle():
    f, val = make_case(matgen.poisson2d(8), nb=8, nemin=4)
    n, k = f.n, 2
    sentinel = -7.25e77
    x = np.full(3 * (n + 2), sentinel)
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    ptr, row, bv = i32([1, 3, 4]), i32([2, 5, 7]), np.array([1.0, 2.0, 3.0])
    sel = i32([1, n, 3])
    ip, dp = api._ip, api._dp
    solve, solve_dev, gram = f.lib.spllt_hip_solve_sparse, f.lib.spllt_hip_solve_sparse_dev, f.lib.spllt_hip_gram_sparse
    good = dict(k=k, ptr=ip(ptr), row=ip(row), val=dp(bv), nsel=3, sel=ip(sel), x=dp(x), ldx=3, job=0)
    bad = [
        (dict(ptr=None), "null"), (dict(x=None), "null"), (dict(row=None), "null"), (dict(val=None), "null"),
        (dict(k=-1), "k < 0"), (dict(ptr=ip(i32([0, 2, 3]))), "bptr[0]"), (dict(ptr=ip(i32([1, 3, 2]))), "decrease"),
        (dict(row=ip(i32([2, 5, n + 1]))), "outside"), (dict(row=ip(i32([0, 5, 7]))), "outside"),
        (dict(row=ip(i32([5, 5, 7]))), "increasing"), (dict(row=ip(i32([5, 2, 7]))), "increasing"),
        (dict(sel=ip(i32([1, n + 1, 3]))), "outside"), (dict(sel=ip(i32([0, 1, 3]))), "outside"),
        (dict(ldx=2), "leading dimension"), (dict(nsel=-1, sel=None, ldx=n - 1), "leading dimension"),
        (dict(job=3), "job"), (dict(job=-1), "job"),
    ]
    for change, word in bad:
        a = dict(good, **change)
        for fn in (solve, solve_dev):
            xarg = a["x"] if fn is solve or a["x"] is None else x.ctypes.data
            rc = fn(f.fkeep, a["k"], a["ptr"], a["row"], a["val"], a["nsel"], a["sel"], xarg, a["ldx"], a["job"])
            assert rc == -10, (change, rc)
            assert word in f.last_error(), (change, f.last_error())
    G = np.full(9, sentinel)
    for change, word in [(dict(ptr=None), "null"), (dict(x=None), "null"), (dict(val=None), "null"), (dict(k=-1), "k < 0"),
                         (dict(row=ip(i32([5, 2, 7]))), "increasing"), (dict(ldx=1), "leading dimension")]:
        a = dict(dict(good, x=dp(G), ldx=2), **change)
        assert gram(f.fkeep, a["k"], a["ptr"], a["row"], a["val"], a["x"], a["ldx"]) == -10, change
        assert word in f.last_error(), (change, f.last_error())
    cnt = np.zeros(2, dtype=np.int64)
    cp = cnt.ctypes.data_as(C.POINTER(C.c_int64))
    plan = f.lib.spllt_hip_solve_sparse_plan
    assert plan(f.fkeep, k, ip(ptr), ip(row), 3, ip(sel), 0, None, 0, None, 0, cp) == 0 and cnt[0] > 0 and cnt[1] > 0
    assert plan(f.fkeep, k, ip(ptr), ip(i32([5, 2, 7])), 3, ip(sel), 0, None, 0, None, 0, cp) == -10
    assert plan(f.fkeep, k, ip(ptr), ip(row), 3, ip(sel), 5, None, 0, None, 0, cp) == -10
    assert plan(f.fkeep, k, ip(ptr), ip(row), 3, ip(sel), 0, None, 0, None, 0, None) == -10
    assert plan(None, k, ip(ptr), ip(row), 3, ip(sel), 0, None, 0, None, 0, cp) == -10
    # good arguments, nothing factorized (or no device to find that out on): an error flag, nothing written
    rc = solve(f.fkeep, k, ip(ptr), ip(row), dp(bv), 3, ip(sel), dp(x), 3, 0)
    assert rc in (-10, -30), rc
    if rc == -10:
        assert "factorized" in f.last_error()
    assert gram(f.fkeep, k, ip(ptr), ip(row), dp(bv), dp(G), 2) in (-10, -30)
    assert solve(None, k, ip(ptr), ip(row), dp(bv), 3, ip(sel), dp(x), 3, 0) == -10
    assert (x == sentinel).all() and (G == sentinel).all()
    out = np.full(6, -1, dtype=np.int64)
    assert f.lib.spllt_hip_solve_sparse_info(f.fkeep, out.ctypes.data_as(C.POINTER(C.c_int64))) == 0 and (out == 0).all()
    assert f.program("solve_sparse_host_us") == 0                         # per handle: no sparse solve has run on it
    assert f.lib.spllt_hip_release_solve_sparse(f.fkeep) in (0, -30)    # (-30: the engine found no device)
    f.close()
