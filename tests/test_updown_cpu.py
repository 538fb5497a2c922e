"""CPU tests of the low-rank update / downdate (spllt_hip_updown*): the plan of spllt_hip_updown_plan against
the union of tree paths computed here from the exported tree, the rejection of malformed and inadmissible
columns, and the recurrence itself -- the numpy interpreter tests/updown_emulate.py, driven by the library's
plan, against a dense Cholesky factor of P (A +- W W^T) P^T at the project's L-parity bar, 1e-12 relative to
max|L|, and on the 12 x 12 Poisson grid, where the recurrence alone is the whole error, 6e-16."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import updown_emulate as em
from helpers import dense_arena, lower_mask, make_case, rel_err, sym_tables
from spllt_amd import api, matgen

BAR = 1e-12
CASES = {
    "p2d12": (lambda: matgen.poisson2d(12), dict(nb=16, nemin=4)),
    "box5": (lambda: matgen.nd_like((5, 5, 4), 1), dict(nb=16)),      # nodes of several block columns
}


@functools.lru_cache(maxsize=None)
def _case(name):
    gen, kw = CASES[name]
    A = sp.csc_matrix(gen())
    f, val = make_case(A, **kw)
    t = sym_tables(f)
    return A, f, t, dense_arena(f, A), lower_mask(f)


def _unit(n, var):
    return sp.csc_matrix(([1.0], ([int(var)], [0])), shape=(n, 1))


def _var_of(t):
    inv = np.empty(len(t["order"]), dtype=np.int64)
    inv[t["order"]] = np.arange(len(t["order"]))
    return inv


# ---- the plan ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_plan_is_the_union_of_tree_paths(name):
    A, f, t, _, _ = _case(name)
    n, nb = f.n, CASES[name][1]["nb"]
    var = _var_of(t)
    nn = len(t["sparent"])
    singles = {"leaf": 0, "last pivot": n - 1}
    # an interior column in the middle of a block column that is not the first of its node, where there is one
    wide = [b for b in range(len(t["bcol_node"])) if t["bcol_r0"][b] > 0 and t["bcol_width"][b] >= 3]
    b = wide[0] if wide else int(np.argmax(t["bcol_width"]))
    s = int(t["bcol_node"][b])
    mid = int(t["sptr"][s]) + int(t["bcol_r0"][b]) + int(t["bcol_width"][b]) // 2
    singles["middle of a block column"] = mid
    if name == "box5":
        assert wide, "the case is meant to have nodes that span several block columns"
    for what, j in singles.items():
        plan = f.updown_plan(_unit(n, var[j]))
        want = em.tree_path_plan(t, nb, [j])
        assert np.array_equal(plan, want), (what, plan, want)
        assert (np.diff(plan) > 0).all()
    assert np.array_equal(f.updown_plan(_unit(n, var[n - 1])), [len(t["bcol_node"]) - 1])
    assert f.updown_plan(_unit(n, var[mid]))[0] == b
    # several vectors on different branches: the first columns of the leaves
    leaves = sorted(set(range(nn)) - set(int(p) for p in t["sparent"]))
    firsts = [int(t["sptr"][s]) for s in leaves[:5]]
    assert len(firsts) >= 2
    W = sp.hstack([_unit(n, var[j]) for j in firsts], format="csc")
    assert np.array_equal(f.updown_plan(W), em.tree_path_plan(t, nb, firsts))
    # empty columns and k = 0 visit nothing
    assert len(f.updown_plan(sp.csc_matrix((n, 3)))) == 0 and len(f.updown_plan(sp.csc_matrix((n, 0)))) == 0


def test_malformed_and_inadmissible_columns_are_rejected():
    A, f, t, _, _ = _case("p2d12")
    n = f.n
    var = _var_of(t)
    L = f.lib
    plan = lambda k, ptr, row: L.spllt_hip_updown_plan(f.fkeep, k, api._ip(np.array(ptr, dtype=np.int32)),
                                                       api._ip(np.array(row, dtype=np.int32)), None, 0)
    upd = lambda k, ptr, row, val, sign=1: L.spllt_hip_updown(f.fkeep, k, api._ip(np.array(ptr, dtype=np.int32)),
                                                              api._ip(np.array(row, dtype=np.int32)),
                                                              api._dp(np.array(val, dtype=np.float64)), sign)
    # two variables that are not adjacent in L's structure: the first pivots of two different leaves
    nn = len(t["sparent"])
    leaves = sorted(set(range(nn)) - set(int(p) for p in t["sparent"]))
    i, j = sorted((int(var[t["sptr"][leaves[0]]]) + 1, int(var[t["sptr"][leaves[1]]]) + 1))
    for fn in (lambda: plan(1, [1, 3], [i, j]), lambda: upd(1, [1, 3], [i, j], [1.0, 1.0])):
        assert fn() == -10 and "admissible" in f.last_error()
    with pytest.raises(api.SplltError) as ei:
        f.updown_plan(sp.csc_matrix(([1.0, 1.0], ([i - 1, j - 1], [0, 0])), shape=(n, 1)))
    assert ei.value.flag == -10
    for fn in (lambda: plan(1, [1, 2], [n + 1]), lambda: upd(1, [1, 2], [n + 1], [1.0]),
               lambda: plan(1, [1, 2], [0])):
        assert fn() == -10 and "outside" in f.last_error()
    e = sp.tril(sp.coo_matrix(A), -1)
    a, b = int(e.row[0]) + 1, int(e.col[0]) + 1
    lo, hi = min(a, b), max(a, b)
    assert plan(1, [1, 3], [lo, hi]) > 0
    for fn in (lambda: plan(1, [1, 3], [hi, lo]), lambda: upd(1, [1, 3], [hi, lo], [1.0, 1.0]),
               lambda: plan(1, [1, 3], [lo, lo])):
        assert fn() == -10 and "increasing" in f.last_error()
    assert plan(-1, [1], [1]) == -10 and plan(1, [2, 1], [1]) == -10
    assert L.spllt_hip_updown_plan(f.fkeep, 1, None, None, None, 0) == -10
    assert L.spllt_hip_updown_plan(None, 0, None, None, None, 0) == -10
    assert upd(1, [1, 2], [1], [1.0], sign=0) == -10 and "sign" in f.last_error()
    assert upd(1, [1, 2], [1], [1.0], sign=2) == -10
    for v in (float("nan"), float("inf")):
        assert upd(1, [1, 2], [1], [v]) == -10 and "finite" in f.last_error()
    assert L.spllt_hip_updown(f.fkeep, 1, api._ip(np.array([1, 2], dtype=np.int32)),
                              api._ip(np.array([1], dtype=np.int32)), None, 1) == -10
    out = np.full(4, -1, dtype=np.int64)
    import ctypes as C
    assert L.spllt_hip_updown_info(f.fkeep, out.ctypes.data_as(C.POINTER(C.c_int64))) == 0 and (out == 0).all()
    assert L.spllt_hip_updown_info(f.fkeep, None) == -10


def test_update_without_a_device_or_a_factor():
    """no device: the no-device flag; with one: nothing has been factorized on the handle"""
    import torch
    A = matgen.poisson2d(10)
    f, val = make_case(A, nb=8)
    w = np.zeros(f.n)
    w[3] = 1.0
    with pytest.raises(api.SplltError) as ei:
        f.update(w)
    if torch.cuda.is_available():
        assert ei.value.flag == -10 and "factorized" in str(ei.value)
    else:
        assert ei.value.flag == -30
    f.close()


def test_partitioned_handle_is_unimplemented_without_a_device():
    A = matgen.poisson2d(32)
    f, val = make_case(A, nb=16, nemin=8, prune=True, ncpu=2)
    f.set_partition(0, 2)
    w = np.zeros(f.n)
    w[0] = 1.0
    with pytest.raises(api.SplltError) as ei:
        f.update(w)
    assert ei.value.flag == -98 and "partitioned" in f.last_error()
    f.close()


# ---- the recurrence ------------------------------------------------------------------------------
def _emulated(f, t, arena, W, sign):
    out = arena.copy()
    bad = em.updown(t, out, f.updown_plan(W), em.pivot_columns(t, W), sign)
    return out, bad


@pytest.mark.parametrize("k", [1, 3, 9])
@pytest.mark.parametrize("name", list(CASES))
def test_emulator_reproduces_the_dense_factor(name, k):
    A, f, t, L0, mask = _case(name)
    W = em.edge_columns(A, k, np.random.default_rng(100 + k))
    up, bad = _emulated(f, t, L0, W, +1)
    assert bad < 0
    want = dense_arena(f, A + W @ W.T)
    err_up = rel_err(up, want, mask)
    back, bad = _emulated(f, t, up, W, -1)
    assert bad < 0
    err_back = rel_err(back, L0, mask)
    print(name, k, "update", err_up, "update then downdate", err_back)
    assert err_up <= BAR and err_back <= BAR
    if name == "p2d12":            # the recurrence alone on the 12 x 12 grid: a few units of rounding
        assert err_up <= 6e-16 and err_back <= 6e-16
    # k vectors in one sweep are k successive rank-1 sweeps, bit for bit
    seq = L0.copy()
    for q in range(k):
        seq, _ = _emulated(f, t, seq, W[:, q], +1)
    assert np.array_equal(seq, up)
    # block columns outside the plan are untouched
    plan = set(f.updown_plan(W).tolist())
    for b in range(len(t["bcol_off"])):
        if b not in plan:
            sl = slice(int(t["bcol_off"][b]), int(t["bcol_off"][b]) + int(t["bcol_nrow"][b]) * int(t["bcol_width"][b]))
            assert np.array_equal(up[sl], L0[sl])


@pytest.mark.parametrize("name", list(CASES))
def test_emulator_on_a_fill_position(name):
    A, f, t, L0, mask = _case(name)
    W = em.fill_column(t, A)
    assert W is not None, "the case is meant to have fill"
    i, j = W.indices
    assert A[i, j] == 0
    up, bad = _emulated(f, t, L0, W, +1)
    err = rel_err(up, dense_arena(f, A + W @ W.T), mask)
    print(name, "fill position", err)
    assert bad < 0 and err <= BAR


def test_emulator_reports_a_failed_downdate():
    A, f, t, L0, mask = _case("p2d12")
    i = 17
    w = np.zeros(f.n)
    w[i] = np.sqrt(2.0 * A[i, i])
    out, bad = _emulated(f, t, L0, w, -1)
    assert bad >= int(t["order"][i]) and np.isfinite(out).all()
