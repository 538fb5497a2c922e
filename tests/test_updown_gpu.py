"""GPU tests of the low-rank update / downdate of the factor (spllt_hip_updown, updown.hip) on the small end of
tests/test_refine_gpu.py::CASES: ragged widths, one to twelve panels per block column, root block columns with
no rows below.  Bars: the project's L-parity bar (1e-12 relative to max|L|) against the CPU oracle's factor of the
modified values on the same handle (against a dense Cholesky for a fill position), the reference checker's
backward error (1e-14) for the solves, the tolerances of tests/test_selinv_gpu.py for the inverse and log det.

Largest errors observed on an MI355X (printed by the tests; the table in DESIGN.md section 14): 1.2e-15 for the
factor, 2.6e-16 for the solves, 4.2e-15 for diag(inv(A')), 7.2e-16 for the log det."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import updown_emulate as em
from helpers import bwd_err, dense_arena, lower_mask, make_case, oracle_factor, rel_err, sym_tables
from spllt_amd import api, matgen

pytestmark = pytest.mark.gpu

CASES = [
    ("p2d40-nb16", lambda: matgen.poisson2d(40), 16),
    ("box11-nb64", lambda: matgen.nd_like((11, 10, 9), 2), 64),
    ("p3d14-nb384", lambda: matgen.poisson3d(14), 384),
    ("fe27-nb768", lambda: matgen.fe27((7, 6, 6), 3), 768),
]
NAMES = [c[0] for c in CASES]
BAR = 1e-12


@functools.lru_cache(maxsize=None)
def _case(name):
    """A, a handle, the values, the symbolic tables, the lower mask, the oracle's factor of A"""
    _, gen, nb = next(c for c in CASES if c[0] == name)
    A = sp.csc_matrix(gen())
    f, val = make_case(A, nb=nb, nemin=16)
    o, rc = oracle_factor(f, val)
    assert rc == 0
    return A, f, val, sym_tables(f), lower_mask(f), o.arena().copy()


@functools.lru_cache(maxsize=None)
def _modified(name, k):
    """W (clique patterns, k columns), A' = A + W W^T, its values on the pattern of A, the oracle's factor of A'"""
    A, f, val, t, mask, L0 = _case(name)
    W = em.edge_columns(A, k, np.random.default_rng(7 * k + len(name)))
    A2 = sp.csc_matrix(A + W @ W.T)
    n2, ptr2, row2, val2 = api.csc_lower_1based(A2)
    assert np.array_equal(ptr2, f.ptr) and np.array_equal(row2, f.row)      # the pattern of A
    o, rc = oracle_factor(f, val2)
    assert rc == 0
    return W, A2, val2, o.arena().copy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _bcol(t, b):
    off, nr, w = int(t["bcol_off"][b]), int(t["bcol_nrow"][b]), int(t["bcol_width"][b])
    return slice(off, off + nr * w), nr, w


@pytest.mark.parametrize("k", [1, 2, 3, 9])       # (2: the kernels exist for 1, 2, 4 and 8 vectors per pass)
@pytest.mark.parametrize("name", NAMES)
def test_update_matches_the_oracle_factor_of_the_modified_matrix(name, k):
    A, f, val, t, mask, L0 = _case(name)
    W, A2, val2, L2 = _modified(name, k)
    f.factor(val).wait()
    assert rel_err(f.get_factor(), L0, mask) <= BAR
    f.update(W)
    err = rel_err(f.get_factor(), L2, mask)
    info = f.updown_info()
    print(name, k, "max|L - L_oracle| / max|L|", err, info)
    assert err <= BAR
    plan = f.updown_plan(W)
    assert info["bcols"] == len(plan) and info["passes"] == -(-k // 8) and info["launches"] > 0
    assert info["entries"] == sum(int(t["bcol_nrow"][b]) * int(t["bcol_width"][b]) for b in plan)
    assert f.updown_device_ms() > 0.0


@pytest.mark.parametrize("name", NAMES)
def test_solves_on_the_updated_factor(name):
    """solve, solve_many and solve_refined read the rebuilt inverses of the diagonal panels"""
    A, f, val, t, mask, L0 = _case(name)
    W, A2, val2, L2 = _modified(name, 9)
    f.factor(val).wait()
    f.update(W)
    rng = np.random.default_rng(3)
    B = np.asfortranarray(A2 @ rng.standard_normal((f.n, 40)))
    e1 = bwd_err(A2, f.solve(B[:, 0]), B[:, 0])
    X = f.solve_many(B)
    e40 = max(bwd_err(A2, X[:, q], B[:, q]) for q in range(40))
    xr, it, err = f.solve_refined(val2, B[:, :3], method="ir", tol=1e-14, max_iter=5)
    er = max(bwd_err(A2, xr[:, q], B[:, q]) for q in range(3))
    print(name, "backward errors: solve", e1, "solve_many", e40, "solve_refined", er, "iterations", it)
    assert e1 <= 1e-14 and e40 <= 1e-14 and er <= 1e-14 and f.refine_status == 0


@pytest.mark.parametrize("name", NAMES)
def test_update_on_a_fill_position(name):
    A, f, val, t, mask, L0 = _case(name)
    W = em.fill_column(t, A)
    assert W is not None
    i, j = W.indices
    assert A[i, j] == 0
    f.factor(val).wait()
    f.update(W)
    err = rel_err(f.get_factor(), dense_arena(f, A + W @ W.T), mask)
    print(name, "fill position", err)
    assert err <= BAR


@pytest.mark.parametrize("name", NAMES)
def test_downdate(name):
    A, f, val, t, mask, L0 = _case(name)
    W, A2, val2, L2 = _modified(name, 3)
    f.factor(val2).wait()
    f.update(W, downdate=True)
    e_down = rel_err(f.get_factor(), L0, mask)
    f.factor(val).wait()
    before = f.get_factor().copy()
    f.update(W)
    f.update(W, downdate=True)
    e_back = rel_err(f.get_factor(), before, mask)
    print(name, "downdate", e_down, "update then downdate", e_back)
    assert e_down <= BAR and e_back <= BAR


@pytest.mark.parametrize("name", NAMES)
def test_untouched_storage_is_bit_identical(name):
    A, f, val, t, mask, L0 = _case(name)
    inv = np.empty(f.n, dtype=np.int64)
    inv[t["order"]] = np.arange(f.n)
    # a column in the middle of a block column, below the root
    b = next(b for b in range(len(t["bcol_off"])) if t["bcol_width"][b] >= 3 and t["bcol_nrow"][b] > t["bcol_width"][b])
    s = int(t["bcol_node"][b])
    jloc = int(t["bcol_width"][b]) // 2
    j = int(t["sptr"][s]) + int(t["bcol_r0"][b]) + jloc
    w = np.zeros(f.n)
    w[inv[j]] = 0.8
    f.factor(val).wait()
    before = f.get_factor().copy()
    f.update(w)
    after = f.get_factor()
    plan = f.updown_plan(w)
    assert plan[0] == b
    for c in range(len(t["bcol_off"])):
        if c not in set(plan.tolist()):
            sl, _, _ = _bcol(t, c)
            assert np.array_equal(_bits(after[sl]), _bits(before[sl])), c
    sl, nr, wd = _bcol(t, b)
    m = mask[sl].reshape(nr, wd)[:, :jloc]
    assert np.array_equal(after[sl].reshape(nr, wd)[:, :jloc][m], before[sl].reshape(nr, wd)[:, :jloc][m])
    assert not np.array_equal(after[sl], before[sl])
    # no-ops: k = 0 and empty columns
    f.update(sp.csc_matrix((f.n, 0)))
    f.update(sp.csc_matrix((f.n, 2)))
    assert np.array_equal(_bits(f.get_factor()), _bits(after))


@pytest.mark.parametrize("name", ["p2d40-nb16", "box11-nb64"])
def test_two_deterministic_handles_agree_bit_for_bit(name):
    A, _, val, t, mask, L0 = _case(name)
    W9 = _modified(name, 9)[0]
    W3 = _modified(name, 3)[0]
    _, gen, nb = next(c for c in CASES if c[0] == name)
    out = []
    for rep in range(2):
        g, _ = make_case(A, nb=nb, nemin=16, engine_flags=4096)
        g.factor(val).wait()
        g.update(W9)
        g.update(W3, downdate=True)
        out.append(g.get_factor().copy())
        g.close()
    assert np.array_equal(out[0], out[1])


def test_failed_downdate_invalidates_the_factor_until_the_next_factorization():
    A, f, val, t, mask, L0 = _case("box11-nb64")
    i = 123
    w = np.zeros(f.n)
    w[i] = np.sqrt(2.0 * A[i, i])
    f.factor(val).wait()
    with pytest.raises(api.SplltError) as ei:
        f.update(w, downdate=True)
    assert ei.value.flag == -20 and "positive definite" in str(ei.value)
    b = A @ np.ones(f.n)
    for call in (lambda: f.solve(b), lambda: f.solve_many(b), lambda: f.get_factor(), lambda: f.log_det(),
                 lambda: f.solve_refined(val, b), lambda: f.update(w)):
        with pytest.raises(api.SplltError) as ei:
            call()
        assert ei.value.flag == -10, call
    f.factor(val).wait()
    assert rel_err(f.get_factor(), L0, mask) <= BAR
    assert bwd_err(A, f.solve(b), b) <= 1e-14


def test_selected_inverse_and_log_det_after_an_update():
    A, f, val, t, mask, L0 = _case("p2d40-nb16")
    W, A2, val2, L2 = _modified("p2d40-nb16", 3)
    f.factor(val).wait()
    f.selected_inverse()
    f.inverse_diag()
    f.update(W)
    for read in (f.get_inverse, f.inverse_diag, f.inverse_on_pattern):
        with pytest.raises(api.SplltError) as ei:
            read()
        assert ei.value.flag == -10 and "selected inverse" in str(ei.value)
    f.selected_inverse()
    Ainv = np.linalg.inv(A2.toarray())
    e_diag = float(np.abs(f.inverse_diag() - np.diag(Ainv)).max() / np.abs(np.diag(Ainv)).max())
    sign, ld = np.linalg.slogdet(A2.toarray())
    e_ld = abs(f.log_det() - ld) / max(1.0, abs(ld))
    print("diag(inv(A')) error", e_diag, "log det error", e_ld)
    assert e_diag <= 1e-11 and sign > 0 and e_ld <= 1e-12
    f.release_inverse()


def test_refactorization_after_an_update_replays_the_graph_as_before():
    A, _, val, t, mask, L0 = _case("p2d40-nb16")
    W, A2, val2, L2 = _modified("p2d40-nb16", 3)
    g, _ = make_case(A, nb=16, nemin=16, engine_flags=32768)     # HIP-graph replay, one chain of kernel nodes
    g.factor(val).wait()
    g.update(W)
    assert rel_err(g.get_factor(), L2, mask) <= BAR
    g.factor(val).wait()
    assert rel_err(g.get_factor(), L0, mask) <= BAR
    g.factor(val2).wait()
    assert rel_err(g.get_factor(), L2, mask) <= BAR
    g.close()


def test_a_rejected_call_leaves_the_arena_alone():
    A, f, val, t, mask, L0 = _case("box11-nb64")
    inv = np.empty(f.n, dtype=np.int64)
    inv[t["order"]] = np.arange(f.n)
    nn = len(t["sparent"])
    leaves = sorted(set(range(nn)) - set(int(p) for p in t["sparent"]))
    w = np.zeros(f.n)
    w[inv[t["sptr"][leaves[0]]]] = 1.0
    w[inv[t["sptr"][leaves[1]]]] = 1.0          # the first pivots of two leaves: not adjacent in L
    good = _modified("box11-nb64", 1)[0]
    f.factor(val).wait()
    before = f.get_factor().copy()
    with pytest.raises(api.SplltError) as ei:
        f.update(sp.hstack([good, sp.csc_matrix(w.reshape(-1, 1))], format="csc"))
    assert ei.value.flag == -10 and "admissible" in str(ei.value)
    assert np.array_equal(_bits(f.get_factor()), _bits(before))
    # a value that is not finite is a parameter error of an update as of a downdate, not a failed pivot
    bad = good.copy()
    bad.data[0] = np.nan
    for down in (False, True):
        with pytest.raises(api.SplltError) as ei:
            f.update(bad, downdate=down)
        assert ei.value.flag == -10 and "finite" in str(ei.value)
    assert np.array_equal(_bits(f.get_factor()), _bits(before))
    b = A @ np.ones(f.n)
    assert bwd_err(A, f.solve(b), b) <= 1e-14


def test_partitioned_handle_is_unimplemented():
    A = matgen.poisson2d(32)
    g, val = make_case(A, nb=16, nemin=8, prune=True, ncpu=2)
    g.set_partition(0, 2)
    w = np.zeros(g.n)
    w[0] = 1.0
    with pytest.raises(api.SplltError) as ei:
        g.update(w)
    assert ei.value.flag == -98
    g.close()
