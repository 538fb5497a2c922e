"""GPU tests of the low-rank update / downdate of the factors of a batch (spllt_hip_updown_batch, batch_updown.hip)
on the four cases of tests/test_updown_gpu.py: ragged widths, one to twelve panels per block column, root block
columns with no rows below.  Members from batch_emulate.member_values.  Bars: the project's L-parity bar (1e-12
relative to max|L|) against the CPU oracle's factor of the modified values on the same handle (a dense Cholesky for a
fill position), the reference checker's backward error (1e-14) for the solves, the tolerances of
tests/test_selinv_gpu.py for the inverse and log det.  Every test prints the largest value it saw (the table in
DESIGN.md section 28).

Largest errors observed on an MI355X: 1.2e-15 for the factors, 1.9e-16 for the solves, 1.0e-15 for the KKT residual
of the constrained solve, 4.3e-15 for diag(inv(A_b')), 9.6e-16 for the log det."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import updown_batch_emulate as bem
import updown_emulate as em
from batch_emulate import member_values
from helpers import bwd_err, dense_arena, lower_mask, make_case, oracle_factor, rel_err, sym_tables
from spllt_amd import _lib, api
from test_updown_gpu import CASES, NAMES

pytestmark = pytest.mark.gpu

BAR = 1e-12
NB = 3


@pytest.fixture(autouse=True)
def _hooks_off():
    yield
    lib = _lib.load()
    assert lib.spllt_hip_debug(b"batch_grid_limit=0") == 0
    assert lib.spllt_hip_debug(b"alloc_fail_at=0") == 0


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _bcol(t, b):
    off, nr, w = int(t["bcol_off"][b]), int(t["bcol_nrow"][b]), int(t["bcol_width"][b])
    return slice(off, off + nr * w)


@functools.lru_cache(maxsize=None)
def _case(name):
    """A, a handle, the tables, the lower mask"""
    _, gen, nb = next(c for c in CASES if c[0] == name)
    A = sp.csc_matrix(gen())
    f, _val = make_case(A, nb=nb, nemin=16)
    cols = np.repeat(np.arange(f.n), np.diff(f.ptr))
    return A, f, sym_tables(f), lower_mask(f), (np.asarray(f.row) - 1, cols)


@functools.lru_cache(maxsize=None)
def _member(name, b):
    """(A_b, its values, the oracle's factor of A_b)"""
    A, f, t, mask, _ = _case(name)
    Ab, vb = member_values(A, b, f.ptr, f.row)
    o, rc = oracle_factor(f, vb)
    assert rc == 0
    return sp.csc_matrix(Ab), np.ascontiguousarray(vb), o.arena().copy()


def _values_on_pattern(name, A2):
    rows, cols = _case(name)[4]
    return np.ascontiguousarray(np.asarray(sp.csc_matrix(A2)[rows, cols]).ravel())


@functools.lru_cache(maxsize=None)
def _pattern(name, k):
    A = _case(name)[0]
    return bem.canonical(em.edge_columns(A, k, np.random.default_rng(7 * k + len(name))))


def _scale(b):
    return 0.5 + 0.25 * (b % 5)


@functools.lru_cache(maxsize=None)
def _modified(name, k, b):
    """member b's values on the pattern of W (W's own, scaled), A_b' = A_b + W_b W_b^T, its values, the oracle's factor"""
    f = _case(name)[1]
    W = _pattern(name, k)
    wv = W.data * _scale(b)
    Wb = bem.member_matrix(W, wv)
    A2 = sp.csc_matrix(_member(name, b)[0] + Wb @ Wb.T)
    val2 = _values_on_pattern(name, A2)
    o, rc = oracle_factor(f, val2)
    assert rc == 0
    return wv, A2, val2, o.arena().copy()


def _factor_members(name, members):
    f = _case(name)[1]
    assert f.factor_batch(np.stack([_member(name, b)[1] for b in members])) == 0


def _wvals(name, k, members):
    return np.stack([_modified(name, k, b)[0] for b in members])


@pytest.mark.parametrize("k", [1, 2, 3, 9])
@pytest.mark.parametrize("name", NAMES)
def test_update_matches_the_oracle_factor_of_every_member(name, k):
    A, f, t, mask, _ = _case(name)
    members = list(range(NB))
    W = _pattern(name, k)
    _factor_members(name, members)
    s0 = f.lib.spllt_hip_factor_serial(f.fkeep, 1)
    assert f.update_batch(W, _wvals(name, k, members)) == 0
    assert f.lib.spllt_hip_factor_serial(f.fkeep, 1) == s0 + 1
    err = max(rel_err(f.get_factor_batch(i), _modified(name, k, b)[3], mask) for i, b in enumerate(members))
    info = f.updown_batch_info()
    print(name, k, "max|L_b - L_oracle| / max|L|", err, info)
    assert err <= BAR
    plan = f.updown_plan(W)
    assert info["bcols"] == len(plan) and info["passes"] == -(-k // 8)
    assert info["entries"] == sum(int(t["bcol_nrow"][b]) * int(t["bcol_width"][b]) for b in plan)
    assert info["served"] == NB and info["failed"] == 0
    # launches: per pass one scatter, per block column of the pass's plan one generate and, with rows below, one apply
    want = 0
    for cs, pplan in bem.passes(f, W):
        want += 1 + sum(1 + (int(t["bcol_nrow"][b]) > int(t["bcol_width"][b])) for b in pplan)
    assert info["launches"] == want
    assert f.updown_batch_device_ms() > 0.0


@pytest.mark.parametrize("nbatch", [1, 17])
@pytest.mark.parametrize("name", NAMES)
def test_update_with_one_and_with_seventeen_members(name, nbatch):
    A, f, t, mask, _ = _case(name)
    members = [b % 4 for b in range(nbatch)]            # (four distinct members, repeated)
    W = _pattern(name, 3)
    _factor_members(name, members)
    assert f.update_batch(W, _wvals(name, 3, members)) == 0
    err = max(rel_err(f.get_factor_batch(i), _modified(name, 3, b)[3], mask) for i, b in enumerate(members))
    print(name, nbatch, "max|L_b - L_oracle| / max|L|", err)
    assert err <= BAR and f.updown_batch_info()["served"] == nbatch


@pytest.mark.parametrize("name", NAMES)
def test_downdate_and_fill_position(name):
    A, f, t, mask, _ = _case(name)
    members = list(range(NB))
    W = _pattern(name, 3)
    wv = _wvals(name, 3, members)
    assert f.factor_batch(np.stack([_modified(name, 3, b)[2] for b in members])) == 0
    assert f.update_batch(W, wv, downdate=True) == 0
    e_down = max(rel_err(f.get_factor_batch(i), _member(name, b)[2], mask) for i, b in enumerate(members))
    _factor_members(name, members)
    before = [f.get_factor_batch(i).copy() for i in range(NB)]
    assert f.update_batch(W, wv) == 0 and f.update_batch(W, wv, downdate=True) == 0
    e_back = max(rel_err(f.get_factor_batch(i), before[i], mask) for i in range(NB))
    Wf = bem.canonical(em.fill_column(t, A))
    i, j = Wf.indices
    assert A[i, j] == 0
    _factor_members(name, members)
    fv = np.stack([Wf.data * _scale(b) for b in members])
    assert f.update_batch(Wf, fv) == 0
    e_fill = 0.0
    for i, b in enumerate(members):
        Wb = bem.member_matrix(Wf, fv[i])
        e_fill = max(e_fill, rel_err(f.get_factor_batch(i), dense_arena(f, _member(name, b)[0] + Wb @ Wb.T), mask))
    print(name, "downdate", e_down, "update then downdate", e_back, "fill position", e_fill)
    assert e_down <= BAR and e_back <= BAR and e_fill <= BAR


@pytest.mark.parametrize("name", NAMES)
def test_sweeps_over_the_batch_see_the_modified_factors(name):
    A, f, t, mask, _ = _case(name)
    n = f.n
    members = list(range(NB))
    W = _pattern(name, 9)
    _factor_members(name, members)
    Cr = np.ones((1, n))
    f.set_constraints_batch(Cr)                          # BEFORE the update: rebuilt on the next call
    assert f.selected_inverse_batch() == 0
    seeds = np.zeros((NB, f.sym_info()["arena"]))
    f.set_factor_adjoint_batch(seeds)
    assert f.update_batch(W, _wvals(name, 9, members)) == 0
    A2 = [_modified(name, 9, b)[1] for b in members]
    val2 = np.stack([_modified(name, 9, b)[2] for b in members])
    rng = np.random.default_rng(3)
    R = rng.standard_normal((n, 33))
    B33 = np.stack([(A2[i] @ R).T for i in range(NB)])             # (B, 33, n): crosses a block of 32
    x1 = f.solve_batch(B33[:, 0, :])
    e1 = max(bwd_err(A2[i], x1[i], B33[i, 0]) for i in range(NB))
    X = f.solve_many_batch(B33)
    e33 = max(bwd_err(A2[i], X[i, q], B33[i, q]) for i in range(NB) for q in range(33))
    xr, it, err = f.solve_refined_batch(val2, B33[:, :3, :], method="ir", tol=1e-14, max_iter=5)
    er = max(bwd_err(A2[i], xr[i, q], B33[i, q]) for i in range(NB) for q in range(3))
    print(name, "backward errors: solve_batch", e1, "solve_many_batch", e33, "solve_refined_batch", er, "iterations", it.max())
    assert e1 <= 1e-14 and e33 <= 1e-14 and er <= 1e-14 and f.refine_status == 0
    # the inverse is stale, the adjoint unseeded
    with pytest.raises(api.SplltError) as ei:
        f.get_inverse_batch(0)
    assert ei.value.flag == -10 and "selected inverse" in str(ei.value)
    with pytest.raises(api.SplltError) as ei:
        f.factor_adjoint_batch()
    assert ei.value.flag == -10
    # the constraints set before the update: C x = e and the KKT residual against A_b'
    xc, lam = f.solve_constrained_batch(B33[:, 0, :], multipliers=True)
    e_c = float(np.abs(xc.sum(axis=1)).max() / (n * np.abs(xc).max()))
    e_kkt = max(float(np.abs(A2[i] @ xc[i] + lam[i, 0] - B33[i, 0]).max() / np.abs(B33[i, 0]).max()) for i in range(NB))
    print(name, "constrained: |C x| / (n max|x|)", e_c, "KKT residual", e_kkt)
    assert e_c <= 1e-12 and e_kkt <= 1e-12
    f.release_constraints_batch()
    if name == "p2d40-nb16":
        ld = f.log_det_batch()
        assert f.selected_inverse_batch() == 0
        dg = f.inverse_diag_batch()
        e_ld = e_dg = 0.0
        for i in range(NB):
            D = A2[i].toarray()
            sign, want = np.linalg.slogdet(D)
            assert sign > 0
            e_ld = max(e_ld, abs(ld[i] - want) / max(1.0, abs(want)))
            di = np.diag(np.linalg.inv(D))
            e_dg = max(e_dg, float(np.abs(dg[i] - di).max() / np.abs(di).max()))
        print(name, "diag(inv(A_b')) error", e_dg, "log det error", e_ld)
        assert e_dg <= 1e-11 and e_ld <= 1e-12
    f.release_inverse_batch()
    f.release_factor_adjoint_batch()


def _arena_after(f, name, members, place, W, wv, solve=None):
    assert f.factor_batch(np.stack([_member(name, b)[1] for b in members])) == 0
    assert f.update_batch(W, wv) == 0
    out = [_bits(f.get_factor_batch(place)).copy()]
    if solve is not None:
        out.append(_bits(f.solve_batch(np.tile(solve, (len(members), 1)))[place]).copy())
    return out


@pytest.mark.parametrize("name", ["p2d40-nb16", "box11-nb64"])
def test_a_members_bits_do_not_depend_on_the_batch(name, monkeypatch):
    """the same member values at place 0 of nbatch = 1 and at places 0 and 16 of nbatch = 17 give identical arena
    bits after the same update, with several member ranges, in both grid orders, and (reproducible batch) identical
    solve_batch bits, which pins the rebuilt dinv"""
    A, f, t, mask, _ = _case(name)
    lib = f.lib
    W = _pattern(name, 3)
    T = 2                                               # the member under test
    others = [b % 4 for b in range(17)]
    m0, m16 = [T] + others[1:], others[:16] + [T]
    w1 = _wvals(name, 3, [T])
    w0, w16 = _wvals(name, 3, m0), _wvals(name, 3, m16)
    rhs = _member(name, T)[0] @ np.ones(f.n)
    prev = f.set_batch_reproducible(True)
    try:
        ref = _arena_after(f, name, [T], 0, W, w1, rhs)
        for got in (_arena_after(f, name, m0, 0, W, w0, rhs), _arena_after(f, name, m16, 16, W, w16, rhs)):
            assert all(np.array_equal(a, b) for a, b in zip(got, ref))
        for limit in (1, 5):                            # one member per launch, then a few
            assert lib.spllt_hip_debug(b"batch_grid_limit=%d" % limit) == 0
            got = _arena_after(f, name, m16, 16, W, w16, rhs)
            assert all(np.array_equal(a, b) for a, b in zip(got, ref)), limit
        assert lib.spllt_hip_debug(b"batch_grid_limit=0") == 0
        _, gen, nb = next(c for c in CASES if c[0] == name)
        for member_fast in ("0", "1"):                  # (read once per engine)
            monkeypatch.setenv("SPLLT_BATCH_MEMBER_FAST", member_fast)
            g, _ = make_case(A, nb=nb, nemin=16)
            try:
                g.set_batch_reproducible(True)
                got = _arena_after(g, name, m16, 16, W, w16, rhs)
                assert all(np.array_equal(a, b) for a, b in zip(got, ref)), member_fast
            finally:
                g.close()
    finally:
        f.set_batch_reproducible(prev)


@pytest.mark.parametrize("name", ["p2d40-nb16", "fe27-nb768"])
def test_nine_columns_in_one_call_equal_nine_calls(name):
    A, f, t, mask, _ = _case(name)
    members = list(range(NB))
    W = _pattern(name, 9)
    wv = _wvals(name, 9, members)
    prev = f.set_batch_reproducible(True)               # (both sweeps start from the same factor bits)
    try:
        _factor_members(name, members)
        start = [f.get_factor_batch(i).copy() for i in range(NB)]
        assert f.update_batch(W, wv) == 0
        one = [f.get_factor_batch(i).copy() for i in range(NB)]
        _factor_members(name, members)
        assert all(np.array_equal(_bits(f.get_factor_batch(i)), _bits(start[i])) for i in range(NB))
        for q in range(9):
            sl = slice(W.indptr[q], W.indptr[q + 1])
            assert f.update_batch(W[:, [q]], wv[:, sl]) == 0
        for i in range(NB):
            assert np.array_equal(f.get_factor_batch(i)[mask], one[i][mask])
    finally:
        f.set_batch_reproducible(prev)


@pytest.mark.parametrize("name", NAMES)
def test_identity_exits(name):
    A, f, t, mask, _ = _case(name)
    k = 3
    W = _pattern(name, k)
    nbc = len(t["bcol_off"])
    # leave-one-out: member b non-zero in column b % 3 only; member 3 all zero; member 4 not positive definite
    good = [0, 1, 2]
    vals = [_member(name, b)[1] for b in good] + [_member(name, 0)[1], _member(name, 1)[1].copy()]
    vals[4][f.ptr[5] - 1] = -1.0                         # a negative diagonal entry
    wv = np.zeros((5, W.nnz))
    wv[:3] = bem.leave_one_out(W, [_scale(b) for b in good], 3)
    wv[4] = W.data
    prev = f.set_batch_reproducible(True)
    try:
        assert f.factor_batch(np.stack(vals)) == -20
        assert list(f.batch_status()[0]) == [0, 0, 0, 0, -20]
        before = [f.get_factor_batch(i).copy() for i in range(5)]
        rhs = np.tile(A @ np.ones(f.n), (5, 1))
        x_before = f.solve_batch(rhs)
        assert f.update_batch(W, wv) == -20               # (member 4 is still flagged; the others are served)
        info = f.updown_batch_info()
        assert info["served"] == 4 and info["failed"] == 0
        worst = 0.0
        for i, b in enumerate(good):
            Wb = bem.member_matrix(W, wv[i])
            A2 = sp.csc_matrix(_member(name, b)[0] + Wb @ Wb.T)
            o, rc = oracle_factor(f, _values_on_pattern(name, A2))
            assert rc == 0
            after = f.get_factor_batch(i)
            worst = max(worst, rel_err(after, o.arena(), mask))
            own = set(f.updown_plan(W[:, [i % k]]).tolist())
            for c in range(nbc):
                if c not in own:
                    assert np.array_equal(_bits(after[_bcol(t, c)]), _bits(before[i][_bcol(t, c)])), (i, c)
        print(name, "leave-one-out max|L_b - L_oracle| / max|L|", worst)
        assert worst <= BAR
        for i in (3, 4):                                 # all zero; flagged
            assert np.array_equal(_bits(f.get_factor_batch(i)), _bits(before[i])), i
        x_after = f.solve_batch(rhs)
        assert np.array_equal(_bits(x_after[3]), _bits(x_before[3]))      # (the dinv slots of member 3 as well)
        assert np.array_equal(x_after[4], rhs[4])
    finally:
        f.set_batch_reproducible(prev)


@pytest.mark.parametrize("name", ["box11-nb64", "p3d14-nb384"])
def test_a_downdate_that_makes_one_member_indefinite(name):
    A, f, t, mask, _ = _case(name)
    members = list(range(NB))
    i = 123
    bad = 1
    W = sp.csc_matrix(([1.0], ([i], [0])), shape=(f.n, 1))
    wv = np.array([[0.1 * np.sqrt(_member(name, b)[0][i, i])] for b in members])
    wv[bad, 0] = 2.0 * np.sqrt(_member(name, bad)[0][i, i])
    _factor_members(name, members)
    assert f.update_batch(W, wv, downdate=True) == -20
    assert "positive definite" in f.last_error()
    # what the interpreter predicts for the member
    arenas = [_member(name, b)[2].copy() for b in members]
    want_flags, _ = bem.updown_batch(t, f, arenas, W, wv, -1)
    flags, cols = f.batch_status()
    assert list(flags) == [0, -20, 0] and want_flags[0] == want_flags[2] == 0
    assert int(cols[bad]) == want_flags[bad] > 0
    assert f.updown_batch_info()["failed"] == 1 and f.updown_batch_info()["served"] == NB
    worst = 0.0
    for b in (0, 2):
        Wb = bem.member_matrix(W, wv[b])
        o, rc = oracle_factor(f, _values_on_pattern(name, sp.csc_matrix(_member(name, b)[0] - Wb @ Wb.T)))
        assert rc == 0
        worst = max(worst, rel_err(f.get_factor_batch(b), o.arena(), mask))
    print(name, "others after one member failed", worst)
    assert worst <= BAR
    rhs = np.tile(A @ np.ones(f.n), (NB, 1))
    x = f.solve_batch(rhs)
    assert np.array_equal(x[bad], rhs[bad]) and not np.array_equal(x[0], rhs[0])
    assert np.isnan(f.log_det_batch()[bad])
    # a second call skips the member and still says -20
    assert f.update_batch(W, 0.5 * wv) == -20 and f.updown_batch_info()["served"] == NB - 1
    _factor_members(name, members)                       # revives it
    assert list(f.batch_status()[0]) == [0, 0, 0]
    assert max(rel_err(f.get_factor_batch(b), _member(name, b)[2], mask) for b in members) <= BAR


def test_refusals_leave_every_arena_and_the_single_factor_alone():
    name = "box11-nb64"
    A, f, t, mask, _ = _case(name)
    members = list(range(NB))
    f.factor(_member(name, 0)[1]).wait()
    single = f.get_factor().copy()
    _factor_members(name, members)
    before = [f.get_factor_batch(i).copy() for i in range(NB)]
    inv = np.empty(f.n, dtype=np.int64)
    inv[t["order"]] = np.arange(f.n)
    leaves = sorted(set(range(len(t["sparent"]))) - set(int(p) for p in t["sparent"]))
    w = np.zeros((f.n, 1))
    w[inv[t["sptr"][leaves[0]]]] = 1.0
    w[inv[t["sptr"][leaves[1]]]] = 1.0                   # the first pivots of two leaves: not adjacent in L
    good = _pattern(name, 1)
    Wbad = sp.hstack([good, sp.csc_matrix(w)], format="csc")
    with pytest.raises(api.SplltError) as ei:
        f.update_batch(Wbad)
    assert ei.value.flag == -10 and "admissible" in str(ei.value)
    nan = np.tile(good.data, (NB, 1))
    nan[2, 0] = np.nan
    for down in (False, True):
        with pytest.raises(api.SplltError) as ei:
            f.update_batch(good, nan, downdate=down)
        assert ei.value.flag == -10 and "finite" in str(ei.value)
    assert f.update_batch(sp.csc_matrix((f.n, 0))) == 0 and f.update_batch(sp.csc_matrix((f.n, 2))) == 0
    assert f.updown_batch_info()["launches"] == 0
    for i in range(NB):
        assert np.array_equal(_bits(f.get_factor_batch(i)), _bits(before[i]))
    assert np.array_equal(_bits(f.get_factor()), _bits(single))
    # no batch on the handle
    g, _ = make_case(A, nb=64, nemin=16)
    try:
        g.factor(_member(name, 0)[1]).wait()
        own = g.get_factor().copy()
        with pytest.raises(api.SplltError) as ei:
            g.update_batch(good, np.tile(good.data, (NB, 1)))
        assert ei.value.flag == -10 and "no batch" in str(ei.value)
        assert np.array_equal(_bits(g.get_factor()), _bits(own))
    finally:
        g.close()


def test_allocation_failures_keep_nothing():
    name = "p2d40-nb16"
    A, _, t, mask, _ = _case(name)
    g, _ = make_case(A, nb=16, nemin=16)
    lib = g.lib
    try:
        members = list(range(NB))
        W = _pattern(name, 3)
        wv = _wvals(name, 3, members)
        g.factor(_member(name, 0)[1]).wait()
        single = g.get_factor().copy()
        assert g.factor_batch(np.stack([_member(name, b)[1] for b in members])) == 0
        before = [g.get_factor_batch(i).copy() for i in range(NB)]
        failures = 0
        for k in range(1, 12):
            assert lib.spllt_hip_debug(b"alloc_fail_at=%d" % k) == 0
            try:
                try:
                    rc = g.update_batch(W, wv)
                except api.SplltError as e:
                    rc = e.flag
                    assert "memory" in g.last_error(), g.last_error()
                armed = lib.spllt_hip_debug(b"alloc_fail_armed")
            finally:
                assert lib.spllt_hip_debug(b"alloc_fail_at=0") == 0
            if armed == 1:                               # the call makes k - 1 allocations
                assert rc == 0
                break
            assert rc == -1, (k, rc)
            failures += 1
            assert all(v == 0 for v in g.updown_batch_info().values())
            for i in range(NB):
                assert np.array_equal(_bits(g.get_factor_batch(i)), _bits(before[i])), (k, i)
            assert np.array_equal(_bits(g.get_factor()), _bits(single))
        assert failures == 6, failures                   # work arrays, scratch, words; positions, entries, staged values
        err = max(rel_err(g.get_factor_batch(i), _modified(name, 3, b)[3], mask) for i, b in enumerate(members))
        assert err <= BAR
        assert np.array_equal(_bits(g.get_factor()), _bits(single))
        g.release_updown_batch()
        assert all(v == 0 for v in g.updown_batch_info().values())
    finally:
        g.close()
