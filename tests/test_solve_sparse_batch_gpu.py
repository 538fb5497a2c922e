"""GPU tests of the sparse right-hand-side solves of a batch (include/spllt_hip_solve_sparse_batch.h,
batch_solve_sparse.hip): the batch's own substitution program filtered to the paths of B's nonzeros and of the wanted
rows, every launch carrying all members.  Yardsticks: the library's unchanged blocked batch solve of the same B stored
densely (rtol = atol = 1e-12, the project's bar between two solves), the scaled backward error 1e-14, the single
handle's solve_sparse / gram per member (1e-12), dense inverses and B^T A_b^-1 B in numpy (1e-11 of the largest
entry).  Members: val_b = (1 + b/4) val with b/2 added to the diagonal entries.  Every test runs a second time with
spllt_hip_debug("solve_sparse_batch_poison=1"): the whole batch workspace is NaN wherever the plan does not reach."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from helpers import bwd_err, make_case
from spllt_amd import api
from test_solve_sparse_gpu import CASES, Case

pytestmark = pytest.mark.gpu

NAMES = ["p2d40-nb16", "box11-nb64"]
NBATCH = [1, 3, 5]
SENTINEL = -7.25e77


@pytest.fixture(autouse=True, params=[0, 1], ids=["plain", "poison"])
def poison(request):
    lib = api._lib.load()
    assert lib.spllt_hip_debug(b"solve_sparse_batch_poison=%d" % request.param) == 0
    yield request.param
    assert lib.spllt_hip_debug(b"solve_sparse_batch_poison=0") == 0


@functools.lru_cache(maxsize=None)
def _base(name):
    """the matrix, a factorized single handle and the column kinds of test_solve_sparse_gpu.py (a handle of its own)"""
    c = Case(name)
    cols = np.repeat(np.arange(c.n), np.diff(c.f.ptr))
    c.diag = np.flatnonzero(np.asarray(c.f.row) - 1 == cols)
    assert len(c.diag) == c.n
    return c


def member_val(c, b):
    v = (1.0 + b / 4.0) * c.val
    v[c.diag] += b / 2.0
    return v


@functools.lru_cache(maxsize=None)
def _member(name, b):
    """(A_b sparse, A_b dense, A_b^-1), computed once and never modified"""
    c = _base(name)
    Ab = sp.csc_matrix((1.0 + b / 4.0) * c.A + (b / 2.0) * sp.identity(c.n))
    Ad = Ab.toarray()
    Ainv = np.linalg.inv(Ad)
    Ainv.setflags(write=False)
    return Ab, Ad, Ainv


def new_batch(name, vals):
    c = _base(name)
    f, _ = make_case(c.A, nb=CASES[name][1], nemin=16)
    rc = f.factor_batch(np.ascontiguousarray(vals))
    return f, rc


@functools.lru_cache(maxsize=None)
def _batch(name, nbatch):
    """a handle of its own with members 0 .. nbatch - 1 factorized; shared by the tests that do not change the batch"""
    c = _base(name)
    f, rc = new_batch(name, np.stack([member_val(c, b) for b in range(nbatch)]))
    assert rc == 0
    return f


def canonical(B):
    B = sp.csc_matrix(B, copy=True)
    B.sum_duplicates()
    B.sort_indices()
    return B


def member_vals(B, nbatch):
    """member b's values on the pattern of B (canonical order): B's own times 1 + b / 2, every third sign flipped
    for the odd members"""
    flip = np.where(np.arange(B.nnz) % 3 == 2, -1.0, 1.0)
    return np.stack([B.data * (1.0 + b / 2.0) * (flip if b % 2 else 1.0) for b in range(nbatch)])


def member_dense(B, vals, b):
    return B.toarray() if vals is None else sp.csc_matrix((vals[b], B.indices, B.indptr), shape=B.shape).toarray()


@functools.lru_cache(maxsize=None)
def _full(name, nbatch, k, per_member):
    """B, its column kinds, the members' values (None: shared) and the library's unchanged blocked batch solve of
    the same B stored densely: computed once, shared, never modified"""
    c, f = _base(name), _batch(name, nbatch)
    B, cols = c.columns(k)
    B = canonical(B)
    vals = member_vals(B, nbatch) if per_member else None
    dense = np.stack([member_dense(B, vals, b).T for b in range(nbatch)])          # (nbatch, k, n)
    X = f.solve_many_batch(dense).transpose(0, 2, 1)                                # (nbatch, n, k)
    X.setflags(write=False)
    return B, cols, vals, X


@pytest.mark.parametrize("per_member", [False, True], ids=["shared", "own"])
@pytest.mark.parametrize("k", [1, 5, 16, 17, 33])
@pytest.mark.parametrize("nbatch", NBATCH)
@pytest.mark.parametrize("name", NAMES)
def test_parity_with_the_blocked_batch_solve(name, nbatch, k, per_member):
    c, f = _base(name), _batch(name, nbatch)
    B, cols, vals, ref = _full(name, nbatch, k, per_member)
    got = f.solve_sparse_batch(B, vals=vals)
    assert f.solve_sparse_batch_status == 0
    assert got.shape == (nbatch, c.n, k) and np.isfinite(got).all()
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-12)
    for b in range(nbatch):
        Ab = _member(name, b)[0]
        Bd = member_dense(B, vals, b)
        for q in range(k):
            if cols[q]:
                assert bwd_err(Ab, got[b, :, q], Bd[:, q]) <= 1e-14, (b, q)
            else:
                assert (got[b, :, q] == 0.0).all() and not np.signbit(got[b, :, q]).any()     # an empty column: +0.0
    fwd, _ = f.solve_sparse_plan(B[:, :min(k, 32)], job=1)
    unreached = np.setdiff1d(np.arange(c.nbc), fwd)
    assert len(unreached) > 0
    zero_pos = [int(c.t["sptr"][int(c.t["bcol_node"][u])]) + int(c.t["bcol_r0"][u]) for u in unreached[:6]]
    spread = np.linspace(0, c.n - 1, 40).astype(np.int64)
    for rows in ([c.var_of[cols[0][0]]], c.var_of[spread], c.var_of[zero_pos], [5, c.n - 1, 5, 5, 0]):
        part = f.solve_sparse_batch(B, rows=rows, vals=vals)
        assert part.shape == (nbatch, len(rows), k)
        np.testing.assert_allclose(part, got[:, np.asarray(rows)], rtol=1e-12, atol=1e-12)
    # the forward result where no path of the first group's columns arrives is an exact +0.0
    y = f.solve_sparse_batch(B[:, :min(k, 32)], rows=c.var_of[zero_pos], job=1,
                             vals=None if vals is None else vals[:, :B.indptr[min(k, 32)]])
    assert (y == 0.0).all() and not np.signbit(y).any()


@pytest.mark.parametrize("name", NAMES)
def test_per_member_against_the_single_handle(name):
    c, nbatch = _base(name), 3
    f = _batch(name, nbatch)
    B, cols = c.columns(17, seed=4)
    B = canonical(B)
    vals = member_vals(B, nbatch)
    rows = c.var_of[np.linspace(0, c.n - 1, 29).astype(np.int64)]
    X, Xr, G = f.solve_sparse_batch(B, vals=vals), f.solve_sparse_batch(B, rows=rows, vals=vals), f.gram_batch(B, vals=vals)
    g, _ = make_case(c.A, nb=CASES[name][1], nemin=16)
    for b in range(nbatch):
        g.factor(member_val(c, b)).wait()
        Bb = sp.csc_matrix((vals[b], B.indices, B.indptr), shape=B.shape)
        np.testing.assert_allclose(X[b], g.solve_sparse(Bb), rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(Xr[b], g.solve_sparse(Bb, rows=rows), rtol=1e-12, atol=1e-12)
        Gs = g.gram(Bb)
        assert np.abs(G[b] - Gs).max() <= 1e-12 * np.abs(Gs).max()
    g.close()


@pytest.mark.parametrize("nbatch", NBATCH)
@pytest.mark.parametrize("name", NAMES)
def test_jobs(name, nbatch):
    c, f = _base(name), _batch(name, nbatch)
    B, cols, vals, ref = _full(name, nbatch, 5, True)
    dense = np.stack([member_dense(B, vals, b).T for b in range(nbatch)])
    y = f.solve_sparse_batch(B, job=1, vals=vals)
    np.testing.assert_allclose(y, f.solve_many_batch(dense, job=1).transpose(0, 2, 1), rtol=1e-12, atol=1e-12)
    assert not np.allclose(y, ref)
    # the backward sweep of the members' forward results: one dense pattern, every member its own values
    Y = canonical(sp.csc_matrix(np.ones((c.n, 5))))
    yv = np.stack([y[b].T.ravel() for b in range(nbatch)])
    np.testing.assert_allclose(f.solve_sparse_batch(Y, job=2, vals=yv), ref, rtol=1e-12, atol=1e-12)
    rows = c.var_of[np.linspace(0, c.n - 1, 17).astype(np.int64)]
    np.testing.assert_allclose(f.solve_sparse_batch(Y, rows=rows, job=2, vals=yv), ref[:, rows], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(f.solve_sparse_batch(B, rows=rows, job=1, vals=vals), y[:, rows], rtol=1e-12, atol=1e-12)
    # job 2: entries of B at leaves cannot reach the last pivot, whose closure is the last block column
    E = sp.csc_matrix((np.ones(2), ([c.var_of[c.leaf_pos[0]], c.var_of[c.leaf_pos[1]]], [0, 1])), shape=(c.n, 2))
    z = f.solve_sparse_batch(E, rows=[c.var_of[c.n - 1]], job=2)
    assert z.shape == (nbatch, 1, 2) and (z == 0.0).all() and not np.signbit(z).any()
    info = f.solve_sparse_batch_info()
    assert info["bwd_bcols"] == 1 and info["fwd_bcols"] == 0 and info["served"] == nbatch and info["flagged"] == 0


def _gram_ref(name, B, vals, nbatch):
    out = []
    for b in range(nbatch):
        Bd = member_dense(B, vals, b)
        out.append(Bd.T @ (_member(name, b)[2] @ Bd))
    return np.stack(out)


def _check_gram(G, ref):
    assert G.shape == ref.shape and np.isfinite(G).all()
    for b in range(len(ref)):
        assert np.abs(G[b] - ref[b]).max() <= 1e-11 * np.abs(ref[b]).max(), b
        assert np.array_equal(G[b], G[b].T), b


@pytest.mark.parametrize("k", [1, 3, 16, 17, 33, 48])
@pytest.mark.parametrize("nbatch", NBATCH)
@pytest.mark.parametrize("name", NAMES)
def test_gram_batch(name, nbatch, k):
    import torch
    c, f = _base(name), _batch(name, nbatch)
    B, cols = c.columns(k, seed=k)
    B = canonical(B)
    for vals in (None, member_vals(B, nbatch)):
        G = f.gram_batch(B, vals=vals)
        assert f.solve_sparse_batch_status == 0
        _check_gram(G, _gram_ref(name, B, vals, nbatch))
        info = f.solve_sparse_batch_info()
        assert info["bwd_bcols"] == 0 and 0 < info["fwd_bcols"] and info["served"] == nbatch
    # ldg > k with sentinels in the padding and behind every member, host and device forms
    ldg = k + 3
    kk, ptr, row, v, ldb = f._sparse_batch_columns(B, vals, "test")
    buf = np.full((nbatch * k + 1) * ldg, SENTINEL)
    assert f.lib.spllt_hip_gram_sparse_batch(f.fkeep, kk, api._ip(ptr), api._ip(row), api._dp(v), ldb, api._dp(buf), ldg) == 0
    gd = torch.full(((nbatch * k + 1) * ldg,), SENTINEL, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    assert f.gram_batch_dev(B, gd.data_ptr(), ldg, vals=vals) == 0
    for img in (buf.reshape(nbatch * k + 1, ldg), gd.cpu().numpy().reshape(nbatch * k + 1, ldg)):
        assert (img[:, k:] == SENTINEL).all() and (img[nbatch * k:] == SENTINEL).all()
        for b in range(nbatch):
            blk = img[b * k:(b + 1) * k, :k]
            np.testing.assert_allclose(blk.T, G[b], rtol=1e-12, atol=1e-12 * np.abs(G[b]).max())   # (atomics in the sweeps)
            assert np.array_equal(blk, blk.T)


@pytest.mark.parametrize("nbatch", NBATCH)
def test_gram_batch_on_ranges_that_are_no_multiple_of_four(nbatch):
    name = "p2d40-nb16"
    c, f = _base(name), _batch(name, nbatch)
    found = None
    for p in c.leaf_pos:                                              # deterministic: the first leaf that qualifies
        E = sp.csc_matrix(([1.5], ([c.var_of[p]], [0])), shape=(c.n, 1))
        fwd, _ = f.solve_sparse_plan(E, rows=[], job=1)
        rg = c.touched_ranges(fwd)
        if sum(l for _, l in rg) % 4 and any(l % 4 for _, l in rg):
            found = (p, E, rg, fwd)
            break
    assert found, "no leaf whose reach has a row total and a range length that are no multiple of 4"
    p, E, rg, fwd = found
    q = rg[-1][0] + rg[-1][1] - 1
    B = canonical(sp.csc_matrix(([1.5, -0.75, 2.0, 1.25], ([c.var_of[p], c.var_of[q], c.var_of[p], c.var_of[q]],
                                                         [0, 1, 2, 2])), shape=(c.n, 3)))
    fwd3, _ = f.solve_sparse_plan(B, rows=[], job=1)
    assert np.array_equal(fwd3, fwd)
    for vals in (None, member_vals(B, nbatch)):
        _check_gram(f.gram_batch(B, vals=vals), _gram_ref(name, B, vals, nbatch))


@pytest.mark.parametrize("nbatch", NBATCH)
@pytest.mark.parametrize("name", NAMES)
def test_gram_batch_on_a_single_block_column(name, nbatch):
    c, f = _base(name), _batch(name, nbatch)
    v = c.var_of[c.n - 1]
    B = canonical(sp.csc_matrix(([2.0, -3.0], ([v, v], [0, 1])), shape=(c.n, 2)))
    fwd, _ = f.solve_sparse_plan(B, rows=[], job=1)
    assert list(fwd) == [c.nbc - 1] and len(c.touched_ranges(fwd)) == 1
    vals = member_vals(B, nbatch)
    _check_gram(f.gram_batch(B, vals=vals), _gram_ref(name, B, vals, nbatch))
    assert f.solve_sparse_batch_info()["fwd_bcols"] == 1


@pytest.mark.parametrize("nbatch", NBATCH)
@pytest.mark.parametrize("name", NAMES)
def test_inverse_block_batch(name, nbatch):
    c, f = _base(name), _batch(name, nbatch)
    i = c.var_of[[c.leaf_pos[0], c.leaf_pos[-1], c.mid_pos, c.n - 1, 7, c.n // 2, c.leaf_pos[0]]]
    j = c.var_of[[c.leaf_pos[1], c.n - 1, c.leaf_pos[0], c.mid_pos, c.n // 3]]
    got = f.inverse_block_batch(i, j)
    assert got.shape == (nbatch, len(i), len(j))
    for b in range(nbatch):
        Ainv = _member(name, b)[2]
        assert np.abs(got[b] - Ainv[np.ix_(i, j)]).max() <= 1e-11 * np.abs(Ainv).max()


@pytest.mark.parametrize("k", [5, 33])
@pytest.mark.parametrize("nbatch", [1, 3])
def test_device_entry_point_and_layout(nbatch, k):
    import torch
    name = "p2d40-nb16"
    c, f = _base(name), _batch(name, nbatch)
    B, cols, vals, ref = _full(name, nbatch, k, True)
    rows = c.var_of[np.linspace(0, c.n - 1, 23).astype(np.int64)]
    for sel, m in ((rows, len(rows)), (None, c.n)):
        ldx = m + 3
        ncol = nbatch * k
        xd = torch.full(((ncol + 2) * ldx,), SENTINEL, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        assert f.solve_sparse_batch_dev(B, xd.data_ptr(), ldx, rows=sel, vals=vals) == 0
        # the host entry point on a padded array
        nsel, selp = f._wanted(sel)
        kk, ptr, row, v, ldb = f._sparse_batch_columns(B, vals, "test")
        xh = np.full((ncol + 2) * ldx, SENTINEL)
        rc = f.lib.spllt_hip_solve_sparse_batch(f.fkeep, kk, api._ip(ptr), api._ip(row), api._dp(v), ldb, nsel,
                                                None if selp is None else api._ip(selp), api._dp(xh), ldx, 0)
        assert rc == 0, f.last_error()
        want = ref if sel is None else ref[:, sel]
        for img in (xd.cpu().numpy().reshape(ncol + 2, ldx), xh.reshape(ncol + 2, ldx)):
            assert (img[:, m:] == SENTINEL).all() and (img[ncol:] == SENTINEL).all()     # behind every member and column
            np.testing.assert_allclose(img[:ncol, :m].reshape(nbatch, k, m).transpose(0, 2, 1), want, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("bad", ["first", "last"])
@pytest.mark.parametrize("name", NAMES)
def test_flagged_members(name, bad):
    c, nbatch = _base(name), 3
    good = _batch(name, nbatch)
    vals_a = np.stack([member_val(c, b) for b in range(nbatch)])
    ib = 0 if bad == "first" else nbatch - 1
    vals_a[ib, c.diag[c.n // 2]] *= -1.0                               # one diagonal value negated
    f, rc = new_batch(name, vals_a)
    assert rc == -20
    B, cols = c.columns(17, seed=2)
    B = canonical(B)
    bv = member_vals(B, nbatch)
    rows = c.var_of[np.linspace(0, c.n - 1, 19).astype(np.int64)]
    others = [b for b in range(nbatch) if b != ib]
    for kw in (dict(), dict(rows=rows), dict(rows=rows, job=1)):
        X = f.solve_sparse_batch(B, vals=bv, **kw)
        assert f.solve_sparse_batch_status == -20 and "positive definite" in f.last_error()
        assert np.isnan(X[ib]).all()
        np.testing.assert_allclose(X[others], good.solve_sparse_batch(B, vals=bv, **kw)[others], rtol=1e-12, atol=1e-12)
        info = f.solve_sparse_batch_info()
        assert (info["served"], info["flagged"]) == (nbatch - 1, 1)
    G = f.gram_batch(B, vals=bv)
    assert f.solve_sparse_batch_status == -20 and np.isnan(G[ib]).all()
    Gg = good.gram_batch(B, vals=bv)
    for b in others:
        assert np.abs(G[b] - Gg[b]).max() <= 1e-12 * np.abs(Gg[b]).max()
    info = f.solve_sparse_batch_info()
    assert (info["served"], info["flagged"]) == (nbatch - 1, 1)
    f.close()


@pytest.mark.parametrize("name", NAMES)
def test_a_member_with_all_zero_values(name):
    c, nbatch = _base(name), 3
    f = _batch(name, nbatch)
    B, cols = c.columns(5)
    B = canonical(B)
    vals = member_vals(B, nbatch)
    vals[1] = 0.0
    X = f.solve_sparse_batch(B, vals=vals)
    assert (X[1] == 0.0).all() and not np.signbit(X[1]).any()
    G = f.gram_batch(B, vals=vals)
    assert (G[1] == 0.0).all()
    full = _full(name, nbatch, 5, True)[3]
    np.testing.assert_allclose(X[[0, 2]], full[[0, 2]], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("name", NAMES)
def test_launch_count_does_not_depend_on_the_number_of_members(name):
    c = _base(name)
    B, cols = c.columns(33)
    B = canonical(B)
    rows = c.var_of[np.linspace(0, c.n - 1, 32).astype(np.int64)]
    counts = {}
    for nbatch in (1, 5):
        f = _batch(name, nbatch)
        per = []
        for call in (lambda: f.solve_sparse_batch(B), lambda: f.solve_sparse_batch(B, rows=rows), lambda: f.gram_batch(B)):
            call()
            per.append(f.solve_sparse_batch_info()["launches"])
        counts[nbatch] = per
    assert counts[1] == counts[5] and min(counts[1]) > 0, counts


@pytest.mark.parametrize("name", NAMES)
def test_grid_split_into_member_ranges(name):
    c, nbatch = _base(name), 5
    f = _batch(name, nbatch)
    B, cols = c.columns(33)
    B = canonical(B)
    vals = member_vals(B, nbatch)
    rows = c.var_of[np.linspace(0, c.n - 1, 70).astype(np.int64)]
    X0, R0, G0 = f.solve_sparse_batch(B, vals=vals), f.solve_sparse_batch(B, rows=rows, vals=vals), f.gram_batch(B, vals=vals)
    l0 = f.solve_sparse_batch_info()["launches"]
    lib = api._lib.load()
    try:
        assert lib.spllt_hip_debug(b"batch_grid_limit=7") == 0        # ranges of a few members, of one member
        X1, R1, G1 = f.solve_sparse_batch(B, vals=vals), f.solve_sparse_batch(B, rows=rows, vals=vals), f.gram_batch(B, vals=vals)
        l1 = f.solve_sparse_batch_info()["launches"]
    finally:
        assert lib.spllt_hip_debug(b"batch_grid_limit=0") == 0
    assert l1 > l0
    np.testing.assert_allclose(X1, X0, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(R1, R0, rtol=1e-12, atol=1e-12)
    for b in range(nbatch):
        np.testing.assert_allclose(G1[b], G0[b], rtol=1e-12, atol=1e-12 * np.abs(G0[b]).max())
        assert np.array_equal(G1[b], G1[b].T)


@pytest.mark.parametrize("name", NAMES)
def test_restriction_is_real(name):
    c, nbatch = _base(name), 3
    f = _batch(name, nbatch)
    v = c.var_of[c.leaf_pos[0]]
    E = sp.csc_matrix(([1.0], ([v], [0])), shape=(c.n, 1))
    x = f.solve_sparse_batch(E, rows=[v])
    small = f.solve_sparse_batch_info()
    fwd, bwd = f.solve_sparse_plan(E, rows=[v])
    assert (small["fwd_bcols"], small["bwd_bcols"]) == (len(fwd), len(bwd))
    for b in range(nbatch):
        Ainv = _member(name, b)[2]
        assert abs(x[b, 0, 0] - Ainv[v, v]) <= 1e-11 * np.abs(Ainv).max()
    f.solve_sparse_batch(canonical(sp.csc_matrix(np.ones((c.n, 1)))))
    dense = f.solve_sparse_batch_info()
    assert dense["fwd_bcols"] == c.nbc and dense["bwd_bcols"] == c.nbc
    assert dense["fwd_entries"] == dense["bwd_entries"] == int((c.t["bcol_nrow"].astype(np.int64) * c.t["bcol_width"]).sum())
    for key in ("fwd_bcols", "bwd_bcols", "fwd_entries", "bwd_entries", "workgroups"):
        assert small[key] < dense[key], (key, small[key], dense[key])
    print(name, "leaf unit column, one entry:", small, "dense column, all entries:", dense)


def test_a_second_batch_and_an_update_are_picked_up():
    name, nbatch = "p2d40-nb16", 3
    c = _base(name)
    vals_a = np.stack([member_val(c, b) for b in range(nbatch)])
    f, rc = new_batch(name, vals_a)
    assert rc == 0
    B, cols = c.columns(5, seed=6)
    B = canonical(B)
    sel = [3, c.n - 1, 17]
    x1 = f.solve_sparse_batch(B, rows=sel)
    G1 = f.gram_batch(B)
    assert f.factor_batch(4.0 * vals_a) == 0
    np.testing.assert_allclose(f.solve_sparse_batch(B, rows=sel), x1 / 4.0, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(f.gram_batch(B), G1 / 4.0, rtol=1e-12, atol=1e-12 * np.abs(G1).max())
    assert f.factor_batch(4.0 * vals_a[:2]) == 0                       # fewer members: the outputs follow
    assert f.solve_sparse_batch(B, rows=sel).shape == (2, 3, 5)
    assert f.factor_batch(4.0 * vals_a) == 0
    w = sp.csc_matrix(([0.5, -0.5], ([0, 1], [0, 0])), shape=(c.n, 1))
    assert c.A[1, 0] != 0                                              # an existing entry: admissible
    assert f.update_batch(w) == 0
    x3 = f.solve_sparse_batch(B)
    Bd = B.toarray()
    for b in range(nbatch):
        A1 = sp.csc_matrix(4.0 * _member(name, b)[0] + w @ w.T)
        assert max(bwd_err(A1, x3[b][:, q], Bd[:, q]) for q in range(5) if cols[q]) <= 1e-14
    np.testing.assert_allclose(f.solve_sparse_batch(B, rows=sel), x3[:, sel], rtol=1e-12, atol=1e-12)
    f.close()


def test_other_features_are_undisturbed_and_release():
    name, nbatch = "box11-nb64", 3
    c = _base(name)
    f, rc = new_batch(name, np.stack([member_val(c, b) for b in range(nbatch)]))
    assert rc == 0
    f.factor(c.val).wait()
    R = np.random.default_rng(8).standard_normal((nbatch, 33, c.n))
    B, cols = c.columns(33, seed=9)
    B = canonical(B)
    many0, one0, single0 = f.solve_many_batch(R), f.solve_batch(R[:, 0]), f.solve_sparse(B)
    x0, G0 = f.solve_sparse_batch(B), f.gram_batch(B)
    np.testing.assert_allclose(f.solve_many_batch(R), many0, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(f.solve_batch(R[:, 0]), one0, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(f.solve_sparse(B), single0, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(x0[0], single0, rtol=1e-12, atol=1e-12)   # (member 0 has the single factor's values)
    f.release_solve_sparse_batch()
    f.release_solve_sparse_batch()
    np.testing.assert_allclose(f.solve_sparse_batch(B), x0, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(f.gram_batch(B), G0, rtol=1e-12, atol=1e-12 * np.abs(G0).max())
    np.testing.assert_allclose(f.solve_many_batch(R), many0, rtol=1e-12, atol=1e-12)
    f.release_batch()
    with pytest.raises(api.SplltError) as ei:
        f.solve_sparse_batch(B)
    assert ei.value.flag == -10 and "no batch" in str(ei.value)
    np.testing.assert_allclose(f.solve_sparse(B), single0, rtol=1e-12, atol=1e-12)
    f.close()


def test_refusals_and_noops():
    name, nbatch = "p2d40-nb16", 3
    c = _base(name)
    f, rc = new_batch(name, np.stack([member_val(c, b) for b in range(nbatch)]))
    assert rc == 0
    B, cols = c.columns(5)
    B = canonical(B)
    vals = member_vals(B, nbatch)
    k, ptr, row, v, ldb = f._sparse_batch_columns(B, vals, "test")
    ip, dp = api._ip, api._dp
    x = np.full(nbatch * k * c.n + 8, SENTINEL)
    sel = np.array([1, 2, 0], dtype=np.int32)
    solve, gram = f.lib.spllt_hip_solve_sparse_batch, f.lib.spllt_hip_gram_sparse_batch
    assert solve(f.fkeep, 0, ip(ptr), ip(row), dp(v), ldb, 2, ip(sel), dp(x), 2, 0) == 0          # k = 0
    assert solve(f.fkeep, k, ip(ptr), ip(row), dp(v), ldb, 0, ip(sel), dp(x), 0, 0) == 0          # nsel = 0
    assert gram(f.fkeep, 0, ip(ptr), ip(row), dp(v), ldb, dp(x), 0) == 0
    assert solve(f.fkeep, k, ip(ptr), ip(row), dp(v), ldb, 2, ip(sel), dp(x), 1, 0) == -10        # ldx < nsel
    assert "leading dimension" in f.last_error()
    assert solve(f.fkeep, k, ip(ptr), ip(row), dp(v), ldb - 1, 2, ip(sel), dp(x), 2, 0) == -10    # ldb too small
    assert "ldb" in f.last_error()
    assert gram(f.fkeep, k, ip(ptr), ip(row), dp(v), ldb - 1, dp(x), k) == -10 and "ldb" in f.last_error()
    assert gram(f.fkeep, k, ip(ptr), ip(row), dp(v), ldb, dp(x), k - 1) == -10 and "leading dimension" in f.last_error()
    assert (x == SENTINEL).all()
    assert f.solve_sparse_batch(B, rows=[]).shape == (nbatch, 0, 5) and f.solve_sparse_batch(B[:, :0]).shape == (nbatch, c.n, 0)
    # the reproducible batch: all four calls refuse, naming the switch, until it is off again
    import torch
    x_ok = f.solve_sparse_batch(B, vals=vals)
    xd = torch.full((nbatch * k * c.n,), SENTINEL, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    f.set_batch_reproducible(True)
    try:
        for call in (lambda: f.solve_sparse_batch(B, vals=vals), lambda: f.gram_batch(B, vals=vals),
                     lambda: f.solve_sparse_batch_dev(B, xd.data_ptr(), c.n, vals=vals),
                     lambda: f.gram_batch_dev(B, xd.data_ptr(), k, vals=vals)):
            with pytest.raises(api.SplltError) as ei:
                call()
            assert ei.value.flag == -98 and "spllt_hip_set_batch_reproducible" in str(ei.value)
    finally:
        f.set_batch_reproducible(False)
    assert (xd.cpu().numpy() == SENTINEL).all()
    np.testing.assert_allclose(f.solve_sparse_batch(B, vals=vals), x_ok, rtol=1e-12, atol=1e-12)
    f.close()


def test_partitioned_handle_returns_unimplemented():
    from spllt_amd import matgen
    g, _ = make_case(matgen.poisson2d(16), nb=16, nemin=8, prune=True, ncpu=2)
    g.set_partition(0, 2)
    E = sp.csc_matrix(([1.0], ([3], [0])), shape=(g.n, 1))
    for call in (lambda: g.solve_sparse_batch(E), lambda: g.gram_batch(E), lambda: g.inverse_block_batch([1], [2])):
        with pytest.raises(api.SplltError) as ei:
            call()
        assert ei.value.flag == -98 and "partitioned" in g.last_error()
    g.close()
