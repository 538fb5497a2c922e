"""GPU tests of the sparse right-hand-side solve (spllt_hip_solve_sparse*, spllt_hip_gram_sparse, solve_sparse.hip):
the substitution program filtered to the elimination-tree paths of B's nonzeros and of the wanted rows, on the
blocked kernels of solve_many.  Yardsticks: the library's own unchanged full solves (rtol = atol = 1e-12, the
bar between two solves of test_solve_many_gpu.py), the scaled backward error 1e-14, a dense inverse (1e-11 of
its largest entry, the bar of the selected inversion).  Every numerical test runs a second time with
spllt_hip_debug("solve_sparse_poison=1"): the workspace is NaN wherever the plan does not reach."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from helpers import bwd_err, make_case, sym_tables
from spllt_amd import api, matgen

pytestmark = pytest.mark.gpu

CASES = {
    "p2d40-nb16": (lambda: matgen.poisson2d(40), 16),
    "box11-nb64": (lambda: matgen.nd_like((11, 10, 9), 2), 64),
    "p3d14-nb384": (lambda: matgen.poisson3d(14), 384),
}
NAMES = list(CASES)
SENTINEL = -7.25e77


@pytest.fixture(params=[0, 1], ids=["plain", "poison"])
def poison(request):
    lib = api._lib.load()
    assert lib.spllt_hip_debug(b"solve_sparse_poison=%d" % request.param) == 0
    yield request.param
    assert lib.spllt_hip_debug(b"solve_sparse_poison=0") == 0


class Case:
    def __init__(self, name):
        gen, nb = CASES[name]
        self.A = gen()
        self.f, self.val = make_case(self.A, nb=nb, nemin=16)
        self.f.factor(self.val).wait()
        f, t = self.f, sym_tables(self.f)
        self.t, self.n, self.nb = t, f.n, nb
        self.nbc = len(t["bcol_off"])
        self.var_of = np.empty(f.n, dtype=np.int64)
        self.var_of[t["order"]] = np.arange(f.n)
        nn = len(t["sparent"])
        leaves = sorted(set(range(nn)) - set(int(p) for p in t["sparent"]))
        self.leaf_pos = [int(t["sptr"][s]) for s in leaves]          # first pivots of distinct leaves
        # the middle of a block column, one that is not the first of its node where the case has such a node
        multi = [s for s in range(nn) if t["node_bcol0"][s + 1] - t["node_bcol0"][s] >= 2]
        b = int(t["node_bcol0"][multi[0]]) + 1 if multi else int(np.argmax(t["bcol_width"]))
        s = int(t["bcol_node"][b])
        self.mid_pos = int(t["sptr"][s]) + int(t["bcol_r0"][b]) + int(t["bcol_width"][b]) // 2
        self.Ad = self.A.toarray()

    @functools.cached_property
    def Ainv(self):
        return np.linalg.inv(self.Ad)

    def columns(self, k, seed=0):
        """k columns of the kinds the issue lists, by pivot position, random values: unit columns at leaf first
        pivots, the last pivot, a mid-block-column pivot, two and three nonzeros across branches, one empty"""
        L, n = self.leaf_pos, self.n
        kinds = [[L[0]], [n - 1], [self.mid_pos], [L[1], L[-1]], [], [L[2], L[len(L) // 2], L[-2]]]
        few = max(1, len(L) // 3)                          # (the leaves behind stay outside every forward reach)
        cols = [kinds[q] if q < len(kinds) else [L[3 + (q - len(kinds)) % few]] for q in range(k)]
        rng = np.random.default_rng(seed)
        rows = [self.var_of[p] for c in cols for p in c]
        cidx = [q for q, c in enumerate(cols) for _ in c]
        vals = rng.uniform(0.5, 1.5, len(rows)) * rng.choice([-1.0, 1.0], len(rows))
        return sp.csc_matrix((vals, (rows, cidx)), shape=(n, k)), cols

    def touched_ranges(self, bcols):
        """maximal runs of the own columns of these block columns: (first pivot position, length)"""
        m = np.zeros(self.n + 1, dtype=bool)
        for b in bcols:
            s = int(self.t["bcol_node"][b])
            c0 = int(self.t["sptr"][s]) + int(self.t["bcol_r0"][b])
            m[c0:c0 + int(self.t["bcol_width"][b])] = True
        edge = np.flatnonzero(np.diff(np.concatenate([[False], m]).astype(np.int8)))
        return [(int(a), int(b - a)) for a, b in zip(edge[0::2], edge[1::2])]


@functools.lru_cache(maxsize=None)
def _case(name):
    return Case(name)


@functools.lru_cache(maxsize=None)
def _full(name, k):
    """the library's unchanged blocked solve of the same B stored densely: computed once, shared, never modified"""
    c = _case(name)
    B, cols = c.columns(k)
    X = c.f.solve_many(B.toarray()).reshape(c.n, k)
    X.setflags(write=False)
    return B, cols, X


@pytest.mark.parametrize("k", [1, 5, 16, 17, 32, 33])
@pytest.mark.parametrize("name", NAMES)
def test_parity_with_the_full_solve(name, k, poison):
    c = _case(name)
    B, cols, ref = _full(name, k)
    got = c.f.solve_sparse(B)
    assert got.shape == (c.n, k) and np.isfinite(got).all()
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-12)
    Bd = B.toarray()
    for q in range(k):
        if cols[q]:
            assert bwd_err(c.A, got[:, q], Bd[:, q]) <= 1e-14, q
        else:
            assert (got[:, q] == 0.0).all()              # an empty column: exact zeros
    fwd, _ = c.f.solve_sparse_plan(B[:, :min(k, 32)], job=1)
    unreached = np.setdiff1d(np.arange(c.nbc), fwd)
    assert len(unreached) > 0
    zero_pos = [int(c.t["sptr"][int(c.t["bcol_node"][b])]) + int(c.t["bcol_r0"][b]) for b in unreached[:6]]
    spread = np.linspace(0, c.n - 1, 40).astype(np.int64)
    for rows in ([c.var_of[cols[0][0]]], c.var_of[spread], c.var_of[zero_pos], [5, c.n - 1, 5, 5, 0]):
        part = c.f.solve_sparse(B, rows=rows)
        assert part.shape == (len(rows), k)
        np.testing.assert_allclose(part, got[np.asarray(rows)], rtol=1e-12, atol=1e-12)
    # the forward result where no path of the first group's columns arrives is an exact zero
    y = c.f.solve_sparse(B[:, :min(k, 32)], rows=c.var_of[zero_pos], job=1)
    assert (y == 0.0).all() and not np.signbit(y).any()


@pytest.mark.parametrize("name", NAMES)
def test_jobs(name, poison):
    c = _case(name)
    B, cols, ref = _full(name, 5)
    y = c.f.solve_sparse(B, job=1)
    np.testing.assert_allclose(y, c.f.solve(B.toarray(), job=1), rtol=1e-12, atol=1e-12)
    assert not np.allclose(y, ref)
    np.testing.assert_allclose(c.f.solve_sparse(y, job=2), ref, rtol=1e-12, atol=1e-12)
    rows = c.var_of[np.linspace(0, c.n - 1, 17).astype(np.int64)]
    np.testing.assert_allclose(c.f.solve_sparse(y, rows=rows, job=2), ref[rows], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(c.f.solve_sparse(B, rows=rows, job=1), y[rows], rtol=1e-12, atol=1e-12)
    # job 2: entries of B at leaves cannot reach the last pivot, whose closure is the last block column
    E = sp.csc_matrix((np.ones(2), ([c.var_of[c.leaf_pos[0]], c.var_of[c.leaf_pos[1]]], [0, 1])), shape=(c.n, 2))
    z = c.f.solve_sparse(E, rows=[c.var_of[c.n - 1]], job=2)
    assert (z == 0.0).all()
    assert c.f.solve_sparse_info()["bwd_bcols"] == 1 and c.f.solve_sparse_info()["fwd_bcols"] == 0


@pytest.mark.parametrize("k", [5, 33])
@pytest.mark.parametrize("name", ["p2d40-nb16", "p3d14-nb384"])
def test_device_entry_point_and_layout(name, k, poison):
    import torch
    c = _case(name)
    B, cols, ref = _full(name, k)
    rows = c.var_of[np.linspace(0, c.n - 1, 23).astype(np.int64)]
    for sel, m in ((rows, len(rows)), (None, c.n)):
        ldx = m + 3
        xd = torch.full(((k + 2) * ldx,), SENTINEL, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        c.f.solve_sparse_dev(B, xd.data_ptr(), ldx, rows=sel)
        img = xd.cpu().numpy().reshape(k + 2, ldx)
        assert (img[:k, m:] == SENTINEL).all() and (img[k:] == SENTINEL).all()
        want = ref if sel is None else ref[sel]
        np.testing.assert_allclose(img[:k, :m].T, want, rtol=1e-12, atol=1e-12)
        # the host entry point on a padded array
        nsel, selp = c.f._wanted(sel)
        kk, ptr, row, val = c.f._sparse_columns(B, "test")
        xh = np.full((k + 2) * ldx, SENTINEL)
        rc = c.f.lib.spllt_hip_solve_sparse(c.f.fkeep, kk, api._ip(ptr), api._ip(row), api._dp(val), nsel,
                                            None if selp is None else api._ip(selp), api._dp(xh), ldx, 0)
        assert rc == 0, c.f.last_error()
        himg = xh.reshape(k + 2, ldx)
        assert (himg[:k, m:] == SENTINEL).all() and (himg[k:] == SENTINEL).all()
        np.testing.assert_allclose(himg[:k, :m].T, want, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("name", NAMES)
def test_inverse_block(name, poison):
    c = _case(name)
    bar = 1e-11 * np.abs(c.Ainv).max()
    i = c.var_of[[c.leaf_pos[0], c.leaf_pos[-1], c.mid_pos, c.n - 1, 7, c.n // 2, c.leaf_pos[0]]]
    j = c.var_of[[c.leaf_pos[1], c.n - 1, c.leaf_pos[0], c.mid_pos, c.n // 3]]
    got = c.f.inverse_block(i, j)
    assert got.shape == (len(i), len(j))
    assert np.abs(got - c.Ainv[np.ix_(i, j)]).max() <= bar
    with pytest.raises(ValueError):                                   # a pair outside the pattern of L
        c.f.selected_inverse()
        c.f.inverse_entries(c.var_of[c.leaf_pos[0]], c.var_of[c.leaf_pos[-1]])
    # pairs inside the pattern (the entries of A are): the selected inversion's numbers
    Ac = sp.tril(c.A).tocoo()
    pick = np.linspace(0, Ac.nnz - 1, 12).astype(np.int64)
    ii, jj = Ac.row[pick], Ac.col[pick]
    Z = c.f.inverse_entries(ii, jj)
    blk = c.f.inverse_block(ii, jj)
    assert np.abs(np.diag(blk) - Z).max() <= bar
    c.f.release_inverse()


@pytest.mark.parametrize("k", [1, 3, 16, 17, 33])
@pytest.mark.parametrize("name", NAMES)
def test_gram(name, k, poison):
    c = _case(name)
    B, cols = c.columns(k, seed=k)
    G = c.f.gram(B)
    Bd = B.toarray()
    ref = Bd.T @ np.linalg.solve(c.Ad, Bd)
    assert G.shape == (k, k) and np.isfinite(G).all()
    assert np.abs(G - ref).max() <= 1e-11 * np.abs(ref).max()
    assert np.array_equal(G, G.T)
    info = c.f.solve_sparse_info()
    assert info["bwd_bcols"] == 0 and 0 < info["fwd_bcols"]
    # ldg > k with a sentinel in the padding and behind the last column
    ldg = k + 3
    kk, ptr, row, val = c.f._sparse_columns(B, "test")
    buf = np.full((k + 1) * ldg, SENTINEL)
    assert c.f.lib.spllt_hip_gram_sparse(c.f.fkeep, kk, api._ip(ptr), api._ip(row), api._dp(val), api._dp(buf), ldg) == 0
    img = buf.reshape(k + 1, ldg)
    assert (img[:k, k:] == SENTINEL).all() and (img[k:] == SENTINEL).all()
    np.testing.assert_allclose(img[:k, :k].T, G, rtol=1e-12, atol=1e-12 * np.abs(G).max())   # (atomics in the sweeps)
    assert np.array_equal(img[:k, :k], img[:k, :k].T)


def test_gram_ranges_that_are_no_multiple_of_four(poison):
    c = _case("p2d40-nb16")
    found = None
    for p in c.leaf_pos:                                              # deterministic: the first leaf that qualifies
        E = sp.csc_matrix(([1.5], ([c.var_of[p]], [0])), shape=(c.n, 1))
        fwd, _ = c.f.solve_sparse_plan(E, rows=[], job=1)
        rg = c.touched_ranges(fwd)
        if sum(l for _, l in rg) % 4 and any(l % 4 for _, l in rg):
            found = (p, E, rg)
            break
    assert found, "no leaf whose reach has a row total and a range length that are no multiple of 4"
    p, E, rg = found
    assert sum(l for _, l in rg) % 4 != 0 and any(l % 4 != 0 for _, l in rg)
    # two more columns inside the same reach: every product is over these ranges only
    q = rg[-1][0] + rg[-1][1] - 1
    B = sp.csc_matrix(([1.5, -0.75, 2.0, 1.25], ([c.var_of[p], c.var_of[q], c.var_of[p], c.var_of[q]], [0, 1, 2, 2])),
                      shape=(c.n, 3))
    fwd3, _ = c.f.solve_sparse_plan(B, rows=[], job=1)
    assert np.array_equal(fwd3, fwd)
    G = c.f.gram(B)
    Bd = B.toarray()
    ref = Bd.T @ np.linalg.solve(c.Ad, Bd)
    assert np.abs(G - ref).max() <= 1e-11 * np.abs(ref).max() and np.array_equal(G, G.T)


@pytest.mark.parametrize("name", NAMES)
def test_gram_on_a_single_block_column(name, poison):
    c = _case(name)
    v = c.var_of[c.n - 1]
    B = sp.csc_matrix(([2.0, -3.0], ([v, v], [0, 1])), shape=(c.n, 2))
    fwd, _ = c.f.solve_sparse_plan(B, rows=[], job=1)
    assert list(fwd) == [c.nbc - 1] and len(c.touched_ranges(fwd)) == 1
    G = c.f.gram(B)
    ref = B.toarray().T @ np.linalg.solve(c.Ad, B.toarray())
    assert np.abs(G - ref).max() <= 1e-11 * np.abs(ref).max() and np.array_equal(G, G.T)
    assert c.f.solve_sparse_info()["fwd_bcols"] == 1


@pytest.mark.parametrize("name", NAMES)
def test_restriction_is_real(name, poison):
    c = _case(name)
    v = c.var_of[c.leaf_pos[0]]
    E = sp.csc_matrix(([1.0], ([v], [0])), shape=(c.n, 1))
    x = c.f.solve_sparse(E, rows=[v])
    small = c.f.solve_sparse_info()
    fwd, bwd = c.f.solve_sparse_plan(E, rows=[v])
    assert (small["fwd_bcols"], small["bwd_bcols"]) == (len(fwd), len(bwd))
    assert abs(x[0, 0] - c.Ainv[v, v]) <= 1e-11 * np.abs(c.Ainv).max()
    c.f.solve_sparse(np.ones((c.n, 1)))
    dense = c.f.solve_sparse_info()
    assert dense["fwd_bcols"] == c.nbc and dense["bwd_bcols"] == c.nbc
    assert dense["fwd_entries"] == dense["bwd_entries"] == int((c.t["bcol_nrow"].astype(np.int64) * c.t["bcol_width"]).sum())
    for key in ("fwd_bcols", "bwd_bcols", "fwd_entries", "bwd_entries", "workgroups"):
        assert small[key] < dense[key], (key, small[key], dense[key])
    print(name, "leaf unit column, one entry:", small, "dense column, all entries:", dense)


def _small():
    A = matgen.nd_like((10, 10, 9), 2)
    f, val = make_case(A, nb=96, nemin=16)
    f.factor(val).wait()
    rng = np.random.default_rng(7)
    rows = rng.choice(f.n, 6, replace=False)
    B = sp.csc_matrix((rng.standard_normal(6), (rows, [0, 0, 1, 2, 2, 2])), shape=(f.n, 4))   # column 3 is empty
    return A, f, val, B


def test_refactorization_and_update_are_picked_up(poison):
    A, f, val, B = _small()
    sel = [3, f.n - 1, 17]
    x1 = f.solve_sparse(B, rows=sel)
    f.factor(4.0 * val).wait()
    x2 = f.solve_sparse(B, rows=sel)
    np.testing.assert_allclose(x2, x1 / 4.0, rtol=1e-12, atol=1e-12)
    w = sp.csc_matrix(([0.5, -0.5], ([0, 1], [0, 0])), shape=(f.n, 1))
    assert A[1, 0] != 0                                                # an existing entry: admissible
    f.update(w)
    A1 = sp.csc_matrix(4.0 * A + w @ w.T)
    ref = np.linalg.solve(A1.toarray(), B.toarray())
    x3 = f.solve_sparse(B)
    Bd = B.toarray()
    assert max(bwd_err(A1, x3[:, q], Bd[:, q]) for q in range(3)) <= 1e-14
    np.testing.assert_allclose(x3, ref, rtol=1e-10, atol=1e-11 * np.abs(ref).max())
    assert (x3[:, 3] == 0.0).all()
    np.testing.assert_allclose(f.solve_sparse(B, rows=sel), x3[sel], rtol=1e-12, atol=1e-12)
    f.close()


def test_other_features_are_undisturbed_and_release(poison):
    A, f, val, B = _small()
    R = A @ np.random.default_rng(8).standard_normal((f.n, 33))
    many0 = f.solve_many(R)
    f.selected_inverse()
    d0 = f.inverse_diag()
    x0 = f.solve_sparse(B)
    G0 = f.gram(B)
    np.testing.assert_allclose(f.solve_many(R), many0, rtol=1e-12, atol=1e-12)
    assert np.array_equal(f.inverse_diag(), d0)
    assert f.factor_batch(np.array([1.0, 2.0])[:, None] * val[None, :]) == 0
    xb = f.solve_batch(np.stack([R[:, 0], R[:, 0]]))
    np.testing.assert_allclose(f.solve_sparse(B), x0, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(xb[0], many0[:, 0], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(f.solve_batch(np.stack([R[:, 0], R[:, 0]]))[1], many0[:, 0] / 2.0, rtol=1e-12, atol=1e-12)
    f.release_solve_sparse()
    f.release_solve_sparse()
    np.testing.assert_allclose(f.solve_sparse(B), x0, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(f.gram(B), G0, rtol=1e-12, atol=1e-12 * np.abs(G0).max())
    np.testing.assert_allclose(f.solve_many(R), many0, rtol=1e-12, atol=1e-12)
    f.close()


def test_noops_and_errors(poison):
    A, f, val, B = _small()
    k, ptr, row, bv = f._sparse_columns(B, "test")
    x = np.full(4 * f.n, SENTINEL)
    sel = np.array([1, 2], dtype=np.int32)
    solve = f.lib.spllt_hip_solve_sparse
    assert solve(f.fkeep, 0, api._ip(ptr), api._ip(row), api._dp(bv), 2, api._ip(sel), api._dp(x), 2, 0) == 0   # k = 0
    assert solve(f.fkeep, k, api._ip(ptr), api._ip(row), api._dp(bv), 0, api._ip(sel), api._dp(x), 0, 0) == 0   # nsel = 0
    assert f.lib.spllt_hip_gram_sparse(f.fkeep, 0, api._ip(ptr), api._ip(row), api._dp(bv), api._dp(x), 0) == 0
    assert solve(f.fkeep, k, api._ip(ptr), api._ip(row), api._dp(bv), 2, api._ip(sel), api._dp(x), 1, 0) == -10  # ldx < nsel
    assert "leading dimension" in f.last_error()
    assert (x == SENTINEL).all()
    assert f.solve_sparse(B, rows=[]).shape == (0, 4) and f.solve_sparse(B[:, :0]).shape == (f.n, 0)
    g, v2 = make_case(A, nb=96, nemin=16)                              # nothing factorized
    with pytest.raises(api.SplltError) as ei:
        g.solve_sparse(B)
    assert ei.value.flag == -10 and "factorized" in g.last_error()
    g.close()
    f.close()


def test_partitioned_factor_returns_unimplemented(poison):
    import torch
    from helpers import drive_exchanges
    A = matgen.poisson2d(32)
    fs, bufs = [], []
    for r in range(2):
        f, val = make_case(A, nb=16, nemin=8, prune=True, ncpu=2)
        xb = torch.zeros(max(1, f.set_partition(r, 2)), dtype=torch.float64, device="cuda")
        f.set_exchange_buffer(xb.data_ptr())
        fs.append(f)
        bufs.append(xb)
    dval = torch.tensor(val, device="cuda")
    torch.cuda.synchronize()
    for f in fs:
        f.factor_dev(dval.data_ptr())
    drive_exchanges(fs, bufs)
    E = sp.csc_matrix(([1.0], ([3], [0])), shape=(fs[0].n, 1))
    for f in fs:
        f.wait()
        for call in (lambda: f.solve_sparse(E), lambda: f.gram(E), lambda: f.inverse_block([1], [2])):
            with pytest.raises(api.SplltError) as ei:
                call()
            assert ei.value.flag == -98 and "partitioned" in f.last_error()
    for f in fs:
        f.close()
