"""GPU tests of the batched factor products and samplers (spllt_hip_factor_mult_batch*, spllt_hip_sample_batch*,
spllt_hip_white_noise_batch_dev; batch_mult.hip).  Accuracy of every member against the dense factor rebuilt from
get_factor_batch(b), with the dot-product bound of tests/test_factor_mult_gpu.py; the relations with A_b and with
solve_batch at that file's tolerances; determinism by results only (np.array_equal).  The matrices are the small
ones of that file: the smallest at which each path of the kernels exists.  No test provokes a device fault: a
member that is not positive definite is a flagged member, which every kernel skips."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import batch_mult_ladder as ladder
from batch_mult_ladder import noise_reference as _noise
import capi_ladder
from helpers import make_case, sym_tables
from spllt_amd import _lib, api, matgen

pytestmark = pytest.mark.gpu

CASES = [
    ("p2d12-nb8", lambda: matgen.poisson2d(12), 8, 4),          # n = 144: block columns narrower than a 16-tile
    ("box11-nb64", lambda: matgen.nd_like((11, 10, 9), 2), 64, 16),   # n = 990
    ("p3d14-nb384", lambda: matgen.poisson3d(14), 384, 16),     # n = 2744: wide block columns, several strips
]
NAMES = [c[0] for c in CASES]
NBATCH = [1, 3, 5]
NVECS = [1, 17, 33]
NV = 33


def dense_factor(f, arena):
    """L of P A P^T (n x n, pivot order) and its stored pattern, from the arena through the sym tables (that of
    tests/test_factor_mult_gpu.py)"""
    t = sym_tables(f)
    n = f.n
    L, pat = np.zeros((n, n)), np.zeros((n, n), dtype=bool)
    for b in range(len(t["bcol_off"])):
        s = int(t["bcol_node"][b])
        rows = t["rlist"][t["rptr"][s]:t["rptr"][s + 1]]
        w, nr, off, r0 = int(t["bcol_width"][b]), int(t["bcol_nrow"][b]), int(t["bcol_off"][b]), int(t["bcol_r0"][b])
        c0 = int(t["sptr"][s]) + r0
        blk = arena[off:off + nr * w].reshape(nr, w).copy()
        low = np.ones((nr, w), dtype=bool)
        low[:w] = np.tril(low[:w])
        blk[~low] = 0.0
        L[np.ix_(rows[r0:r0 + nr], np.arange(c0, c0 + w))] = blk
        pat[np.ix_(rows[r0:r0 + nr], np.arange(c0, c0 + w))] = low
    return L, pat


class Case:
    def __init__(self, name):
        _, gen, nb, nemin = next(c for c in CASES if c[0] == name)
        self.name, self.A = name, sp.csc_matrix(gen())
        self.f, self.val = make_case(self.A, nb=nb, nemin=nemin)
        f = self.f
        self.n = f.n
        self.diag = np.array([f.ptr[j] - 1 for j in range(f.n)])
        assert (f.row[self.diag] == np.arange(1, f.n + 1)).all()
        self.order = f.sym("order")
        X = np.random.default_rng(0).standard_normal((5, NV, f.n))
        X.setflags(write=False)
        self.X = X

    def values(self, nbatch, bad=None):
        """member b: (1 + 0.1 b) val plus 0.05 b on the diagonal: diagonally dominant, distinct factors; `bad`: that
        member gets one negative diagonal entry, as in tests/test_factor_batch_gpu.py"""
        vals = np.stack([(1 + 0.1 * b) * self.val for b in range(nbatch)])
        for b in range(nbatch):
            vals[b, self.diag] += 0.05 * b
        if bad is not None:
            vals[bad, self.diag[self.n // 2]] *= -1.0
        return vals

    def member(self, b):
        return ((1 + 0.1 * b) * self.A + 0.05 * b * sp.identity(self.n)).tocsc()

    def batch(self, nbatch, bad=None):
        """the handle's last batch becomes this one; returns the return code of factor_batch"""
        return self.f.factor_batch(self.values(nbatch, bad))


@functools.lru_cache(maxsize=None)
def _case(name):
    return Case(name)


def reference(c, L, X, job):
    """X: (nvec, n) in user order.  (want, size): the product (nvec, n) and sum |.| |.| of what was added up"""
    Xp = np.empty((c.n, X.shape[0]))
    Xp[c.order] = X.T
    if job == 1:
        y, s = L @ Xp, np.abs(L) @ np.abs(Xp)
    elif job == 2:
        y, s = L.T @ Xp, np.abs(L.T) @ np.abs(Xp)
    else:
        y, s = L @ (L.T @ Xp), np.abs(L) @ (np.abs(L.T) @ np.abs(Xp))
    return y[c.order].T, s[c.order].T


def check_accuracy(c, members, nbatch, tag):
    """every job and nvec for the given members of the current batch of nbatch"""
    f = c.f
    dense = {b: dense_factor(f, f.get_factor_batch(b)) for b in members}
    for job in (0, 1, 2):
        for nvec in NVECS:
            X = c.X[:nbatch, :nvec]
            got = f.factor_mult_batch(X if nvec > 1 else X[:, 0], job).reshape(nbatch, nvec, c.n)
            for b in members:
                L, pat = dense[b]
                assert np.isfinite(got[b]).all()
                want, size = reference(c, L, X[b], job)
                # the dot-product bound with the longest row of L (stored entries); job 0 is two such products in a row
                n_terms = int(pat.sum(axis=1).max())
                bound = 64 * n_terms * 2.0 ** -53 * float(size.max())
                err = float(np.abs(got[b] - want).max())
                print(tag, c.name, "nbatch", nbatch, "member", b, "job", job, "nvec", nvec, "n_terms", n_terms,
                      "max|got - want|", err, "bound", bound)
                assert err <= bound


@pytest.mark.parametrize("nbatch", NBATCH)
@pytest.mark.parametrize("name", NAMES)
def test_accuracy(name, nbatch):
    c = _case(name)
    assert c.batch(nbatch) == 0
    check_accuracy(c, range(nbatch), nbatch, "accuracy")


@pytest.mark.parametrize("name", NAMES)
def test_relations(name):
    c = _case(name)
    f, nbatch = c.f, 3
    assert c.batch(nbatch) == 0
    X = c.X[:nbatch, :5]
    Y0 = f.factor_mult_batch(X, 0)
    for b in range(nbatch):
        want = (c.member(b) @ X[b].T).T
        np.testing.assert_allclose(Y0[b], want, rtol=1e-12, atol=1e-12 * np.abs(want).max())
    for job in (0, 1, 2):
        np.testing.assert_allclose(f.solve_batch(f.factor_mult_batch(X, job), job), X, rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(f.factor_mult_batch(f.solve_batch(X, job), job), X, rtol=1e-9, atol=1e-9)


def _padded(X, ldx, sentinel=-7.25e77):
    """(B * nvec + 2, ldx) image of X (B, nvec, n): padding behind every vector and two spare rows behind the last
    member (the C layout has no room between the members)"""
    B, nvec, n = X.shape
    img = np.full((B * nvec + 2, ldx), sentinel)
    img[:B * nvec, :n] = X.reshape(B * nvec, n)
    return img


@pytest.mark.parametrize("name", NAMES)
def test_bits(name):
    import torch
    c = _case(name)
    f, nbatch, n = c.f, 3, c.n
    assert c.batch(nbatch) == 0
    X = c.X[:nbatch]
    lib = f.lib
    for job in (0, 1, 2):
        y = f.factor_mult_batch(X, job)
        assert np.array_equal(f.factor_mult_batch(X, job), y)                      # two calls
        assert np.array_equal(f.factor_mult_batch(X[:, :17], job), y[:, :17])      # a block of 17
        for q in (0, 16, 32):                                                      # alone
            assert np.array_equal(f.factor_mult_batch(X[:, q], job), y[:, q]), (job, q)
        perm = np.random.default_rng(1).permutation(NV)
        assert np.array_equal(f.factor_mult_batch(X[:, perm], job), y[:, perm])
        # the other members' vectors do not matter
        X2 = X.copy()
        X2[0], X2[2] = 3.0 * X[2], -X[0]
        assert np.array_equal(f.factor_mult_batch(X2, job)[1], y[1])
        # blocks of 16 only (what is left when the workspaces of 32 do not fit)
        f.release_factor_mult_batch()
        assert lib.spllt_hip_debug(b"fmult_alloc_fail=1") == 0
        try:
            y16 = f.factor_mult_batch(X, job)
        finally:
            assert lib.spllt_hip_debug(b"fmult_alloc_fail=0") == 0
        assert np.array_equal(y16, y)
        # after a release the storage is taken again, blocks of 32 again
        f.release_factor_mult_batch()
        assert np.array_equal(f.factor_mult_batch(X, job), y)
        # member ranges: one member per launch
        assert lib.spllt_hip_debug(b"batch_grid_limit=1") == 0
        try:
            yr = f.factor_mult_batch(X, job)
        finally:
            assert lib.spllt_hip_debug(b"batch_grid_limit=0") == 0
        assert np.array_equal(yr, y)
        # host (padded), device (padded), device in pivot order
        nvec, ldx = 5, n + 7
        want = y[:, :nvec]
        img = _padded(X[:, :nvec], ldx)
        xh = img.copy()
        assert lib.spllt_hip_factor_mult_batch(f.fkeep, nvec, xh.ctypes.data, ldx, job) == 0, f.last_error()
        assert np.array_equal(xh[:, n:], img[:, n:]) and np.array_equal(xh[nbatch * nvec:], img[nbatch * nvec:])
        assert np.array_equal(xh[:nbatch * nvec, :n].reshape(nbatch, nvec, n), want)
        xd = torch.tensor(img, device="cuda")
        torch.cuda.synchronize()
        assert f.factor_mult_batch_dev(xd.data_ptr(), nvec, ldx=ldx, job=job) == 0
        dimg = xd.cpu().numpy()
        assert np.array_equal(dimg[:, n:], img[:, n:]) and np.array_equal(dimg[nbatch * nvec:], img[nbatch * nvec:])
        assert np.array_equal(dimg[:nbatch * nvec, :n].reshape(nbatch, nvec, n), want)
        pimg = img.copy()
        pimg[:nbatch * nvec, c.order] = img[:nbatch * nvec, :n]
        pd_ = torch.tensor(pimg, device="cuda")
        torch.cuda.synchronize()
        assert f.factor_mult_batch_dev(pd_.data_ptr(), nvec, ldx=ldx, job=job, pivot_order=True) == 0
        got = pd_.cpu().numpy()
        assert np.array_equal(got[:, n:], img[:, n:])
        assert np.array_equal(got[:nbatch * nvec, c.order].reshape(nbatch, nvec, n), want)
    # nvec = 0 is a no-op
    x = np.full(n, 3.0)
    assert lib.spllt_hip_factor_mult_batch(f.fkeep, 0, x.ctypes.data, n, 0) == 0 and (x == 3.0).all()


@pytest.mark.parametrize("name", NAMES)
def test_poison(name):
    c = _case(name)
    f, nbatch = c.f, 3
    assert c.batch(nbatch) == 0
    X = c.X[:nbatch, :17]
    want = [f.factor_mult_batch(X, job) for job in (0, 1, 2)]
    assert f.lib.spllt_hip_debug(b"fmult_poison=1") == 0
    try:
        got = [f.factor_mult_batch(X, job) for job in (0, 1, 2)]
    finally:
        assert f.lib.spllt_hip_debug(b"fmult_poison=0") == 0
    for g, w in zip(got, want):
        assert np.isfinite(g).all() and np.array_equal(g, w)


@pytest.mark.parametrize("nbatch,bad", [(3, 1), (5, 4)])
@pytest.mark.parametrize("name", NAMES)
def test_failed_member(name, nbatch, bad):
    import torch
    c = _case(name)
    f, n = c.f, c.n
    assert c.batch(nbatch, bad) == -20
    X = c.X[:nbatch, :17]
    for job in (0, 1, 2):
        x = X.copy()
        rc = f.lib.spllt_hip_factor_mult_batch(f.fkeep, 17, x.ctypes.data, n, job)
        assert rc == -20 and "spllt_hip_factor_mult_batch: " in f.last_error() and "unchanged" in f.last_error()
        assert np.array_equal(x[bad], X[bad])
        assert np.array_equal(f.factor_mult_batch(X, job)[bad], X[bad])         # (Python: no exception)
        xd = torch.tensor(X, device="cuda")
        torch.cuda.synchronize()
        assert f.factor_mult_batch_dev(xd.data_ptr(), 17, job=job) == -20
        assert np.array_equal(xd.cpu().numpy()[bad], X[bad])
    good = [b for b in range(nbatch) if b != bad]
    Z = f.white_noise_batch(4, seed=3)
    assert np.isnan(Z[bad]).all() and np.isfinite(Z[good]).all()
    m = np.ones(n)
    for kind in ("precision", "covariance"):
        S = f.sample_batch(4, seed=3, kind=kind, mean=m)
        assert np.isnan(S[bad]).all() and np.isfinite(S[good]).all()
        x = np.zeros((nbatch, 4, n))
        rc = f.lib.spllt_hip_sample_batch(f.fkeep, 4, x.ctypes.data, n, f._sample_kind(kind), 3, 0, 0, 1, None, 0)
        assert rc == -20 and "spllt_hip_sample_batch: " in f.last_error() and "NaN" in f.last_error()
    check_accuracy(c, good, nbatch, "failed member %d" % bad)
    assert c.batch(nbatch) == 0                       # the handle is still good
    assert np.isfinite(f.sample_batch(2, kind="covariance")).all()


# ---- noise and sampling ---------------------------------------------------------------------------
def _ulps(a, b):
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


def test_white_noise():
    c = _case("box11-nb64")
    f, n, nbatch = c.f, c.n, 3
    assert c.batch(nbatch) == 0
    for seed, first, stream0 in ((7, 0, 0), ((1 << 40) + 12345, (1 << 33) + 1, 4000000000)):
        Z = f.white_noise_batch(5, seed=seed, first_sample=first, stream0=stream0)
        assert Z.shape == (nbatch, n, 5)
        for b in range(nbatch):
            worst = float(_ulps(Z[b], _noise(n, 5, seed, (stream0 + b) & 0xFFFFFFFF, first)).max())
            print("noise of stream", stream0 + b, "against numpy Philox4x32-10 + Box-Muller: worst", worst, "ulp")
            assert worst <= 4
        assert not np.array_equal(Z[0], Z[1]) and not np.array_equal(Z[1], Z[2])
        assert np.array_equal(Z, f.white_noise_batch(5, seed=seed, first_sample=first, stream0=stream0))
        assert np.array_equal(Z[:, :, 2:5], f.white_noise_batch(3, seed=seed, first_sample=first + 2, stream0=stream0))
        # member b of a batch that starts at stream0 + 1 is member b + 1 of this one
        assert np.array_equal(f.white_noise_batch(5, seed=seed, first_sample=first, stream0=stream0 + 1)[:2], Z[1:])
    # common random numbers: every member gets stream0's noise, and stream 0 is the noise of the single handle
    Zc = f.white_noise_batch(5, seed=7, common_noise=True)
    f.factor(c.val).wait()
    single = f.white_noise(5, seed=7)
    for b in range(nbatch):
        assert np.array_equal(Zc[b], single)
    assert np.array_equal(f.white_noise_batch(5, seed=7)[0], single)
    assert not np.array_equal(f.white_noise_batch(5, seed=8)[0], single)


@pytest.mark.parametrize("name", NAMES)
def test_sampling_identities(name):
    import torch
    c = _case(name)
    f, n, nbatch, ns = c.f, c.n, 3, 35
    assert c.batch(nbatch) == 0
    rng = np.random.default_rng(4)
    m1, mB = rng.standard_normal(n), rng.standard_normal((nbatch, n))
    for common in (False, True):
        Z = f.white_noise_batch(ns, seed=11, common_noise=common)       # (B, n, ns), pivot order
        Zu = np.ascontiguousarray(Z[:, c.order, :].transpose(0, 2, 1))   # the noise laid out in user positions
        zd = torch.tensor(Zu, device="cuda")
        torch.cuda.synchronize()
        assert f.factor_mult_batch_dev(zd.data_ptr(), ns, job=1) == 0
        LZ = zd.cpu().numpy()
        kw = dict(seed=11, kind="covariance", common_noise=common)
        assert np.array_equal(f.sample_batch(ns, **kw), LZ)
        assert np.array_equal(f.sample_batch(ns, mean=m1, **kw), m1[None, None, :] + LZ)
        xc = f.sample_batch(ns, mean=mB, **kw)
        assert np.array_equal(xc, mB[:, None, :] + LZ)
        assert np.array_equal(f.sample_batch(3, mean=mB, first_sample=20, **kw), xc[:, 20:23])
        # the device entry point, padded, per-member mean with a stride
        ldx, ldm = n + 3, n + 5
        xd = torch.full((nbatch * ns + 1, ldx), -7.25e77, dtype=torch.float64, device="cuda")
        md = torch.zeros((nbatch, ldm), dtype=torch.float64, device="cuda")
        md[:, :n] = torch.tensor(mB, device="cuda")
        torch.cuda.synchronize()
        assert f.sample_batch_dev(xd.data_ptr(), ns, ldx=ldx, mean_dev_ptr=md.data_ptr(), ldmean=ldm, **kw) == 0
        img = xd.cpu().numpy()
        assert np.array_equal(img[:nbatch * ns, :n].reshape(nbatch, ns, n), xc)
        assert (img[:, n:] == -7.25e77).all() and (img[nbatch * ns] == -7.25e77).all()
        # precision: the backward sweep of the batch solve
        xp = f.sample_batch(ns, seed=11, kind="precision", mean=mB, common_noise=common)
        want = mB[:, None, :] + f.solve_batch(Zu, job=2)
        np.testing.assert_allclose(xp, want, rtol=1e-12, atol=1e-12 * np.abs(xp).max())
        xp1 = f.sample_batch(ns, seed=11, kind="precision", mean=m1, common_noise=common)
        np.testing.assert_allclose(xp1 - m1, xp - mB[:, None, :], rtol=1e-12, atol=1e-12 * np.abs(xp).max())


# ---- lifetime ---------------------------------------------------------------------------------------
def test_lifetime():
    c = _case("box11-nb64")
    f, n = c.f, c.n
    X = c.X[:, :5]
    # the single handle's products, blocked solve and selected inverse
    f.factor(c.val).wait()
    Xs = np.asfortranarray(X[0].T)
    single = (f.factor_mult(Xs, 0), f.solve_many(Xs))
    f.selected_inverse()
    zdiag = f.inverse_diag()
    assert c.batch(2) == 0
    y2 = f.factor_mult_batch(X[:2], 0)
    assert c.batch(5) == 0                               # a larger batch is picked up
    y5 = f.factor_mult_batch(X, 0)
    for b in range(5):
        want = (c.member(b) @ X[b].T).T
        np.testing.assert_allclose(y5[b], want, rtol=1e-12, atol=1e-12 * np.abs(want).max())
    np.testing.assert_allclose(y5[:2], y2, rtol=1e-12, atol=1e-12 * np.abs(y2).max())
    f.release_batch()                                    # ... takes the products' storage with it
    with pytest.raises(api.SplltError) as ei:
        f.factor_mult_batch(X)
    assert ei.value.flag == -10 and "no batch" in f.last_error()
    assert c.batch(3) == 0
    y3 = f.factor_mult_batch(X[:3], 0)
    np.testing.assert_allclose(y3, y5[:3], rtol=1e-12, atol=1e-12 * np.abs(y5).max())
    f.sample_batch(3, kind="covariance", mean=np.ones(n))
    f.release_factor_mult_batch()
    f.release_factor_mult_batch()
    assert np.array_equal(f.factor_mult_batch(X[:3], 0), y3)
    # the tables are shared with the single-handle products: releasing either user leaves the other working
    f.release_factor_mult()
    assert np.array_equal(f.factor_mult_batch(X[:3], 0), y3)
    assert np.array_equal(f.factor_mult(Xs, 0), single[0])
    f.release_factor_mult_batch()
    assert np.array_equal(f.factor_mult(Xs, 0), single[0])
    # untouched by everything above
    assert np.array_equal(f.factor_mult(Xs, 0), single[0])
    np.testing.assert_allclose(f.solve_many(Xs), single[1], rtol=1e-12, atol=1e-12)
    assert np.array_equal(f.inverse_diag(), zdiag)


def test_allocation_failure_leaves_the_batch_and_the_solves_usable():
    c = _case("box11-nb64")
    f, n = c.f, c.n
    f.factor(c.val).wait()
    assert c.batch(3) == 0
    X = c.X[:3, :3]
    xb = f.solve_batch(X)
    xs = f.solve(X[0, 0])
    f.release_factor_mult_batch()
    assert f.lib.spllt_hip_debug(b"fmult_alloc_fail=2") == 0      # blocks of 32 and blocks of 16
    try:
        with pytest.raises(api.SplltError) as ei:
            f.factor_mult_batch(X)
    finally:
        assert f.lib.spllt_hip_debug(b"fmult_alloc_fail=0") == 0
    assert ei.value.flag == _lib_allocation() and "memory" in f.last_error()
    np.testing.assert_allclose(f.solve_batch(X), xb, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(f.solve(X[0, 0]), xs, rtol=1e-12, atol=1e-12)
    want = (c.member(1) @ X[1].T).T
    np.testing.assert_allclose(f.factor_mult_batch(X)[1], want, rtol=1e-12, atol=1e-12 * np.abs(want).max())


def _lib_allocation():
    """SPLLT_ERROR_ALLOCATION of include/spllt_iface.h"""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return int(re.search(r"#define\s+SPLLT_ERROR_ALLOCATION\s+\((-?\d+)\)", open(os.path.join(root, "include", "spllt_iface.h")).read()).group(1))


def test_errors():
    c = _case("p2d12-nb8")
    f, n = c.f, c.n
    assert c.batch(2) == 0
    x = np.ones(2 * 3 * n)
    p = x.ctypes.data
    assert f.lib.spllt_hip_factor_mult_batch(f.fkeep, 3, p, n, 3) == -10
    assert f.lib.spllt_hip_factor_mult_batch(f.fkeep, 3, p, n - 1, 0) == -10
    assert f.lib.spllt_hip_sample_batch(f.fkeep, 3, p, n, 2, 0, 0, 0, 1, None, 0) == -10
    assert f.lib.spllt_hip_sample_batch(f.fkeep, 3, p, n, 1, 0, 0, 0, 2, None, 0) == -10 and "stream_step" in f.last_error()
    assert f.lib.spllt_hip_sample_batch(f.fkeep, 3, p, n, 1, 0, 0, 0, 1, p, n - 1) == -10 and "ldmean" in f.last_error()
    assert (x == 1.0).all()
    with pytest.raises(ValueError):
        f.factor_mult_batch(np.zeros((3, n)))            # the batch has two members
    with pytest.raises(ValueError):
        f.sample_batch(2, mean=np.zeros((3, n)))


@pytest.mark.parametrize("state", ["analysed", "engine", "factored", "batch", "batch_inverse"])
def test_ladder_on_the_gpu(state):
    cx = capi_ladder.Ctx(_lib.load(), True)
    rows = ladder.check_state(cx, state, ladder.golden(True))
    assert rows >= 5 * 5 + 1


# ---- torch ------------------------------------------------------------------------------------------
def test_torch_sample_batch():
    import torch
    from spllt_amd.torch_ops import SparseCholesky
    c = _case("box11-nb64")
    n, nbatch, ns = c.n, 3, 6
    chol = SparseCholesky(c.A, nb=64, nemin=16)
    vals = torch.tensor(c.values(nbatch), device="cuda", requires_grad=True)
    mB = torch.tensor(np.random.default_rng(5).standard_normal((nbatch, n)), device="cuda")
    for kind in ("covariance", "precision"):
        for common in (False, True):
            S = chol.sample_batch(vals, ns, seed=9, kind=kind, mean=mB, common_noise=common)
            assert S.shape == (nbatch, n, ns) and S.dtype == torch.float64 and S.device == vals.device
            assert S.requires_grad is False
            # Factorization.sample_batch on the handle that holds these factors
            want = chol.f.sample_batch(ns, seed=9, kind=kind, mean=mB.cpu().numpy(), common_noise=common)
            got = S.cpu().numpy().transpose(0, 2, 1)
            if kind == "covariance":
                assert np.array_equal(got, want)
            else:
                np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12 * np.abs(want).max())
    # a shared mean, common noise
    S = chol.sample_batch(vals, ns, seed=9, kind="covariance", mean=mB[0])
    assert np.array_equal(S.cpu().numpy().transpose(0, 2, 1),
                          chol.f.sample_batch(ns, seed=9, kind="covariance", mean=mB[0].cpu().numpy()))
    Sc = chol.sample_batch(vals, ns, seed=9, kind="covariance", common_noise=True)
    Zc = chol.f.white_noise_batch(ns, seed=9, common_noise=True)
    assert np.array_equal(Zc[0], Zc[1]) and np.array_equal(Zc[1], Zc[2])
    assert np.array_equal(Sc.cpu().numpy().transpose(0, 2, 1), chol.f.sample_batch(ns, seed=9, kind="covariance", common_noise=True))
    with pytest.raises(ValueError):
        chol.sample_batch(vals, ns, mean=mB[:2])
    rep = SparseCholesky(c.A, nb=64, nemin=16, reproducible=True)
    with pytest.raises(NotImplementedError):
        rep.sample_batch(vals, ns)
