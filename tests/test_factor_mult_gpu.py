"""GPU tests of the factor products (spllt_hip_factor_mult*) and the Gaussian samplers (spllt_hip_sample*,
spllt_hip_white_noise_dev; factor_mult.hip).  Accuracy against the dense factor rebuilt from get_factor() through
the sym tables, with the dot-product bound of the case's longest row of L; the inverse relation with solve_many at
the project's backward-error bar; determinism by results only (np.array_equal)."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from factor_mult_emulate import white_noise_reference
from helpers import bwd_err, lower_mask, make_case, sym_tables
from spllt_amd import api, matgen

pytestmark = pytest.mark.gpu

CASES = [
    ("p2d12-nb8", lambda: matgen.poisson2d(12), 8, 4),
    ("p2d40-nb16", lambda: matgen.poisson2d(40), 16, 16),
    ("box11-nb64", lambda: matgen.nd_like((11, 10, 9), 2), 64, 16),
    ("p3d14-nb384", lambda: matgen.poisson3d(14), 384, 16),
    ("box12-nb512", lambda: matgen.nd_like((10, 12, 12), 3), 512, 16),
]
NAMES = [c[0] for c in CASES]
NV = 33


def dense_factor(f, arena):
    """L of P A P^T (n x n, pivot order) and its stored pattern, from the arena through the sym tables"""
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


@functools.lru_cache(maxsize=None)
def _case(name):
    _, gen, nb, nemin = next(c for c in CASES if c[0] == name)
    A = gen()
    f, val = make_case(A, nb=nb, nemin=nemin)
    f.factor(val).wait()
    L, pat = dense_factor(f, f.get_factor())
    X = np.random.default_rng(0).standard_normal((A.shape[0], NV))
    X.setflags(write=False)
    return A, f, val, L, pat, X


def reference(f, L, X, job):
    """(want, size): the product in user order and sum |.| |.| of what was added up for every entry"""
    order = f.sym("order")
    Xp = np.empty_like(X)
    Xp[order] = X
    if job == 1:
        y, s = L @ Xp, np.abs(L) @ np.abs(Xp)
    elif job == 2:
        y, s = L.T @ Xp, np.abs(L.T) @ np.abs(Xp)
    else:
        y, s = L @ (L.T @ Xp), np.abs(L) @ (np.abs(L.T) @ np.abs(Xp))
    return y[order], s[order]


@pytest.mark.parametrize("nvec", [1, 3, 16, 17, 33])
@pytest.mark.parametrize("job", [0, 1, 2])
@pytest.mark.parametrize("name", NAMES)
def test_accuracy(name, job, nvec):
    A, f, val, L, pat, X33 = _case(name)
    X = X33[:, :nvec]
    got = f.factor_mult(X if nvec > 1 else X[:, 0], job).reshape(f.n, nvec)
    assert np.isfinite(got).all()
    want, size = reference(f, L, X, job)
    # the dot-product bound with the longest row of L (stored entries); job 0 is two such products in a row
    n_terms = int(pat.sum(axis=1).max())
    bound = 64 * n_terms * 2.0 ** -53 * float(size.max())
    err = float(np.abs(got - want).max())
    print(name, job, nvec, "n_terms", n_terms, "max|got - want|", err, "bound", bound)
    assert err <= bound


@pytest.mark.parametrize("name", NAMES)
def test_inverse_relation(name):
    A, f, val, L, pat, X33 = _case(name)
    X = X33[:, :5]
    order = f.sym("order")
    P = sp.csc_matrix((np.ones(f.n), (order, np.arange(f.n))), shape=(f.n, f.n))   # pivot <- user
    ops = {0: sp.csc_matrix(A), 1: P.T @ sp.csc_matrix(L) @ P, 2: P.T @ sp.csc_matrix(L.T) @ P}
    for job in (0, 1, 2):
        Y = f.factor_mult(X, job)
        back = f.solve_many(Y, job)
        # scaled backward error of the system op(job) x = Y that solve_many(job) solves
        errs = [bwd_err(ops[job], back[:, q], Y[:, q]) for q in range(5)]
        print(name, job, "max scaled backward error", max(errs))
        assert max(errs) <= 1e-14
        np.testing.assert_allclose(back, X, rtol=1e-9, atol=1e-9)
        # ... and the other way round
        np.testing.assert_allclose(f.factor_mult(f.solve_many(X, job), job), X, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(f.factor_mult(X, 0), A @ X, rtol=1e-12, atol=1e-12 * np.abs(A @ X).max())


@pytest.mark.parametrize("name", NAMES)
def test_bit_identity_and_group_independence(name):
    A, f, val, L, pat, X = _case(name)
    for job in (0, 1, 2):
        y = f.factor_mult(X, job)
        for _ in range(2):
            assert np.array_equal(f.factor_mult(X, job), y)
        for q in (0, 1, 15, 16, 17, 31, 32):
            assert np.array_equal(f.factor_mult(X[:, q], job), y[:, q]), (job, q)
        perm = np.random.default_rng(1).permutation(NV)
        assert np.array_equal(f.factor_mult(X[:, perm], job), y[:, perm])
    # blocks of 16 only (what is left when the workspace of 32 does not fit): the same bits per vector
    y = f.factor_mult(X, 0)
    f.release_factor_mult()
    assert f.lib.spllt_hip_debug(b"fmult_alloc_fail=1") == 0
    try:
        y16 = f.factor_mult(X, 0)
    finally:
        assert f.lib.spllt_hip_debug(b"fmult_alloc_fail=0") == 0
    assert np.array_equal(y16, y)
    f.release_factor_mult()
    assert np.array_equal(f.factor_mult(X, 0), y)


def test_allocation_failure_leaves_the_factor_and_the_solves_usable():
    A, f, val, L, pat, X = _case("box11-nb64")
    x = f.solve_many(X[:, :3])
    f.release_factor_mult()
    assert f.lib.spllt_hip_debug(b"fmult_alloc_fail=4") == 0      # blocks of 32 and blocks of 16
    try:
        with pytest.raises(api.SplltError) as ei:
            f.factor_mult(X[:, :3])
    finally:
        assert f.lib.spllt_hip_debug(b"fmult_alloc_fail=0") == 0
    assert ei.value.flag == -1 and "memory" in f.last_error()
    np.testing.assert_allclose(f.solve_many(X[:, :3]), x, rtol=1e-12, atol=1e-12)
    assert np.array_equal(f.solve_reproducible(X[:, :3]), f.solve_reproducible(X[:, :3]))
    np.testing.assert_allclose(f.factor_mult(X[:, :3]), A @ X[:, :3], rtol=1e-12, atol=1e-12 * np.abs(A @ X).max())


@pytest.mark.parametrize("name", ["box11-nb64", "box12-nb512"])
def test_entry_points(name):
    import torch
    A, f, val, L, pat, X33 = _case(name)
    nvec = 5
    X = X33[:, :nvec]
    n, ldx, sentinel = f.n, f.n + 7, -7.25e77
    order = f.sym("order")
    for job in (0, 1, 2):
        want = f.factor_mult(X, job)
        xh = np.full((nvec + 2) * ldx, sentinel)
        for q in range(nvec):
            xh[q * ldx:q * ldx + n] = X[:, q]
        before = xh.copy().reshape(nvec + 2, ldx)
        assert f.lib.spllt_hip_factor_mult(f.fkeep, nvec, api._dp(xh), ldx, job) == 0, f.last_error()
        img = xh.reshape(nvec + 2, ldx)
        assert np.array_equal(img[:nvec, n:], before[:nvec, n:]) and np.array_equal(img[nvec:], before[nvec:])
        assert np.array_equal(img[:nvec, :n].T, want)
        # device, user order, padded
        xd = torch.tensor(before.ravel(), device="cuda")
        torch.cuda.synchronize()
        f.factor_mult_dev(xd.data_ptr(), nvec, ldx=ldx, job=job)
        dimg = xd.cpu().numpy().reshape(nvec + 2, ldx)
        assert np.array_equal(dimg[:nvec, n:], before[:nvec, n:]) and np.array_equal(dimg[nvec:], before[nvec:])
        assert np.array_equal(dimg[:nvec, :n].T, want)
        # device, pivot order, padded
        Xp = np.full((nvec + 2, ldx), sentinel)
        Xp[:nvec, order] = X.T
        yd = torch.tensor(Xp.ravel(), device="cuda")
        torch.cuda.synchronize()
        f.factor_mult_dev(yd.data_ptr(), nvec, ldx=ldx, job=job, pivot_order=True)
        pimg = yd.cpu().numpy().reshape(nvec + 2, ldx)
        assert np.array_equal(pimg[:nvec, n:], Xp[:nvec, n:]) and np.array_equal(pimg[nvec:], Xp[nvec:])
        assert np.array_equal(pimg[:nvec, order].T, want)
    # nvec = 0
    x = np.full(n, 3.0)
    assert f.lib.spllt_hip_factor_mult(f.fkeep, 0, api._dp(x), n, 0) == 0 and (x == 3.0).all()
    assert f.factor_mult(np.zeros((n, 0))).shape == (n, 0)


def test_two_handles():
    A = matgen.nd_like((11, 10, 9), 2)
    X = np.random.default_rng(2).standard_normal((A.shape[0], 5))
    ys, Ls = [], []
    for _ in range(2):
        f, val = make_case(A, nb=64, nemin=16, engine_flags=4096)
        f.factor(val).wait()
        Ls.append(f.get_factor())
        ys.append([f.factor_mult(X, job) for job in (0, 1, 2)] + [f.sample(3, seed=5, kind="covariance")])
        f.close()
    assert np.array_equal(Ls[0], Ls[1])
    for a, b in zip(ys[0], ys[1]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("name", NAMES)
def test_poison(name):
    import torch
    A, f, val, L, pat, X33 = _case(name)
    X = X33[:, :17]
    want = [f.factor_mult(X, job) for job in (0, 1, 2)]
    # the strict upper triangles of the diagonal tiles in the device arena
    arena = f.sym_info()["arena"]
    ptr = f.device_factor_ptr()
    upper = torch.as_tensor(np.nonzero(~lower_mask(f))[0], device="cuda")
    assert upper.numel() > 0

    class _Arena:      # a torch view of the device arena (no copy, not owned)
        __cuda_array_interface__ = {"shape": (arena,), "typestr": "<f8", "data": (int(ptr), False), "version": 2}
    Ld = torch.as_tensor(_Arena(), device="cuda")
    saved = Ld[upper].clone()
    Ld[upper] = float("nan")
    torch.cuda.synchronize()
    try:
        for key in (b"rsolve_poison", b"fmult_poison"):
            assert f.lib.spllt_hip_debug(key + b"=1") == 0
        got = [f.factor_mult(X, job) for job in (0, 1, 2)]
    finally:
        for key in (b"rsolve_poison", b"fmult_poison"):
            assert f.lib.spllt_hip_debug(key + b"=0") == 0
        Ld[upper] = saved
        torch.cuda.synchronize()
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


def test_after_update_and_refactorization():
    A = matgen.nd_like((11, 10, 9), 2)
    f, val = make_case(A, nb=64, nemin=16)
    n = f.n
    X = np.random.default_rng(3).standard_normal((n, 4))
    with pytest.raises(api.SplltError) as ei:          # before the first factorization
        f.factor_mult(X)
    assert ei.value.flag == -10 and "factorized" in f.last_error()
    with pytest.raises(api.SplltError) as ei:
        f.sample(2)
    assert ei.value.flag == -10
    f.factor(val).wait()
    y1 = f.factor_mult(X)
    f.factor(4.0 * val).wait()                         # a later factorization is picked up
    np.testing.assert_allclose(f.factor_mult(X), 4.0 * y1, rtol=1e-12, atol=1e-12 * np.abs(y1).max())
    f.factor(val).wait()
    # one clique column: an existing off-diagonal entry of A, so that the pattern of L holds the update
    Al = sp.tril(sp.csc_matrix(A), -1).tocoo()
    i, j = int(Al.row[0]), int(Al.col[0])
    W = sp.csc_matrix(([0.5, -0.25], ([i, j], [0, 0])), shape=(n, 1))
    A1 = (A + W @ W.T).tocsc()
    f.update(W)
    want = A1 @ X
    np.testing.assert_allclose(f.factor_mult(X, 0), want, rtol=1e-12, atol=1e-12 * np.abs(want).max())
    # release and use again
    y = f.factor_mult(X, 0)
    f.release_factor_mult()
    assert np.array_equal(f.factor_mult(X, 0), y)
    # the tables are shared with the reproducible solve: releasing one user leaves the other working
    xr = f.solve_reproducible(X)
    f.release_factor_mult()
    assert np.array_equal(f.solve_reproducible(X), xr)
    assert np.array_equal(f.factor_mult(X, 0), y)
    f.release_solve_repro()
    assert np.array_equal(f.factor_mult(X, 0), y)
    assert np.array_equal(f.solve_reproducible(X), xr)
    f.close()


def test_errors():
    A, f, val, L, pat, X = _case("p2d12-nb8")
    n = f.n
    x = np.ones(3 * n)
    assert f.lib.spllt_hip_factor_mult(f.fkeep, 3, api._dp(x), n, 3) == -10
    assert f.lib.spllt_hip_factor_mult(f.fkeep, 3, api._dp(x), n - 1, 0) == -10
    assert f.lib.spllt_hip_sample(f.fkeep, 3, api._dp(x), n, 2, 0, 0, None) == -10
    assert f.lib.spllt_hip_sample(f.fkeep, 3, api._dp(x), n - 1, 0, 0, 0, None) == -10
    assert (x == 1.0).all()


def test_partitioned_factor_returns_unimplemented():
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
    xd = torch.ones(2 * fs[0].n, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    for f in fs:
        f.wait()
        with pytest.raises(api.SplltError) as ei:
            f.factor_mult(np.ones((f.n, 2)))
        assert ei.value.flag == -98 and "partitioned" in f.last_error()
        with pytest.raises(api.SplltError) as ei:
            f.factor_mult_dev(xd.data_ptr(), 2)
        assert ei.value.flag == -98
        for kind in ("precision", "covariance"):
            with pytest.raises(api.SplltError) as ei:
                f.sample(2, kind=kind)
            assert ei.value.flag == -98
        with pytest.raises(api.SplltError) as ei:
            f.white_noise(2, seed=1)
        assert ei.value.flag == -98
    for f in fs:
        f.close()


# ---- noise and sampling ---------------------------------------------------------------------------
def _ulps(a, b):
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


def test_white_noise():
    A, f, val, L, pat, X = _case("p2d40-nb16")
    n = f.n
    Z = f.white_noise(5, seed=7)
    assert Z.shape == (n, 5)
    ref = white_noise_reference(n, 5, seed=7)
    worst = float(_ulps(Z, ref).max())
    print("white noise against numpy Philox4x32-10 + Box-Muller: worst", worst, "ulp")
    assert worst <= 4
    assert np.array_equal(Z[:, 2:5], f.white_noise(3, seed=7, first_sample=2))
    assert np.array_equal(Z, f.white_noise(5, seed=7))
    assert not np.array_equal(Z, f.white_noise(5, seed=8))
    big = (1 << 40) + 12345                      # the high words of seed and sample index take part
    Zb = f.white_noise(2, seed=big, first_sample=(1 << 33) + 1)
    assert float(_ulps(Zb, white_noise_reference(n, 2, seed=big, first_sample=(1 << 33) + 1)).max()) <= 4
    assert not np.array_equal(Zb, f.white_noise(2, seed=12345, first_sample=1))


@pytest.mark.parametrize("name", ["p2d12-nb8", "box11-nb64", "p3d14-nb384"])
def test_sampling_identities(name):
    import torch
    A, f, val, L, pat, X = _case(name)
    n, ns = f.n, 35
    order = f.sym("order")
    Zu = f.white_noise(ns, seed=11)[order]           # the pivot-order noise laid out in user positions
    m = np.random.default_rng(4).standard_normal(n)
    xc = f.sample(ns, seed=11, kind="covariance", mean=m)
    assert np.array_equal(xc, m[:, None] + f.factor_mult(Zu, job=1))
    assert np.array_equal(f.sample(ns, seed=11, kind="covariance"), f.factor_mult(Zu, job=1))
    assert np.array_equal(f.sample(3, seed=11, kind="covariance", mean=m, first_sample=20), xc[:, 20:23])
    # the device entry point, padded
    ldx = n + 3
    xd = torch.full((ns + 1, ldx), -7.25e77, dtype=torch.float64, device="cuda")
    md = torch.tensor(m, device="cuda")
    torch.cuda.synchronize()
    f.sample_dev(xd.data_ptr(), ns, ldx=ldx, seed=11, kind="covariance", mean_dev_ptr=md.data_ptr())
    img = xd.cpu().numpy()
    assert np.array_equal(img[:ns, :n].T, xc) and (img[:ns, n:] == -7.25e77).all() and (img[ns] == -7.25e77).all()
    # precision: the backward sweep, reproducible when the switch is on
    plain = f.sample(ns, seed=11, kind="precision", mean=m)
    np.testing.assert_allclose(plain - m[:, None], f.solve_reproducible(Zu, job=2), rtol=1e-12,
                               atol=1e-12 * np.abs(plain).max())
    assert f.set_reproducible_solve(True) is False
    try:
        xp = f.sample(ns, seed=11, kind="precision")
        assert np.array_equal(xp, f.solve_reproducible(Zu, job=2))
        assert np.array_equal(f.sample(ns, seed=11, kind="precision", mean=m), m[:, None] + xp)
        xd.fill_(0.0)
        torch.cuda.synchronize()
        f.sample_dev(xd.data_ptr(), ns, ldx=ldx, seed=11, kind=0)
        assert np.array_equal(xd.cpu().numpy()[:ns, :n].T, xp)
    finally:
        assert f.set_reproducible_solve(False) is True


@pytest.mark.parametrize("kind", ["precision", "covariance"])
def test_statistics(kind):
    A, f, val, L, pat, X = _case("p2d12-nb8")
    ns = 4096
    S = f.sample(ns, seed=0, kind=kind)
    Sh = S @ S.T / ns
    Sigma = np.linalg.inv(A.toarray()) if kind == "precision" else A.toarray()
    d = np.diag(Sigma)
    t = np.abs(Sh - Sigma) / np.sqrt((np.outer(d, d) + Sigma ** 2) / ns)
    print(kind, "max standardized deviation of the sample covariance", float(t.max()))
    assert t.max() <= 6
