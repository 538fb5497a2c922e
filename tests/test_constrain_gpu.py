"""GPU tests of the hard linear constraints (include/spllt_hip_constrain.h, spllt_amd/csrc/constrain.hip) against
the dense emulation of constrain_emulate.py and the KKT solve.  The matrices are the smallest at which the tiling can
still go wrong: poisson2d(8) (n = 64: one chunk, full tiles), poisson2d(12) (n = 144: three chunks, a tail of 16) and
poisson3d(5) (n = 125: no multiple of 4, 16 or the chunk of 64); k in {1, 3, 16, 17, 33} and 64 on the two larger
ones (every count of 16-row tiles, with and without a tail, and k not a multiple of 4); nvec in {1, 5, 32, 33, 40}
(a block of 16, one of 32, 32 + a tail).  ldx = n + 3, ldc = n + 5, lde = k + 1, ldl = k + 2, all padding NaN."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import capi_ladder
import constrain_emulate as emu
import constrain_ladder as ladder
from spllt_amd import _lib, api

pytestmark = pytest.mark.gpu

MATS = ("p2d8", "p2d12", "p3d5")
CASES = [(m, k) for m in MATS for k in (1, 3, 16, 17, 33, 64) if not (m == "p2d8" and k == 64)]
NVECS = (1, 5, 32, 33, 40)
NAN = float("nan")


class Case:
    def __init__(self, name):
        A, nb, nemin = emu.case_matrix(name)
        self.A = A.toarray()
        self.n, self.ptr, self.row, self.val = api.csc_lower_1based(A)
        self.nb, self.nemin = nb, nemin
        self.f = self.new_factor()
        self.ainv_max = float(np.abs(np.linalg.inv(self.A)).max())

    def new_factor(self, scale=1.0):
        f = api.Factorization(self.n, self.ptr, self.row, nb=self.nb, nemin=self.nemin)
        f.factor(scale * self.val).wait()
        return f


@functools.lru_cache(maxsize=None)
def _case(name):
    return Case(name)


@functools.lru_cache(maxsize=None)
def _con(name, k):
    c = _case(name)
    return emu.Constraints(c.A, emu.constraint_rows(k, c.n))


def _padded(M, ld):
    """the columns of M (len x nvec) as vectors at q * ld, padding NaN"""
    M = np.asarray(M, dtype=np.float64).reshape(M.shape[0], -1)
    out = np.full((M.shape[1], ld), NAN)
    out[:, :M.shape[0]] = M.T
    return out


def _dp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def _set(f, Crows, dev=False):
    """spllt_hip_set_constraints(_dev) with ldc = n + 5 and NaN in the padding"""
    k, n = Crows.shape
    cp = np.full((k, n + 5), NAN)
    cp[:, :n] = Crows
    if dev:
        import torch
        ct = torch.tensor(cp, device="cuda")
        return f.lib.spllt_hip_set_constraints_dev(f.fkeep, k, C.c_void_p(ct.data_ptr()), n + 5)
    return f.lib.spllt_hip_set_constraints(f.fkeep, k, _dp(cp), n + 5)


def _run(f, entry, X, e, k, dev):
    """entry (constrain / solve_constrained) on padded arrays; e: None, (k,) or (k, nvec).  Returns (x, lambda)
    after checking that no padding was touched and no result is NaN."""
    n, nvec = X.shape
    xp = _padded(X, n + 3)
    lp = np.full((nvec, k + 2), NAN)
    ep, lde = None, 0
    if e is not None and e.ndim == 1:
        ep = e.copy()
    elif e is not None:
        ep, lde = _padded(e, k + 1), k + 1
    if dev:
        import torch
        xt, lt = torch.tensor(xp, device="cuda"), torch.tensor(lp, device="cuda")
        et = None if ep is None else torch.tensor(ep, device="cuda")
        rc = getattr(f.lib, f"spllt_hip_{entry}_dev")(f.fkeep, nvec, C.c_void_p(xt.data_ptr()), n + 3,
                                                       None if et is None else C.c_void_p(et.data_ptr()), lde,
                                                       C.c_void_p(lt.data_ptr()), k + 2)
        xp, lp = xt.cpu().numpy(), lt.cpu().numpy()
    else:
        rc = getattr(f.lib, f"spllt_hip_{entry}")(f.fkeep, nvec, _dp(xp), n + 3, _dp(ep), lde, _dp(lp), k + 2)
    assert rc == 0, (entry, rc, f.last_error())
    assert np.isnan(xp[:, n:]).all() and np.isnan(lp[:, k:]).all()
    x, lam = xp[:, :n].T, lp[:, :k].T
    assert not np.isnan(x).any() and not np.isnan(lam).any()
    return x, lam


def _targets(rng, k, nvec):
    return (None, rng.standard_normal(k), rng.standard_normal((k, nvec)))


# ---- 1. constrain and solve_constrained against the emulation and the KKT solve --------------------------------
@pytest.mark.parametrize("name,k", CASES)
def test_constrain_and_solve_constrained(name, k):
    c, con = _case(name), _con(name, k)
    f, n = c.f, c.n
    assert _set(f, con.C) == 0, f.last_error()
    rng = np.random.default_rng(17 * k + n)
    for nvec in NVECS:
        X = rng.standard_normal((n, nvec))
        for e in _targets(rng, k, nvec):
            E = con.targets(e, nvec)
            want_x, want_l = con.correct(X, e)
            kkt_x, kkt_l = con.kkt_solve(X, e)         # (X as right-hand sides)
            got = {}
            for dev in (False, True):
                x, lam = _run(f, "constrain", X, e, k, dev)
                np.testing.assert_allclose(x, want_x, rtol=1e-12, atol=1e-12)
                np.testing.assert_allclose(lam, want_l, rtol=1e-12, atol=1e-12)
                assert np.abs(con.C @ x - E).max() <= emu.residual_bar(con.C, x, e)
                xs, ls = _run(f, "solve_constrained", X, e, k, dev)
                np.testing.assert_allclose(xs, kkt_x, rtol=1e-12, atol=1e-12)
                np.testing.assert_allclose(ls, kkt_l, rtol=1e-12, atol=1e-12)
                assert np.abs(con.C @ xs - E).max() <= emu.residual_bar(con.C, xs, e)
                got[dev] = (x, lam, xs, ls)
            # host and device entry points: the correction is the same arithmetic, the solve in front of it adds
            # with atomics and agrees to rounding
            assert np.array_equal(got[False][0], got[True][0]) and np.array_equal(got[False][1], got[True][1])
            np.testing.assert_allclose(got[False][2], got[True][2], rtol=1e-12, atol=1e-12)
            np.testing.assert_allclose(got[False][3], got[True][3], rtol=1e-12, atol=1e-12)
    # the Python wrappers: the same numbers, F-ordered (n, nvec) in and out, a vector for a vector
    X = rng.standard_normal((n, 5))
    e = rng.standard_normal(k)
    x, lam = f.constrain(X, e=e, multipliers=True)
    assert x.shape == (n, 5) and lam.shape == (k, 5) and x.flags["F_CONTIGUOUS"]
    assert np.array_equal(x, _run(f, "constrain", X, e, k, False)[0])
    x1 = f.solve_constrained(X[:, 0])
    assert x1.shape == (n,)
    np.testing.assert_allclose(x1, con.kkt_solve(X[:, 0])[0], rtol=1e-12, atol=1e-12)
    # the device entry point of set_constraints stores the same rows
    # (a second build: W comes from the blocked solve, whose strips add with atomics -- equal to rounding)
    ld0 = f.constraints_info()["log_det_s"]
    assert _set(f, con.C, dev=True) == 0
    np.testing.assert_allclose(f.constrain(X, e=e), x, rtol=1e-12, atol=1e-12)
    assert f.constraints_info()["log_det_s"] == pytest.approx(ld0, rel=1e-12, abs=1e-12)


# ---- 2. fixed arithmetic -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", [(m, k) for m in MATS for k in (3, 33)])
def test_fixed_arithmetic(name, k):
    c, con = _case(name), _con(name, k)
    f, n = c.f, c.n
    assert _set(f, con.C) == 0
    rng = np.random.default_rng(k)
    X = rng.standard_normal((n, 40))
    e = rng.standard_normal((k, 40))
    a, la = _run(f, "constrain", X, e, k, False)
    b, lb = _run(f, "constrain", X, e, k, False)
    assert np.array_equal(a, b) and np.array_equal(la, lb)
    # vector 37 of 40 (the tail block of 16, place 5) and the same vector alone (a block of 16, place 0), on both entries
    for dev in (False, True):
        one, l1 = _run(f, "constrain", X[:, 37:38], e[:, 37:38], k, dev)
        assert np.array_equal(one[:, 0], a[:, 37]) and np.array_equal(l1[:, 0], la[:, 37])
    # ... and in the first block of 32
    one, _ = _run(f, "constrain", X[:, 20:21], e[:, 20:21], k, False)
    assert np.array_equal(one[:, 0], a[:, 20])
    # with the reproducible solve W has the same bits in two separate builds, and so have U, G and log det S
    before = f.set_reproducible_solve(True)
    try:
        assert _set(f, con.C) == 0
        r1, i1 = _run(f, "constrain", X, e, k, False), f.constraints_info()
        assert f.release_constraints() is f and _set(f, con.C) == 0
        r2, i2 = _run(f, "constrain", X, e, k, False), f.constraints_info()
        assert np.array_equal(r1[0], r2[0]) and np.array_equal(r1[1], r2[1])
        assert i1["log_det_s"] == i2["log_det_s"] and i1["min_relative_pivot"] == i2["min_relative_pivot"]
    finally:
        f.set_reproducible_solve(before)


# ---- 3. sample_constrained --------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", [(m, k) for m in MATS for k in (1, 17)])
def test_sample_constrained(name, k):
    c, con = _case(name), _con(name, k)
    f, n = c.f, c.n
    assert _set(f, con.C) == 0
    rng = np.random.default_rng(k + 1)
    mu, e = rng.standard_normal(n), rng.standard_normal(k)
    order = f.sym("order")
    Zu = f.white_noise(40, seed=5)[order]               # the pivot-order noise laid out in user positions
    base = mu[:, None] + f.solve_many(Zu, job=2)
    for mean, tgt in ((mu, e), (None, None)):
        X = f.sample_constrained(40, seed=5, mean=mean, e=tgt)
        want = con.correct(base if mean is not None else base - mu[:, None], tgt)[0]
        np.testing.assert_allclose(X, want, rtol=1e-12, atol=1e-12)
        assert np.abs(con.C @ X - con.targets(tgt, 40)).max() <= emu.residual_bar(con.C, X, tgt)
        # sample q is a function of (seed, first_sample + q) alone
        part = f.sample_constrained(3, seed=5, mean=mean, e=tgt, first_sample=35)
        np.testing.assert_allclose(part, X[:, 35:38], rtol=1e-12, atol=1e-12)
    # the device entry point, and with the reproducible solve the same bits whatever nsamp
    import torch
    xt = torch.full((40, n + 3), NAN, dtype=torch.float64, device="cuda")
    mt, et = torch.tensor(mu, device="cuda"), torch.tensor(e, device="cuda")
    f.sample_constrained_dev(xt.data_ptr(), 40, ldx=n + 3, seed=5, mean_dev_ptr=mt.data_ptr(), e_dev_ptr=et.data_ptr())
    xd = xt.cpu().numpy()
    assert np.isnan(xd[:, n:]).all()
    np.testing.assert_allclose(xd[:, :n].T, con.correct(base, e)[0], rtol=1e-12, atol=1e-12)
    before = f.set_reproducible_solve(True)
    try:
        X = f.sample_constrained(40, seed=9, mean=mu, e=e)
        assert np.array_equal(f.sample_constrained(3, seed=9, mean=mu, e=e, first_sample=35), X[:, 35:38])
        assert np.array_equal(f.constrain(f.sample(40, seed=9, mean=mu), e=e), X)
    finally:
        f.set_reproducible_solve(before)


# ---- 4. inverse_diag_constrained ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", MATS)
def test_inverse_diag_constrained(name):
    c = _case(name)
    f = c.new_factor()

    def refused_like_the_sibling():
        with pytest.raises(api.SplltError) as e0:
            f.inverse_diag()
        with pytest.raises(api.SplltError) as e1:
            f.inverse_diag_constrained()
        assert e1.value.flag == e0.value.flag == -10
        assert "spllt_hip_inverse_diag_constrained: no selected inverse" in f.last_error()

    try:
        assert _set(f, _con(name, 17).C) == 0
        refused_like_the_sibling()                  # no selected inverse yet
        f.selected_inverse()
        plain = f.inverse_diag()
        for k in (17, 1, 33 if name == "p2d8" else 64):
            con = _con(name, k)
            assert _set(f, con.C) == 0
            v = f.inverse_diag_constrained()
            assert np.abs(v - np.diag(con.conditional_cov())).max() <= 1e-11 * c.ainv_max
            assert (v > 0).all() and (v < plain).all()
        f.factor(c.val).wait()
        refused_like_the_sibling()                  # a stale one
    finally:
        f.close()


# ---- 5. constraints_info ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", CASES)
def test_constraints_info(name, k):
    c, con = _case(name), _con(name, k)
    f = c.f
    assert _set(f, con.C) == 0
    info = f.constraints_info()
    want = con.log_det_s()
    assert abs(info["log_det_s"] - want) <= 1e-12 * abs(want)
    assert info["k"] == k and info["launches"] > 0 and info["device_bytes"] >= 2 * 8 * k * c.n
    # (pivots of O(0.1 .. 1) from sums of n products: the dense-inverse bar is ample)
    assert abs(info["min_relative_pivot"] - con.min_relative_pivot()) <= 1e-11
    f.constrain(np.ones(c.n))
    assert f.constraints_info()["launches"] == 3


# ---- 6. dependent rows ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MATS)
def test_dependent_rows(name):
    c = _case(name)
    f, n = c.f, c.n
    base = emu.constraint_rows(5, n)
    zero = base.copy()
    zero[2] = 0.0
    dup = base.copy()
    dup[4] = dup[1]
    for rows, bad in ((zero, 3), (dup, 5)):
        assert _set(f, base) == 0 and f.constraints_info()["k"] == 5
        assert _set(f, rows) == -20
        assert f"row {bad} of C" in f.last_error(), f.last_error()
        assert f.constraints_info()["k"] == 0
        with pytest.raises(api.SplltError) as ei:
            f.constrain(np.ones(n))
        assert ei.value.flag == -10 and "no constraints" in f.last_error()
        b = c.A @ np.ones(n)
        np.testing.assert_allclose(f.solve_many(b), np.ones(n), rtol=1e-12, atol=1e-12)
    # a NaN in C is a pivot that is not finite
    nanrow = base.copy()
    nanrow[1, 3] = NAN
    assert _set(f, nanrow) == -20 and "of C" in f.last_error()


# ---- 7. a later factor is picked up ----------------------------------------------------------------------
@pytest.mark.parametrize("name", MATS)
def test_pickup_of_a_later_factor(name):
    c = _case(name)
    f, n = c.new_factor(), c.n
    try:
        Crows = emu.constraint_rows(17, n)
        assert _set(f, Crows) == 0
        rng = np.random.default_rng(3)
        X, e = rng.standard_normal((n, 33)), rng.standard_normal(17)
        r0 = f.constraints_info()["rebuilds"]
        np.testing.assert_allclose(f.constrain(X, e=e), emu.Constraints(c.A, Crows).correct(X, e)[0], rtol=1e-12, atol=1e-12)
        assert f.constraints_info()["rebuilds"] == r0
        f.factor(2.0 * c.val).wait()
        con2 = emu.Constraints(2.0 * c.A, Crows)
        x, lam = f.constrain(X, e=e, multipliers=True)
        np.testing.assert_allclose(x, con2.correct(X, e)[0], rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(lam, con2.correct(X, e)[1], rtol=1e-12, atol=1e-12)
        assert f.constraints_info()["rebuilds"] == r0 + 1
        w = sp.csc_matrix(([0.5, -0.5], ([0, 1], [0, 0])), shape=(n, 1))     # one clique column
        f.update(w)
        A3 = 2.0 * c.A + (w @ w.T).toarray()
        con3 = emu.Constraints(A3, Crows)
        xs, ls = f.solve_constrained(X, e=e, multipliers=True)
        kx, kl = con3.kkt_solve(X, e)
        np.testing.assert_allclose(xs, kx, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(ls, kl, rtol=1e-12, atol=1e-12)
        assert f.constraints_info()["rebuilds"] == r0 + 2
        np.testing.assert_allclose(f.constrain(X, e=e), con3.correct(X, e)[0], rtol=1e-12, atol=1e-12)
        assert f.constraints_info()["rebuilds"] == r0 + 2
        assert abs(f.constraints_info()["log_det_s"] - con3.log_det_s()) <= 1e-12 * abs(con3.log_det_s())
    finally:
        f.close()


# ---- 8. the GPU rows of the ladder ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ctx():
    return capi_ladder.Ctx(_lib.load(), True)


@pytest.mark.parametrize("state", ladder.GPU_STATES)
def test_ladder_with_a_device(state):
    assert ladder.check_state(_ctx(), state, ladder.golden(True)) == ladder.ROWS


def test_ladder_rows_of_this_family_alone():
    c = _ctx()
    h = c.handle("factored")
    lib, fk, n = c.lib, h[1], c.n
    out, stat = np.zeros(4, dtype=np.int64), np.zeros(2)

    def err():
        return (lib.spllt_hip_last_error(fk) or b"").decode()

    def info():
        """the k that is set; out and stat refreshed"""
        assert lib.spllt_hip_constraints_info(fk, out.ctypes.data_as(C.POINTER(C.c_int64)), _dp(stat)) == 0
        return int(out[0])

    try:
        rows = emu.constraint_rows(3, n)
        x, e3, lam = np.ones(2 * n), np.zeros(8), np.zeros(8)
        # nothing set yet
        assert lib.spllt_hip_constrain(fk, 2, _dp(x), n, None, 0, None, 0) == -10 and "no constraints" in err()
        assert lib.spllt_hip_set_constraints(fk, 65, _dp(rows), n) == -10 and "k > 64" in err()
        assert lib.spllt_hip_set_constraints(fk, 3, _dp(rows), n) == 0 and info() == 3
        # the strides of e and lambda are checked against the k that is set
        assert lib.spllt_hip_constrain(fk, 2, _dp(x), n, _dp(e3), 2, None, 0) == -10 and "lde" in err()
        assert lib.spllt_hip_constrain(fk, 2, _dp(x), n, _dp(e3), 0, _dp(lam), 2) == -10 and "ldl < k" in err()
        assert lib.spllt_hip_constrain(fk, 2, _dp(x), n, _dp(e3), 3, _dp(lam), 3) == 0
        assert lib.spllt_hip_constrain(fk, 0, _dp(x), n, None, 0, None, 0) == 0          # nvec = 0: a no-op
        # k = 0 clears
        assert lib.spllt_hip_set_constraints(fk, 0, None, n) == 0 and info() == 0
        assert lib.spllt_hip_solve_constrained(fk, 2, _dp(x), n, None, 0, None, 0) == -10 and "no constraints" in err()
        # release, then use, then release again
        assert lib.spllt_hip_set_constraints(fk, 3, _dp(rows), n) == 0 and info() == 3 and out[2] > 0
        assert lib.spllt_hip_release_constraints(fk) == 0 and info() == 0 and out[2] == 0
        assert lib.spllt_hip_sample_constrained(fk, 2, _dp(x), n, 1, 0, None, None) == -10 and "no constraints" in err()
        assert lib.spllt_hip_release_constraints(fk) == 0
        assert lib.spllt_hip_solve_many(fk, 2, _dp(x), n, 0) == 0
    finally:
        c.free(h)


# ---- the torch front end -------------------------------------------------------------------------------------
def test_torch_front_end_without_gradients():
    import torch
    from spllt_amd.torch_ops import SparseCholesky
    c, con = _case("p3d5"), _con("p3d5", 3)
    n = c.n
    ch = SparseCholesky((c.n, c.ptr, c.row), nb=c.nb, nemin=c.nemin)
    try:
        val = torch.tensor(c.val, device="cuda", requires_grad=True)
        B = torch.tensor(np.random.default_rng(0).standard_normal((n, 5)), device="cuda")
        e = torch.tensor(np.arange(3.0), device="cuda")
        with pytest.raises(RuntimeError):
            ch.solve_constrained(val, B)
        ch.set_constraints(torch.tensor(con.C, device="cuda"))
        x, lam = ch.solve_constrained(val, B, e)
        kx, kl = con.kkt_solve(B.cpu().numpy(), e.cpu().numpy())
        np.testing.assert_allclose(x.cpu().numpy(), kx, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(lam.cpu().numpy(), kl, rtol=1e-12, atol=1e-12)
        assert not x.requires_grad and not lam.requires_grad
        s = ch.sample(val, 6, seed=2, constrained=True, e=e)
        assert s.shape == (n, 6) and not s.requires_grad
        assert np.abs(con.C @ s.cpu().numpy() - np.arange(3.0)[:, None]).max() <= emu.residual_bar(con.C, s.cpu().numpy(), np.arange(3.0))
        np.testing.assert_allclose(s.cpu().numpy(), ch.f.sample_constrained(6, seed=2, e=np.arange(3.0)),
                                   rtol=1e-12, atol=1e-12)
    finally:
        ch.close()
