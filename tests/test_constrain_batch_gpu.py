"""GPU tests of the hard linear constraints of a batch (include/spllt_hip_constrain_batch.h,
spllt_amd/csrc/constrain_batch.hip) against the per-member dense emulation of constrain_batch_emulate.py and the KKT
solve.  The matrices, k and nvec are those of tests/test_constrain_gpu.py -- the smallest at which the tiling can go
wrong: n = 64 (one chunk), 144 (three chunks, a tail of 16), 125 (no multiple of 4, 16 or 64); every count of 16-row
tiles of C with and without a tail; a block of 16, one of 32, 32 + a tail -- with three members (five in the test of
the member that is not positive definite).  ldx = n + 3, ldc = n + 5, lde = k + 1, ldl = k + 2, all padding NaN.
No test provokes a device fault: a member that is not positive definite is a flagged member, which every kernel of
the family skips."""
import ctypes as C
import functools

import numpy as np
import pytest

import capi_ladder
import constrain_batch_emulate as bemu
import constrain_batch_ladder as ladder
import constrain_emulate as emu
from spllt_amd import _lib, api

pytestmark = pytest.mark.gpu

NAN = float("nan")
NB = bemu.NBATCH
ALL_NVEC_CASE = ("p2d12", 17)


class Case:
    def __init__(self, name):
        self.m = bemu.matrix(name)
        self.n = self.m.n
        self.f = self.new_handle()
        assert self.f.factor_batch(self.m.values(NB)) == 0

    def new_handle(self):
        m = self.m
        return api.Factorization(m.n, m.ptr, m.row, nb=m.nb, nemin=m.nemin)


@functools.lru_cache(maxsize=None)
def _case(name):
    return Case(name)


def _vp(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _set(f, Crows, dev=False):
    """spllt_hip_set_constraints_batch(_dev) with ldc = n + 5 and NaN in the padding"""
    k, n = Crows.shape
    cp = np.full((k, n + 5), NAN)
    cp[:, :n] = Crows
    if dev:
        import torch
        ct = torch.tensor(cp, device="cuda")
        return f.lib.spllt_hip_set_constraints_batch_dev(f.fkeep, k, C.c_void_p(ct.data_ptr()), n + 5)
    return f.lib.spllt_hip_set_constraints_batch(f.fkeep, k, cp.ctypes.data_as(C.POINTER(C.c_double)), n + 5)


def _padded(M, ld):
    """M (B, nvec, len) as vectors at (b * nvec + q) * ld, padding NaN"""
    out = np.full(M.shape[:2] + (ld,), NAN)
    out[:, :, :M.shape[2]] = M
    return out


def _run(f, entry, X, e, k, dev, want_rc=0):
    """entry (constrain / solve_constrained) on padded arrays; X (B, nvec, n); e: None, (k,) or (B, nvec, k).
    Returns (x, lambda) of shapes (B, nvec, n) and (B, nvec, k) after checking that no padding was touched."""
    nb, nvec, n = X.shape
    xp = _padded(X, n + 3)
    lp = np.full((nb, nvec, k + 2), NAN)
    ep, lde = None, 0
    if e is not None and e.ndim == 1:
        ep = e.copy()
    elif e is not None:
        ep, lde = _padded(e, k + 1), k + 1
    if dev:
        import torch
        xt, lt = torch.tensor(xp, device="cuda"), torch.tensor(lp, device="cuda")
        et = None if ep is None else torch.tensor(ep, device="cuda")
        torch.cuda.synchronize()
        rc = getattr(f.lib, f"spllt_hip_{entry}_batch_dev")(f.fkeep, nvec, C.c_void_p(xt.data_ptr()), n + 3,
                                                             None if et is None else C.c_void_p(et.data_ptr()), lde,
                                                             C.c_void_p(lt.data_ptr()), k + 2)
        xp, lp = xt.cpu().numpy(), lt.cpu().numpy()
    else:
        rc = getattr(f.lib, f"spllt_hip_{entry}_batch")(f.fkeep, nvec, _vp(xp), n + 3, _vp(ep), lde, _vp(lp), k + 2)
    assert rc == want_rc, (entry, rc, f.last_error())
    assert np.isnan(xp[:, :, n:]).all() and np.isnan(lp[:, :, k:]).all()
    return xp[:, :, :n].copy(), lp[:, :, :k].copy()


def _targets(rng, nb, nvec, k):
    return (None, rng.standard_normal(k), rng.standard_normal((nb, nvec, k)))


def _assert_residual(bc, x, e):
    for b, E in enumerate(bc.targets(e, x.shape[1])):
        r = np.abs(bc.C @ x[b].T - E).max()
        assert r <= emu.residual_bar(bc.C, x[b], None if e is None else E), (b, r)


# ---- 1. constrain_batch and solve_constrained_batch against the emulation and the KKT solve ----------------------
@pytest.mark.parametrize("name,k", bemu.CASES)
def test_constrain_and_solve_constrained(name, k):
    c, bc = _case(name), bemu.batch(name, k)
    f, n = c.f, c.n
    assert _set(f, bc.C, dev=k % 2 == 0) == 0, f.last_error()
    rng = np.random.default_rng(17 * k + n)
    for nvec in (bemu.NVECS if (name, k) == ALL_NVEC_CASE else (1, 33, 40)):
        X = rng.standard_normal((NB, nvec, n))
        for e in _targets(rng, NB, nvec, k):
            want_x, want_l = bc.correct(X, e)
            xh, lh = _run(f, "constrain", X, e, k, False)
            xd, ld = _run(f, "constrain", X, e, k, True)
            assert not np.isnan(xh).any() and not np.isnan(lh).any()
            assert np.array_equal(xh, xd) and np.array_equal(lh, ld)       # one arithmetic behind both entry points
            np.testing.assert_allclose(xh, want_x, rtol=1e-12, atol=1e-12)
            np.testing.assert_allclose(lh, want_l, rtol=1e-12, atol=1e-12)
            _assert_residual(bc, xh, e)
            want_x, want_l = bc.solve_constrained(X, e)
            kkt_x, kkt_l = bc.kkt_solve(X, e)
            for dev in (False, True):
                x, lam = _run(f, "solve_constrained", X, e, k, dev)
                np.testing.assert_allclose(x, want_x, rtol=1e-12, atol=1e-12)
                np.testing.assert_allclose(lam, want_l, rtol=1e-12, atol=1e-12)
                np.testing.assert_allclose(x, kkt_x, rtol=1e-12, atol=1e-12)
                np.testing.assert_allclose(lam, kkt_l, rtol=1e-12, atol=1e-12)
                _assert_residual(bc, x, e)
    # the Python wrappers: the same numbers, the shapes of solve_many_batch
    X = rng.standard_normal((NB, 5, n))
    E = rng.standard_normal((NB, 5, k))
    x, lam = f.solve_constrained_batch(X, e=E, multipliers=True)
    wx, wl = bc.solve_constrained(X, E)
    assert x.shape == (NB, 5, n) and lam.shape == (NB, 5, k) and f.constrain_batch_status == 0
    np.testing.assert_allclose(x, wx, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(lam, wl, rtol=1e-12, atol=1e-12)
    x1, l1 = f.constrain_batch(X[:, 0], multipliers=True)
    assert x1.shape == (NB, n) and l1.shape == (NB, k)
    assert np.array_equal(x1, f.constrain_batch(X[:, :1])[:, 0])


# ---- 2. fixed arithmetic ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", [("p2d12", 17), ("p3d5", 64)])
def test_fixed_arithmetic(name, k):
    c, bc = _case(name), bemu.batch(name, k)
    f, n = c.f, c.n
    assert _set(f, bc.C) == 0
    rng = np.random.default_rng(5)
    X, E = rng.standard_normal((NB, 40, n)), rng.standard_normal((NB, 40, k))
    for dev in (False, True):
        x, lam = _run(f, "constrain", X, E, k, dev)
        x2, lam2 = _run(f, "constrain", X, E, k, dev)
        assert np.array_equal(x, x2) and np.array_equal(lam, lam2)
        # vector 37 of 40 alone: another pass width, another place in its pass
        x37, l37 = _run(f, "constrain", X[:, 37:38], E[:, 37:38], k, dev)
        assert np.array_equal(x37[:, 0], x[:, 37]) and np.array_equal(l37[:, 0], lam[:, 37])
        # member b with the OTHER members' vectors and targets replaced
        for b in range(NB):
            Xo, Eo = rng.standard_normal(X.shape), rng.standard_normal(E.shape)
            Xo[b], Eo[b] = X[b], E[b]
            xo, lo = _run(f, "constrain", Xo, Eo, k, dev)
            assert np.array_equal(xo[b], x[b]) and np.array_equal(lo[b], lam[b])


# ---- 3. constrained samples ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", [("p2d8", 3), ("p2d12", 33), ("p3d5", 17)])
def test_sample_constrained(name, k):
    import torch
    c, bc = _case(name), bemu.batch(name, k)
    f, n, ns = c.f, c.n, 35
    assert _set(f, bc.C) == 0
    order = f.sym("order")
    rng = np.random.default_rng(k)
    mB, e = rng.standard_normal((NB, n)), rng.standard_normal(k)
    for common in (False, True):
        Z = f.white_noise_batch(ns, seed=11, common_noise=common)               # (B, n, ns), pivot order
        Zu = np.ascontiguousarray(Z[:, order, :].transpose(0, 2, 1))           # the noise laid out in user positions
        plain = mB[:, None, :] + f.solve_many_batch(Zu, job=2)
        want, _ = bc.correct(plain, e)
        got = f.sample_constrained_batch(ns, seed=11, mean=mB, e=e, common_noise=common)
        assert got.shape == (NB, ns, n) and f.constrain_batch_status == 0
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)
        _assert_residual(bc, got, e)
        # the corrected samples of sample_batch itself
        also, _ = bc.correct(f.sample_batch(ns, seed=11, mean=mB, common_noise=common), e)
        np.testing.assert_allclose(got, also, rtol=1e-12, atol=1e-12)
        # first_sample slices the same draws
        tail = f.sample_constrained_batch(ns - 33, seed=11, mean=mB, e=e, common_noise=common, first_sample=33)
        np.testing.assert_allclose(tail, got[:, 33:], rtol=1e-12, atol=1e-12)
    # e absent: zeros; a shared mean
    m1 = rng.standard_normal(n)
    got0 = f.sample_constrained_batch(5, seed=3, mean=m1)
    want0, _ = bc.correct(f.sample_batch(5, seed=3, mean=m1), None)
    np.testing.assert_allclose(got0, want0, rtol=1e-12, atol=1e-12)
    _assert_residual(bc, got0, None)
    # _dev with NaN padding, a mean per member
    ldx, ldm = n + 3, n + 2
    xd = torch.full((NB * ns + 1, ldx), NAN, dtype=torch.float64, device="cuda")
    mp = np.full((NB, ldm), NAN)
    mp[:, :n] = mB
    md, ed = torch.tensor(mp, device="cuda"), torch.tensor(e, device="cuda")
    torch.cuda.synchronize()
    assert f.sample_constrained_batch_dev(xd.data_ptr(), ns, ldx=ldx, seed=11, mean_dev_ptr=md.data_ptr(), ldmean=ldm,
                                          e_dev_ptr=ed.data_ptr(), common_noise=True) == 0
    img = xd.cpu().numpy()
    assert np.isnan(img[:, n:]).all() and np.isnan(img[NB * ns]).all()
    np.testing.assert_allclose(img[:NB * ns, :n].reshape(NB, ns, n), got, rtol=1e-12, atol=1e-12)


# ---- 4. constrained marginal variances ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", [("p2d8", 1), ("p2d12", 64), ("p3d5", 33)])
def test_inverse_diag_constrained(name, k):
    c, bc = _case(name), bemu.batch(name, k)
    f, n = c.f, c.n
    assert f.factor_batch(c.m.values(NB)) == 0           # (a new batch: whatever Z the handle holds is stale)
    assert _set(f, bc.C) == 0
    out = np.zeros((NB, n))
    # refused exactly like inverse_diag_batch without a batch Z or with a stale one
    for call in ("spllt_hip_inverse_diag_batch", "spllt_hip_inverse_diag_constrained_batch"):
        assert getattr(f.lib, call)(f.fkeep, api._dp(out), n) == -10
        assert f.last_error() == call + ": no selected inverse of the current batch (call " \
                                        "spllt_hip_selected_inverse_batch after every spllt_hip_factor_batch)"
    assert f.selected_inverse_batch() == 0
    v, plain = f.inverse_diag_constrained_batch(), f.inverse_diag_batch()
    assert f.constrain_batch_status == 0 and f.constraints_batch_info()["launches"] == 1   # (the gather is the batch's)
    cov = bc.conditional_cov_diag()
    for b, m in enumerate(bc.members):
        assert np.abs(v[b] - cov[b]).max() <= 1e-11 * np.abs(np.linalg.inv(m.A)).max(), b
    assert (v > 0).all() and (v < plain).all()
    assert f.factor_batch(c.m.values(NB)) == 0           # stale again
    assert f.lib.spllt_hip_inverse_diag_constrained_batch(f.fkeep, api._dp(out), n) == -10
    assert "no selected inverse of the current batch" in f.last_error()


# ---- 5. the scalars and the launch counts ------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", [("p2d8", 16), ("p2d12", 64), ("p3d5", 3)])
def test_info(name, k):
    c, bc = _case(name), bemu.batch(name, k)
    f, n = c.f, c.n
    assert _set(f, bc.C) == 0
    info = f.constraints_batch_info()
    assert info["k"] == k and info["launches"] == 3 and info["device_bytes"] > 0
    np.testing.assert_allclose(info["log_det_s"], bc.log_det_s(), rtol=1e-12, atol=1e-12)
    assert np.abs(info["min_relative_pivot"] - bc.min_relative_pivot()).max() <= 1e-11
    X = np.random.default_rng(1).standard_normal((NB, 32, n))
    f.constrain_batch(X)
    assert f.constraints_batch_info()["launches"] == 3
    f.constrain_batch(np.concatenate([X, X[:, :8]], axis=1))      # two passes
    assert f.constraints_batch_info()["launches"] == 6
    # the same counts with one member
    g = c.new_handle()
    assert g.factor_batch(c.m.values(1)) == 0
    assert _set(g, bc.C) == 0 and g.constraints_batch_info()["launches"] == 3
    x1 = g.constrain_batch(X[:1])
    assert g.constraints_batch_info()["launches"] == 3
    # ... and member 0's numbers (not its bits: each handle's U_0 comes out of its own blocked solve, whose strips
    # add atomically)
    np.testing.assert_allclose(x1[0], f.constrain_batch(X)[0], rtol=1e-12, atol=1e-12)
    g.close()


# ---- 6. dependent rows -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["zero", "duplicate", "nan"])
def test_dependent_rows_are_refused(what):
    c = _case("p2d12")
    f, n = c.f, c.n
    Crows = emu.constraint_rows(6, n).copy()
    if what == "zero":
        Crows[4] = 0.0
    elif what == "duplicate":
        Crows[4] = Crows[1]
    else:
        Crows[4, n // 2] = NAN
    rc = _set(f, Crows)
    err = f.last_error()
    # (a NaN in row 5 poisons column 5 of S_b from row 5 on: the first pivot that is not finite is that of row 5)
    assert rc == -20 and "member 0, row 5 of C" in err and err.startswith("set_constraints_batch:"), (rc, err)
    info = f.constraints_batch_info()
    assert info["k"] == 0 and info["device_bytes"] == 0
    with pytest.raises(api.SplltError) as ei:
        f.set_constraints_batch(Crows)
    assert ei.value.flag == -20
    X = np.random.default_rng(2).standard_normal((NB, 3, n))
    Xc = X.copy()
    assert f.lib.spllt_hip_constrain_batch(f.fkeep, 3, _vp(Xc), n, None, 0, None, 0) == -10 and np.array_equal(Xc, X)
    assert "no constraints are set on this batch" in f.last_error()
    # the batch and its solves are as they were
    x = f.solve_many_batch(X)
    for b in range(NB):
        np.testing.assert_allclose(x[b].T, np.linalg.solve(c.m.member(b)[0], X[b].T), rtol=1e-12, atol=1e-12)


# ---- 7. a later batch is picked up; the single handle's constraints are another state ------------------------------
def test_later_batch_is_picked_up_and_single_handle_is_independent():
    name, k = "p3d5", 17
    c = _case(name)
    n, m = c.n, c.m
    f = c.new_handle()
    rng = np.random.default_rng(3)
    X = rng.standard_normal((5, 4, n))
    assert f.factor_batch(m.values(NB)) == 0
    f.set_constraints_batch(bemu.rows(name, k))
    r0 = f.constraints_batch_info()["rebuilds"]
    np.testing.assert_allclose(f.solve_constrained_batch(X[:NB]), bemu.batch(name, k).solve_constrained(X[:NB])[0],
                               rtol=1e-12, atol=1e-12)
    # the single handle on the same handle: its own C, its own factor
    f.factor(m.val).wait()
    C1 = emu.constraint_rows(3, n, seed=1)
    con1 = emu.Constraints(m.A.toarray(), C1)
    f.set_constraints(C1)
    np.testing.assert_allclose(f.constrain(X[0].T), con1.correct(X[0].T)[0], rtol=1e-12, atol=1e-12)
    assert f.constraints_info()["k"] == 3 and f.constraints_batch_info()["k"] == k
    assert f.constraints_batch_info()["rebuilds"] == r0
    # doubled values: one rebuild, the new numbers
    assert f.factor_batch(m.values(NB, 2.0)) == 0
    assert np.isnan(f.constraints_batch_info()["log_det_s"]).all()            # (never the old batch's numbers)
    bc2 = bemu.batch(name, k, NB, 2.0)
    np.testing.assert_allclose(f.solve_constrained_batch(X[:NB]), bc2.solve_constrained(X[:NB])[0], rtol=1e-12, atol=1e-12)
    info = f.constraints_batch_info()
    assert info["rebuilds"] == r0 + 1
    np.testing.assert_allclose(info["log_det_s"], bc2.log_det_s(), rtol=1e-12, atol=1e-12)
    f.constrain_batch(X[:NB])
    assert f.constraints_batch_info()["rebuilds"] == r0 + 1 and f.constraints_batch_info()["launches"] == 3
    # a batch with MORE members: the storage is taken again, C is kept
    bytes3 = info["device_bytes"]
    assert f.factor_batch(m.values(5)) == 0
    x5, l5 = f.solve_constrained_batch(X, multipliers=True)
    w5, wl5 = bemu.batch(name, k, 5).solve_constrained(X)
    np.testing.assert_allclose(x5, w5, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(l5, wl5, rtol=1e-12, atol=1e-12)
    info = f.constraints_batch_info()
    assert info["rebuilds"] == r0 + 2 and info["device_bytes"] > bytes3 and info["log_det_s"].shape == (5,)
    # the single handle's constraints were not touched, and do not touch the batch's
    np.testing.assert_allclose(f.constrain(X[0].T), con1.correct(X[0].T)[0], rtol=1e-12, atol=1e-12)
    f.release_constraints()
    assert f.constraints_info()["k"] == 0 and f.constraints_batch_info()["k"] == k
    assert np.array_equal(f.constrain_batch(X), f.constrain_batch(X))
    f.close()


# ---- 8. a member that is not positive definite -------------------------------------------------------------------
def test_member_that_is_not_positive_definite():
    import torch
    name, k, nbatch, bad = "p2d12", 17, 5, 1
    c = _case(name)
    n, m = c.n, c.m
    f = c.new_handle()
    vals = m.values(nbatch).copy()
    j = n // 2
    vals[bad, f.ptr[j] - 1] *= -1.0              # the diagonal entry of variable j (as tests/test_factor_batch_gpu.py)
    assert vals[bad, f.ptr[j] - 1] < 0 and f.row[f.ptr[j] - 1] == j + 1
    assert f.factor_batch(vals) == -20
    bc = bemu.batch(name, k, nbatch)
    good = [b for b in range(nbatch) if b != bad]
    assert _set(f, bc.C) == -20 and "not positive definite" in f.last_error()
    info = f.constraints_batch_info()
    assert info["k"] == k
    assert np.isnan(info["log_det_s"][bad]) and np.isnan(info["min_relative_pivot"][bad])
    np.testing.assert_allclose(info["log_det_s"][good], bc.log_det_s()[good], rtol=1e-12, atol=1e-12)
    rng = np.random.default_rng(8)
    X, E = rng.standard_normal((nbatch, 33, n)), rng.standard_normal((nbatch, 33, k))
    for entry, ref in (("constrain", bc.correct), ("solve_constrained", bc.solve_constrained)):
        want_x, want_l = ref(X, E)
        for dev in (False, True):
            x, lam = _run(f, entry, X, E, k, dev, want_rc=-20)
            assert "unchanged" in f.last_error()
            assert np.array_equal(x[bad], X[bad]) and np.isnan(lam[bad]).all()
            np.testing.assert_allclose(x[good], want_x[good], rtol=1e-12, atol=1e-12)
            np.testing.assert_allclose(lam[good], want_l[good], rtol=1e-12, atol=1e-12)
            _assert_residual(bemu.batch(name, k, 1), x[:1], E[:1])
    S = f.sample_constrained_batch(4, seed=3, e=E[0, 0])
    assert f.constrain_batch_status == -20 and np.isnan(S[bad]).all() and np.isfinite(S[good]).all()
    want_s, _ = bc.correct(np.nan_to_num(f.sample_batch(4, seed=3)), E[0, 0])
    np.testing.assert_allclose(S[good], want_s[good], rtol=1e-12, atol=1e-12)
    sd = torch.zeros((nbatch, 4, n), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    assert f.sample_constrained_batch_dev(sd.data_ptr(), 4, seed=3) == -20
    assert np.isnan(sd.cpu().numpy()[bad]).all() and np.isfinite(sd.cpu().numpy()[good]).all()
    assert f.selected_inverse_batch() == -20
    v = f.inverse_diag_constrained_batch()
    assert f.constrain_batch_status == -20 and np.isnan(v[bad]).all()
    cov = bc.conditional_cov_diag()
    for b in good:
        assert np.abs(v[b] - cov[b]).max() <= 1e-11 * np.abs(np.linalg.inv(bc.members[b].A)).max(), b
    f.close()


# ---- 9. the ladder with a device, giving the memory back, the torch front end -----------------------------------
@pytest.mark.parametrize("state", ladder.GPU_STATES)
def test_ladder_with_a_device(state):
    c = capi_ladder.Ctx(_lib.load(), True)
    assert ladder.check_state(c, state, ladder.golden(True)) == ladder.ROWS


def test_release_returns_the_bytes():
    name, k = "p2d8", 3
    c = _case(name)
    f = c.new_handle()
    assert f.factor_batch(c.m.values(NB)) == 0
    owned0 = f.constraints_batch_info()
    assert owned0["device_bytes"] == 0
    n, nc = c.n, 1
    f.set_constraints_batch(bemu.rows(name, k))
    # the formula of the header, in doubles
    want = k * n + NB * k * n + NB * (64 * 64 + 4) + NB * nc * 64 * 64 + NB * 3 * 32 * 64
    assert f.constraints_batch_info()["device_bytes"] == 8 * want
    f.release_constraints_batch()
    info = f.constraints_batch_info()
    assert info["k"] == 0 and info["device_bytes"] == 0
    f.release_constraints_batch()                                # nothing held: a no-op
    with pytest.raises(api.SplltError) as ei:
        f.constrain_batch(np.zeros((NB, n)))
    assert ei.value.flag == -10 and "no constraints are set on this batch" in f.last_error()
    # k = 0 clears; release_batch gives the constraints' storage back with the batch's
    f.set_constraints_batch(bemu.rows(name, k))
    f.set_constraints_batch(None)
    assert f.constraints_batch_info()["k"] == 0
    f.set_constraints_batch(bemu.rows(name, k))
    assert f.constraints_batch_info()["device_bytes"] > 0
    f.release_batch()
    info = f.constraints_batch_info()
    assert info["k"] == 0 and info["device_bytes"] == 0
    with pytest.raises(api.SplltError) as ei:
        f.constrain_batch(np.zeros((NB, n)))
    assert ei.value.flag == -10 and "no batch has been factorized" in f.last_error()
    f.close()


def test_torch_front_end_without_gradients():
    import torch
    from spllt_amd.torch_ops import SparseCholesky
    name, k = "p3d5", 17
    m, bc = bemu.matrix(name), bemu.batch(name, k)
    n = m.n
    chol = SparseCholesky((m.n, m.ptr, m.row), nb=m.nb, nemin=m.nemin)
    vals = torch.tensor(m.values(NB), device="cuda", requires_grad=True)
    rng = np.random.default_rng(4)
    Bn, en = rng.standard_normal((NB, n, 5)), rng.standard_normal(k)
    B = torch.tensor(Bn, device="cuda", requires_grad=True)
    e = torch.tensor(en, device="cuda")
    with pytest.raises(RuntimeError):
        chol.solve_constrained_batch(vals, B)                   # no constraints yet
    chol.set_constraints(torch.tensor(bc.C, device="cuda"))
    x, lam = chol.solve_constrained_batch(vals, B, e=e)
    assert x.shape == (NB, n, 5) and lam.shape == (NB, k, 5) and not x.requires_grad and not lam.requires_grad
    wx, wl = bc.solve_constrained(Bn.transpose(0, 2, 1), en)
    np.testing.assert_allclose(x.cpu().numpy().transpose(0, 2, 1), wx, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(lam.cpu().numpy().transpose(0, 2, 1), wl, rtol=1e-12, atol=1e-12)
    mean = torch.tensor(rng.standard_normal((NB, n)), device="cuda", requires_grad=True)
    S = chol.sample_batch(vals, 6, seed=5, mean=mean, constrained=True, e=e)
    assert S.shape == (NB, n, 6) and not S.requires_grad
    plain = chol.sample_batch(vals, 6, seed=5, mean=mean).cpu().numpy().transpose(0, 2, 1)
    np.testing.assert_allclose(S.cpu().numpy().transpose(0, 2, 1), bc.correct(plain, en)[0], rtol=1e-12, atol=1e-12)
    with pytest.raises(ValueError):
        chol.sample_batch(vals, 6, e=e)                         # e needs constrained=True
    with pytest.raises(ValueError):
        chol.sample_batch(vals, 6, kind="covariance", constrained=True)
    with pytest.raises(ValueError):
        chol.solve_constrained_batch(vals, B, e=torch.zeros(k + 1, dtype=torch.float64, device="cuda"))
