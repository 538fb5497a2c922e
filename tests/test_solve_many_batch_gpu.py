"""GPU tests of the blocked batch solve (spllt_hip_solve_many_batch*, batch_solve_many.hip): the kernels of
solve_many with member offsets on the batch's own solve program.  Bars: the scaled backward error of
tests/test_solve_many_gpu.py (1e-14 per vector, against the member's own A_b) and rtol = atol = 1e-12 between two
solves of the project (here: against solve_batch, the other way to the same numbers).  The matrices and the
members are those of tests/test_batch_mult_gpu.py: the smallest at which each path of the kernels exists.
Right-hand sides per member: 1 (one live lane of a block of 16), 16, 17 (17 live in a block of 32), 33 (32 + a
tail of 1), 40 (32 + a tail of 8).  No test provokes a device fault: a member that is not positive definite is a
flagged member, which every kernel skips."""
import functools

import numpy as np
import pytest

import batch_solve_many_ladder as ladder
import capi_ladder
from helpers import bwd_err
from spllt_amd import _lib, api
from test_batch_mult_gpu import NAMES, _case, _lib_allocation, _padded

pytestmark = pytest.mark.gpu

NBATCH = [1, 3, 5]
NRHS = [1, 16, 17, 33, 40]
NV = 40


def _blocks(nrhs, rb=32):
    """blocks per member: 32 while more than 16 are left, a tail of at most 16 is a block of 16"""
    k = 0
    while nrhs > 0:
        nrhs -= 32 if (nrhs > 16 and rb == 32) else 16
        k += 1
    return k


@functools.lru_cache(maxsize=None)
def _rhs(name):
    """(5, NV, n): B_b = A_b X for one random X, so that the solutions are O(1); shared, read-only"""
    c = _case(name)
    X = np.random.default_rng(2).standard_normal((NV, c.n))
    B = np.ascontiguousarray(np.stack([(c.member(b) @ X.T).T for b in range(5)]))   # (C order: vector q of member b is a row)
    B.setflags(write=False)
    return B


def check_members(c, members, got, B, tag):
    """every vector of the given members against its own A_b"""
    worst = 0.0
    for b in members:
        A = c.member(b)
        assert np.isfinite(got[b]).all()
        for q in range(got.shape[1]):
            worst = max(worst, bwd_err(A, got[b, q], B[b, q]))
    print(tag, c.name, "members", list(members), "nrhs", got.shape[1], "max scaled backward error", worst)
    assert worst <= 1e-14


@pytest.mark.parametrize("nbatch", NBATCH)
@pytest.mark.parametrize("name", NAMES)
def test_accuracy(name, nbatch):
    c = _case(name)
    f = c.f
    assert c.batch(nbatch) == 0
    for nrhs in NRHS:
        B = _rhs(name)[:nbatch, :nrhs]
        got = f.solve_many_batch(B if nrhs > 1 else B[:, 0]).reshape(nbatch, nrhs, c.n)
        check_members(c, range(nbatch), got, B, "accuracy")
        want = f.solve_batch(B if nrhs > 1 else B[:, 0]).reshape(nbatch, nrhs, c.n)
        print("accuracy", name, "nbatch", nbatch, "nrhs", nrhs, "max|blocked - solve_batch|", np.abs(got - want).max())
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)
        # it is the blocked path: blocks of 32, a tail of at most 16 as a block of 16
        info = f.solve_many_batch_info()
        assert info["rb"] == 32 and info["blocks"] == _blocks(nrhs) and info["launches"] > 0
        assert info["workspace_bytes"] >= nbatch * 32 * c.n * 8


@pytest.mark.parametrize("name", NAMES)
def test_jobs(name):
    c = _case(name)
    f, nbatch = c.f, 3
    assert c.batch(nbatch) == 0
    B = _rhs(name)[:nbatch, :17]
    x0 = f.solve_many_batch(B, 0)
    np.testing.assert_allclose(f.solve_many_batch(f.solve_many_batch(B, 1), 2), x0, rtol=1e-12, atol=1e-12)
    for job in (1, 2):
        np.testing.assert_allclose(f.solve_many_batch(B, job), f.solve_batch(B, job), rtol=1e-12, atol=1e-12)
    X = c.X[:nbatch, :5]
    for job in (0, 1, 2):
        np.testing.assert_allclose(f.factor_mult_batch(f.solve_many_batch(X, job), job), X, rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(f.solve_many_batch(f.factor_mult_batch(X, job), job), X, rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("name", NAMES)
def test_layout_and_entry_points(name):
    import torch
    c = _case(name)
    f, nbatch, n = c.f, 3, c.n
    assert c.batch(nbatch) == 0
    lib = f.lib
    nrhs, ldx = 17, n + 7
    B = _rhs(name)[:nbatch, :nrhs]
    nan = float("nan")
    for job in (0, 1, 2):
        want = f.solve_many_batch(B, job)
        img = _padded(B, ldx, sentinel=nan)
        xh = img.copy()
        assert lib.spllt_hip_solve_many_batch(f.fkeep, nrhs, xh.ctypes.data, ldx, job) == 0, f.last_error()
        # what lies between the vectors and behind the last member is bit-identical (NaN sentinels: as bytes)
        assert xh[:, n:].tobytes() == img[:, n:].tobytes() and xh[nbatch * nrhs:].tobytes() == img[nbatch * nrhs:].tobytes()
        np.testing.assert_allclose(xh[:nbatch * nrhs, :n].reshape(nbatch, nrhs, n), want, rtol=1e-12, atol=1e-12)
        xd = torch.tensor(img, device="cuda")
        torch.cuda.synchronize()
        assert f.solve_many_batch_dev(xd.data_ptr(), nrhs, ldx=ldx, job=job) == 0
        dimg = xd.cpu().numpy()
        assert dimg[:, n:].tobytes() == img[:, n:].tobytes() and dimg[nbatch * nrhs:].tobytes() == img[nbatch * nrhs:].tobytes()
        np.testing.assert_allclose(dimg[:nbatch * nrhs, :n].reshape(nbatch, nrhs, n), want, rtol=1e-12, atol=1e-12)
        pimg = img.copy()
        pimg[:nbatch * nrhs, c.order] = img[:nbatch * nrhs, :n]
        pd_ = torch.tensor(pimg, device="cuda")
        torch.cuda.synchronize()
        assert f.solve_many_batch_dev(pd_.data_ptr(), nrhs, ldx=ldx, job=job, pivot_order=True) == 0
        got = pd_.cpu().numpy()
        assert got[:, n:].tobytes() == img[:, n:].tobytes()
        np.testing.assert_allclose(got[:nbatch * nrhs, c.order].reshape(nbatch, nrhs, n), want, rtol=1e-12, atol=1e-12)
    # nrhs = 0 is a no-op
    x = np.full(n, 3.0)
    assert lib.spllt_hip_solve_many_batch(f.fkeep, 0, x.ctypes.data, n, 0) == 0 and (x == 3.0).all()
    xd = torch.full((n,), 3.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    assert f.solve_many_batch_dev(xd.data_ptr(), 0) == 0 and bool((xd == 3.0).all())


@pytest.mark.parametrize("name", NAMES)
def test_independence(name):
    c = _case(name)
    f, nbatch = c.f, 3
    assert c.batch(nbatch) == 0
    lib = f.lib
    B = _rhs(name)[:nbatch]
    tol = dict(rtol=1e-12, atol=1e-12)
    for job in (0, 2):
        x = f.solve_many_batch(B, job)
        np.testing.assert_allclose(f.solve_many_batch(B[:, :17], job), x[:, :17], **tol)      # a block of 17
        for q in (0, 16, 32, 39):                                                          # alone
            np.testing.assert_allclose(f.solve_many_batch(B[:, q], job), x[:, q], **tol)
        perm = np.random.default_rng(1).permutation(NV)                                    # its place in the block
        np.testing.assert_allclose(f.solve_many_batch(B[:, perm], job), x[:, perm], **tol)
        B2 = B.copy()                                                                      # the other vectors of its member
        B2[:, 1:] *= -3.0
        np.testing.assert_allclose(f.solve_many_batch(B2, job)[:, 0], x[:, 0], **tol)
        B3 = B.copy()                                                                      # the other members' vectors
        B3[0], B3[2] = 3.0 * B[2], -B[0]
        np.testing.assert_allclose(f.solve_many_batch(B3, job)[1], x[1], **tol)
        # blocks of 16 only (what is left when the workspace of 32 does not fit)
        f.release_solve_many_batch()
        assert f.solve_many_batch_info()["rb"] == 0
        assert lib.spllt_hip_debug(b"fmult_alloc_fail=1") == 0
        try:
            x16 = f.solve_many_batch(B, job)
        finally:
            assert lib.spllt_hip_debug(b"fmult_alloc_fail=0") == 0
        info = f.solve_many_batch_info()
        assert info["rb"] == 16 and info["blocks"] == _blocks(NV, 16) == 3
        np.testing.assert_allclose(x16, x, **tol)
        f.release_solve_many_batch()                       # after a release the storage is taken again, blocks of 32
        np.testing.assert_allclose(f.solve_many_batch(B, job), x, **tol)
        assert f.solve_many_batch_info()["rb"] == 32


@pytest.mark.parametrize("nbatch,bad", [(3, 0), (3, 1), (5, 4), (1, 0)])
@pytest.mark.parametrize("name", NAMES)
def test_failed_member(name, nbatch, bad):
    import torch
    c = _case(name)
    f, n = c.f, c.n
    assert c.batch(nbatch, bad) == -20
    B = _rhs(name)[:nbatch, :17]
    good = [b for b in range(nbatch) if b != bad]
    for job in (0, 1, 2):
        x = B.copy()
        rc = f.lib.spllt_hip_solve_many_batch(f.fkeep, 17, x.ctypes.data, n, job)
        assert rc == -20 and "spllt_hip_solve_many_batch: " in f.last_error() and "unchanged" in f.last_error()
        assert np.array_equal(x[bad], B[bad])
        if job == 0:
            check_members(c, good, x, B, "failed member %d" % bad)
        assert np.array_equal(f.solve_many_batch(B, job)[bad], B[bad])          # (Python: no exception)
        xd = torch.tensor(np.ascontiguousarray(B), device="cuda")
        torch.cuda.synchronize()
        assert xd.is_contiguous() and f.solve_many_batch_dev(xd.data_ptr(), 17, job=job) == -20
        got = xd.cpu().numpy()
        assert np.array_equal(got[bad], B[bad])
        if good:
            np.testing.assert_allclose(got[good], x[good], rtol=1e-12, atol=1e-12)
    # the samples of the flagged member are NaN with the switch on as with it off
    f.set_batch_blocked_solve(True)
    try:
        S = f.sample_batch(4, seed=3, kind="precision", mean=np.ones(n))
        assert np.isnan(S[bad]).all() and np.isfinite(S[good]).all()
        x = np.zeros((nbatch, 4, n))
        rc = f.lib.spllt_hip_sample_batch(f.fkeep, 4, x.ctypes.data, n, 0, 3, 0, 0, 1, None, 0)
        assert rc == -20 and "spllt_hip_sample_batch: " in f.last_error() and "NaN" in f.last_error()
    finally:
        f.set_batch_blocked_solve(False)
    assert c.batch(nbatch) == 0                       # the handle is still good


def test_member_ranges():
    c = _case("box11-nb64")
    f = c.f
    lib = f.lib
    B = _rhs(c.name)[:, :17]
    launches = {}
    for nbatch in (2, 5):
        assert c.batch(nbatch) == 0
        x = f.solve_many_batch(B[:nbatch])
        launches[nbatch] = f.solve_many_batch_info()["launches"]
        assert lib.spllt_hip_debug(b"batch_grid_limit=1") == 0       # one member per launch
        try:
            xr = f.solve_many_batch(B[:nbatch])
        finally:
            assert lib.spllt_hip_debug(b"batch_grid_limit=0") == 0
        np.testing.assert_allclose(xr, x, rtol=1e-12, atol=1e-12)
        assert f.solve_many_batch_info()["launches"] == nbatch * launches[nbatch]
    # without the hook the number of launches does not depend on nbatch
    assert launches[2] == launches[5] > 2


@pytest.mark.parametrize("name", NAMES)
def test_sampling(name):
    c = _case(name)
    f, n, nbatch, ns = c.f, c.n, 3, 35
    assert c.batch(nbatch) == 0
    mB = np.random.default_rng(4).standard_normal((nbatch, n))
    for common in (False, True):
        kw = dict(seed=11, mean=mB, common_noise=common)
        off = {k: f.sample_batch(ns, kind=k, **kw) for k in ("precision", "covariance")}
        Z = f.white_noise_batch(ns, seed=11, common_noise=common)
        assert f.set_batch_blocked_solve(True) is False
        try:
            on = {k: f.sample_batch(ns, kind=k, **kw) for k in ("precision", "covariance")}
            assert np.array_equal(f.white_noise_batch(ns, seed=11, common_noise=common), Z)
        finally:
            assert f.set_batch_blocked_solve(False) is True
        assert np.array_equal(on["covariance"], off["covariance"])
        print("sampling", name, "max|on - off|", np.abs(on["precision"] - off["precision"]).max())
        np.testing.assert_allclose(on["precision"], off["precision"], rtol=1e-12, atol=1e-12)
        # and it is the backward sweep on the noise
        Zu = np.ascontiguousarray(Z[:, c.order, :].transpose(0, 2, 1))
        np.testing.assert_allclose(on["precision"], mB[:, None, :] + f.solve_many_batch(Zu, job=2), rtol=1e-12, atol=1e-12)


def test_lifetime():
    c = _case("box11-nb64")
    f = c.f
    B = _rhs(c.name)[:, :5]
    tol = dict(rtol=1e-12, atol=1e-12)
    f.factor(c.val).wait()
    Bs = np.asfortranarray(B[0].T)
    single = f.solve_many(Bs)
    assert c.batch(2) == 0
    f.release_solve_many_batch()                         # (the handle is shared: what an earlier test took)
    sb = f.solve_batch(B[:2])
    x2 = f.solve_many_batch(B[:2])
    bytes2 = f.solve_many_batch_info()["workspace_bytes"]
    assert c.batch(5) == 0                               # a larger batch is picked up
    x5 = f.solve_many_batch(B)
    assert f.solve_many_batch_info()["workspace_bytes"] > bytes2
    check_members(c, range(5), x5, B, "lifetime")
    np.testing.assert_allclose(x5[:2], x2, **tol)
    np.testing.assert_allclose(f.solve_batch(B)[:2], sb, **tol)
    f.release_batch()                                    # ... takes the storage with it
    assert f.solve_many_batch_info()["rb"] == 0 and f.solve_many_batch_info()["workspace_bytes"] == 0
    with pytest.raises(api.SplltError) as ei:
        f.solve_many_batch(B)
    assert ei.value.flag == -10 and "no batch" in f.last_error()
    assert c.batch(3) == 0
    x3 = f.solve_many_batch(B[:3])
    np.testing.assert_allclose(x3, x5[:3], **tol)
    f.release_solve_many_batch()
    f.release_solve_many_batch()
    assert f.solve_many_batch_info()["rb"] == 0
    np.testing.assert_allclose(f.solve_many(Bs), single, **tol)
    np.testing.assert_allclose(f.solve_batch(B[:3])[:2], sb, **tol)
    np.testing.assert_allclose(f.solve_many_batch(B[:3]), x3, **tol)
    assert f.solve_many_batch_info()["rb"] == 32
    np.testing.assert_allclose(f.solve_many(Bs), single, **tol)


def test_allocation_failure_leaves_the_batch_and_the_solves_usable():
    c = _case("box11-nb64")
    f = c.f
    f.factor(c.val).wait()
    assert c.batch(3) == 0
    B = _rhs(c.name)[:3, :3]
    xb = f.solve_batch(B)
    xs = f.solve(B[0, 0])
    f.release_solve_many_batch()
    assert f.lib.spllt_hip_debug(b"fmult_alloc_fail=2") == 0      # blocks of 32 and blocks of 16
    try:
        with pytest.raises(api.SplltError) as ei:
            f.solve_many_batch(B)
    finally:
        assert f.lib.spllt_hip_debug(b"fmult_alloc_fail=0") == 0
    assert ei.value.flag == _lib_allocation() and "memory" in f.last_error()
    assert f.solve_many_batch_info()["rb"] == 0 and f.solve_many_batch_info()["workspace_bytes"] == 0
    np.testing.assert_allclose(f.solve_batch(B), xb, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(f.solve(B[0, 0]), xs, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(f.solve_many_batch(B), xb, rtol=1e-12, atol=1e-12)


def test_errors():
    c = _case("p2d12-nb8")
    f, n = c.f, c.n
    assert c.batch(2) == 0
    x = np.ones(2 * 3 * n)
    p = x.ctypes.data
    assert f.lib.spllt_hip_solve_many_batch(f.fkeep, 3, p, n, 3) == -10
    assert f.lib.spllt_hip_solve_many_batch(f.fkeep, 3, p, n - 1, 0) == -10
    assert f.lib.spllt_hip_solve_many_batch(f.fkeep, -1, p, n, 0) == -10
    assert f.lib.spllt_hip_solve_many_batch(f.fkeep, 3, None, n, 0) == -10
    assert (x == 1.0).all()
    with pytest.raises(ValueError):
        f.solve_many_batch(np.zeros((3, n)))            # the batch has two members


@pytest.mark.parametrize("state", ["analysed", "engine", "factored", "batch", "batch_inverse"])
def test_ladder_on_the_gpu(state):
    cx = capi_ladder.Ctx(_lib.load(), True)
    rows = ladder.check_state(cx, state, ladder.golden(True))
    assert rows == 2 * 6 + 2 + 2 + 2


# ---- torch ------------------------------------------------------------------------------------------
def test_torch_batch_blocked():
    import torch
    from spllt_amd.torch_ops import SparseCholesky
    c = _case("box11-nb64")
    n, nbatch, nrhs = c.n, 3, 2
    default = SparseCholesky(c.A, nb=64, nemin=16)
    blocked = SparseCholesky(c.A, nb=64, nemin=16, batch_blocked=True)
    assert blocked.batch_blocked and not default.batch_blocked
    rng = np.random.default_rng(4)
    vals = c.values(nbatch)
    B = np.stack([c.member(b) @ rng.standard_normal((n, nrhs)) for b in range(nbatch)])
    G = rng.standard_normal((nbatch, n, nrhs))
    out = {}
    for key, chol in (("default", default), ("blocked", blocked)):
        tv = torch.tensor(vals, device="cuda", requires_grad=True)
        tb = torch.tensor(B, device="cuda", requires_grad=True)
        X = chol.solve_batch(tv, tb)
        assert X.shape == (nbatch, n, nrhs)
        (X * torch.tensor(G, device="cuda")).sum().backward()
        out[key] = (X.detach().cpu().numpy(), tb.grad.cpu().numpy(), tv.grad.cpu().numpy())
        if key == "blocked":
            # both passes went through the blocked path, and the gradient to vals is the sampled outer product
            assert chol.f.solve_many_batch_info()["rb"] == 32 and chol.f.solve_many_batch_info()["blocks"] == 1
            for b in range(nbatch):
                assert torch.equal(tv.grad[b], chol.pattern_outer(tb.grad[b], X[b].detach(), alpha=-1.0)), b
        else:
            assert chol.f.solve_many_batch_info()["rb"] == 0
    x, lam, gv = out["blocked"]
    for b in range(nbatch):
        for q in range(nrhs):
            ex, el = bwd_err(c.member(b), x[b, :, q], B[b, :, q]), bwd_err(c.member(b), lam[b, :, q], G[b, :, q])
            print(f"member {b} column {q}: bwd_err x {ex:.2e} lambda {el:.2e}")
            assert ex <= 1e-14 and el <= 1e-14
    for got, want in zip(out["blocked"], out["default"]):
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)
    # sampling: the precision kind to rounding, the covariance kind bit for bit, the switch back where it was
    tv = torch.tensor(vals, device="cuda")
    mB = torch.tensor(rng.standard_normal((nbatch, n)), device="cuda")
    # (on ONE instance, whose cached factors both draws use: two factorizations of a batch agree to rounding only)
    for kind in ("precision", "covariance"):
        a = blocked.sample_batch(tv, 6, seed=9, kind=kind, mean=mB).cpu().numpy()
        blocked.batch_blocked = False
        try:
            b_ = blocked.sample_batch(tv, 6, seed=9, kind=kind, mean=mB).cpu().numpy()
        finally:
            blocked.batch_blocked = True
        if kind == "covariance":
            assert np.array_equal(a, b_)
        else:
            np.testing.assert_allclose(a, b_, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(a, default.sample_batch(tv, 6, seed=9, kind=kind, mean=mB).cpu().numpy(),
                                   rtol=1e-12, atol=1e-12)
    assert blocked.f.set_batch_blocked_solve(False) is False
    rep = SparseCholesky(c.A, nb=64, nemin=16, reproducible=True, batch_blocked=True)
    with pytest.raises(NotImplementedError):
        rep.solve_batch(None, None)
    with pytest.raises(NotImplementedError):
        rep.sample_batch(tv, 2)
    for chol in (default, blocked, rep):
        chol.close()
