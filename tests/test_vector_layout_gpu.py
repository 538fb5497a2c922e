"""GPU tests of what the vector entry points share: the device order table and the permutation kernel (one
workgroup of 256 per 256 variables and vector), on padded vectors.  n = 4, 256 and 289: less than a workgroup,
exactly one, one and a partial one.  Five right-hand sides: a sweep of 4 + 1 for the reproducible solve, one
zero-padded block of 16 for the blocked solve.  Every vector lies at x[q * ldx ..] with ldx = n + 7, two spare
vectors behind the used ones, every slot outside the vectors holds a sentinel that must come back untouched.

The reproducible solve and the product have no atomic add: user order, pivot order and the host entry point
must give the same bits (the product is also held to A @ B at the bar of the refine tests).  The blocked
solve and the batch solve add with atomics, so two runs may differ in the last bits: they are held to the
existing bars of their own tests instead (scaled backward error 1e-14 per vector; rtol = atol = 1e-12 against
spllt_solve), in both orders.

The blocked features walk their vectors in blocks of 32 (16 when the workspace of 32 did not fit) and stage a
host call block by block: test_block_walk runs each of them on 49 padded vectors per member, from the host and
on the device, at both widths.  49 = 32 + 17 in a block of 32, or 16 + 16 + 16 + 1."""
import functools

import numpy as np
import pytest

from helpers import bwd_err, make_case
from spllt_amd import matgen

pytestmark = pytest.mark.gpu

KS = [2, 16, 17]
NRHS, SPARE, PAD, SENTINEL = 5, 2, 7, -7.25e77


@functools.lru_cache(maxsize=None)
def _case(k):
    A = matgen.poisson2d(k)
    f, val = make_case(A, nb=16, nemin=4)
    f.factor(val).wait()
    assert f.n == k * k
    B = np.random.default_rng(k).standard_normal((f.n, NRHS))
    return A, f, val, B, f.sym("order"), f.solve(B).reshape(f.n, NRHS)


def _padded(V, cols=None):
    """V (n x NRHS) as NRHS + SPARE vectors of stride n + PAD; cols: the position of V's row i in its vector"""
    n = V.shape[0]
    img = np.full((NRHS + SPARE, n + PAD), SENTINEL)
    img[:NRHS, np.arange(n) if cols is None else cols] = V.T
    return img


def _run(img, call):
    """call(device pointer) on a device copy of img; the image afterwards, its sentinels checked"""
    import torch
    n = img.shape[1] - PAD
    xd = torch.tensor(img.ravel(), device="cuda")
    torch.cuda.synchronize()
    call(xd.data_ptr())
    torch.cuda.synchronize()
    out = xd.cpu().numpy().reshape(img.shape)
    assert np.array_equal(out[:NRHS, n:], img[:NRHS, n:]) and np.array_equal(out[NRHS:], img[NRHS:])
    return out


def _both_orders(k, V, call):
    """call(pointer, pivot_order) on V in user order and in pivot order: the two results, n x NRHS, user order"""
    order = _case(k)[4]
    n = V.shape[0]
    user = _run(_padded(V), lambda p: call(p, False))[:NRHS, :n].T
    pivot = _run(_padded(V, order), lambda p: call(p, True))[:NRHS, order].T
    return user, pivot


def _check_bars(A, B, want, got):
    assert np.isfinite(got).all()
    errs = [bwd_err(A, got[:, q], B[:, q]) for q in range(NRHS)]
    print("max scaled backward error", max(errs), "max |x - solve|", float(np.abs(got - want).max()))
    assert max(errs) <= 1e-14, (int(np.argmax(errs)), max(errs))
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("k", KS)
def test_solve_many(k):
    A, f, val, B, order, want = _case(k)
    ldx = f.n + PAD
    user, pivot = _both_orders(k, B, lambda p, po: f.solve_many_dev(p, NRHS, ldx=ldx, pivot_order=po))
    print("user and pivot order agree bit for bit:", np.array_equal(user, pivot))
    _check_bars(A, B, want, user)
    _check_bars(A, B, want, pivot)


@pytest.mark.parametrize("k", KS)
def test_solve_reproducible(k):
    A, f, val, B, order, want = _case(k)
    ldx = f.n + PAD
    user, pivot = _both_orders(k, B, lambda p, po: f.solve_reproducible_dev(p, NRHS, ldx=ldx, pivot_order=po))
    assert np.array_equal(user, pivot)
    assert np.array_equal(f.solve_reproducible(B), user)
    _check_bars(A, B, want, user)


@pytest.mark.parametrize("k", KS)
def test_matvec(k):
    import torch
    A, f, val, B, order, want = _case(k)
    n, ldx = f.n, f.n + PAD
    vd = torch.tensor(val, device="cuda")
    res = []
    for po in (False, True):
        cols = order if po else np.arange(n)
        ximg = _padded(B, cols)
        xd = torch.tensor(ximg.ravel(), device="cuda")
        yimg = _run(np.full_like(ximg, SENTINEL), lambda p: f.matvec_dev(vd.data_ptr(), val.size, xd.data_ptr(), p, NRHS,
                                                                         ldx=ldx, ldy=ldx, pivot_order=po))
        assert np.array_equal(xd.cpu().numpy().reshape(ximg.shape), ximg)      # x is only read
        res.append(yimg[:NRHS, cols].T)
    assert np.array_equal(res[0], res[1])
    assert np.array_equal(f.matvec(val, B), res[0])
    np.testing.assert_allclose(res[0], A @ B, rtol=1e-13, atol=1e-13)      # (the bar of tests/test_refine_gpu.py)


@pytest.mark.parametrize("k", KS)
def test_solve_batch(k):
    A, f, val, B, order, want = _case(k)
    ldx = f.n + PAD
    assert f.factor_batch(val[None, :]) == 0
    user, pivot = _both_orders(k, B, lambda p, po: f.solve_batch_dev(p, NRHS, ldx=ldx, pivot_order=po))
    print("user and pivot order agree bit for bit:", np.array_equal(user, pivot))
    _check_bars(A, B, want, user)
    _check_bars(A, B, want, pivot)


NV = 49      # per member: 32 + 17-in-a-block-of-32, or 16 + 16 + 16 + 1 in blocks of 16


def _image(V):
    """the vectors V (rows of n) at stride n + PAD with SPARE vectors behind them, sentinels everywhere else"""
    img = np.full((V.shape[0] + SPARE, V.shape[1] + PAD), SENTINEL)
    img[:V.shape[0], :V.shape[1]] = V
    return img


def _host_and_dev(V, host, dev):
    """host(pointer to the padded image of V on the host) and dev(integer pointer to a device copy of it): the
    vectors of the two images afterwards, their sentinels checked"""
    import ctypes
    import torch
    img = _image(V)
    nv, n = V.shape
    h = img.copy()
    host(ctypes.c_void_p(h.ctypes.data))
    xd = torch.tensor(img.ravel(), device="cuda")
    torch.cuda.synchronize()
    dev(xd.data_ptr())
    torch.cuda.synchronize()
    d = xd.cpu().numpy().reshape(img.shape)
    for out in (h, d):
        assert np.array_equal(out[:nv, n:], img[:nv, n:]) and np.array_equal(out[nv:], img[nv:])
    return h[:nv, :n].copy(), d[:nv, :n].copy()


def _solve_bars(A, B, want, got):
    """the bars of _check_bars for vectors in rows"""
    assert np.isfinite(got).all()
    errs = [bwd_err(A, got[q], B[q]) for q in range(B.shape[0])]
    print("max scaled backward error", max(errs), "max |x - solve|", float(np.abs(got - want).max()))
    assert max(errs) <= 1e-14, (int(np.argmax(errs)), max(errs))
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)


def test_block_walk():
    import ctypes as C
    A, f, val = _case(17)[:3]
    n, ldx, lib, fk = f.n, f.n + PAD, f.lib, f.fkeep
    assert n == 289
    dptr = lambda p: C.cast(p, C.POINTER(C.c_double))
    rng = np.random.default_rng(49)
    X = rng.standard_normal((NV, n))                    # one arena
    XB = rng.standard_normal((2 * NV, n))               # member b's vector q in row b * NV + q
    scale = np.repeat([1.0, 2.0], NV)[:, None]          # member 1 is 2 A
    want = f.solve(np.asfortranarray(X.T)).T
    wantB = f.solve(np.asfortranarray(XB.T)).T / scale
    assert f.factor_batch(np.stack([val, 2.0 * val])) == 0
    zeros, zerosB = np.zeros((NV, n)), np.zeros((2 * NV, n))
    seed = 20

    def solve_many():
        h, d = _host_and_dev(X, lambda p: f._call("spllt_hip_solve_many", fk, NV, dptr(p), ldx, 0),
                             lambda p: f.solve_many_dev(p, NV, ldx=ldx))
        for got in (h, d):
            _solve_bars(A, X, want, got)
        return h

    def factor_mult():
        h, d = _host_and_dev(X, lambda p: f._call("spllt_hip_factor_mult", fk, NV, dptr(p), ldx, 0),
                             lambda p: f.factor_mult_dev(p, NV, ldx=ldx))
        assert np.array_equal(h, d)
        return h

    def sample():
        h, d = _host_and_dev(zeros, lambda p: f._call("spllt_hip_sample", fk, NV, dptr(p), ldx, 1, seed, 0, None),
                             lambda p: f.sample_dev(p, NV, ldx=ldx, seed=seed, kind=1))
        assert np.array_equal(h, d)
        return h

    def factor_mult_batch():
        h, d = _host_and_dev(XB, lambda p: f._call("spllt_hip_factor_mult_batch", fk, NV, p, ldx, 0),
                             lambda p: f.factor_mult_batch_dev(p, NV, ldx=ldx))
        assert np.array_equal(h, d)
        return h

    def sample_batch():
        h, d = _host_and_dev(zerosB, lambda p: f._call("spllt_hip_sample_batch", fk, NV, p, ldx, 1, seed, 0, 0, 1, None, 0),
                             lambda p: f.sample_batch_dev(p, NV, ldx=ldx, seed=seed, kind=1))
        assert np.array_equal(h, d)
        return h

    def solve_many_batch(rb, blocks):
        h, d = _host_and_dev(XB, lambda p: f._call("spllt_hip_solve_many_batch", fk, NV, p, ldx, 0),
                             lambda p: f.solve_many_batch_dev(p, NV, ldx=ldx))
        info = f.solve_many_batch_info()
        assert info["rb"] == rb and info["blocks"] == blocks, info
        for got in (h, d):
            _solve_bars(A, XB[:NV], wantB[:NV], got[:NV])
            _solve_bars(2.0 * A, XB[NV:], wantB[NV:], got[NV:])
        return h

    def blocks_of_16(release, run):
        release()
        assert lib.spllt_hip_debug(b"fmult_alloc_fail=1") == 0
        try:
            return run()
        finally:
            assert lib.spllt_hip_debug(b"fmult_alloc_fail=0") == 0

    solve_many()
    # the product against A X (the bar of tests/test_factor_mult_gpu.py); the samples by themselves: sample q is
    # a function of (seed, q) alone, wherever it lies in a block
    y, s = factor_mult(), sample()
    np.testing.assert_allclose(y, (A @ X.T).T, rtol=1e-12, atol=1e-12 * np.abs(A @ X.T).max())
    for q in (0, 31, 32, 48):
        assert np.array_equal(f.sample(1, seed=seed, kind=1, first_sample=q)[:, 0], s[q]), q
    yb, sb = factor_mult_batch(), sample_batch()
    np.testing.assert_allclose(yb, scale * (A @ XB.T).T, rtol=1e-12, atol=1e-12 * 2.0 * np.abs(A @ XB.T).max())
    solve_many_batch(32, 2)
    # blocks of 16 (what is left when the storage of 32 does not fit): per vector the same sums in the same order
    y16, s16 = blocks_of_16(f.release_factor_mult, lambda: (factor_mult(), sample()))
    assert np.array_equal(y16, y) and np.array_equal(s16, s)
    yb16, sb16 = blocks_of_16(f.release_factor_mult_batch, lambda: (factor_mult_batch(), sample_batch()))
    assert np.array_equal(yb16, yb) and np.array_equal(sb16, sb)
    blocks_of_16(f.release_solve_many_batch, lambda: solve_many_batch(16, 4))
    for release in (f.release_factor_mult, f.release_factor_mult_batch, f.release_solve_many_batch):
        release()     # (the next user takes blocks of 32 again)
