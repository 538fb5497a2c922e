"""GPU tests of what the vector entry points share: the device order table and the permutation kernel (one
workgroup of 256 per 256 variables and vector), on padded vectors.  n = 4, 256 and 289: less than a workgroup,
exactly one, one and a partial one.  Five right-hand sides: a sweep of 4 + 1 for the reproducible solve, one
zero-padded block of 16 for the blocked solve.  Every vector lies at x[q * ldx ..] with ldx = n + 7, two spare
vectors behind the used ones, every slot outside the vectors holds a sentinel that must come back untouched.

The reproducible solve and the product have no atomic add: user order, pivot order and the host entry point
must give the same bits (the product is also held to A @ B at the bar of the refine tests).  The blocked
solve and the batch solve add with atomics, so two runs may differ in the last bits: they are held to the
existing bars of their own tests instead (scaled backward error 1e-14 per vector; rtol = atol = 1e-12 against
spllt_solve), in both orders."""
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
