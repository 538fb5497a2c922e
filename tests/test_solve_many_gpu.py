"""GPU tests of the blocked many-right-hand-side solve (spllt_hip_solve_many / spllt_hip_solve_many_dev,
solve_many.hip): the substitution program of spllt_solve on blocks of 32 right-hand sides with the
products on the fp64 matrix cores.  Bars: the reference harness's scaled backward error (1e-14 per
vector, tests/test_gpu_parity.py) and the tolerances the existing solve test uses against the CPU
oracle and between two solves."""
import functools
import time

import numpy as np
import pytest

from helpers import bwd_err, make_case, oracle_factor
from spllt_amd import api, matgen

pytestmark = pytest.mark.gpu

# the four (generator, nb) pairs of test_device_solve_jobs_and_multiple_rhs, one case with block columns
# between 256 and 512 wide, and one at nb = 1024; min_width: a block column wider than this must occur
CASES = [
    ("p2d40-nb16", lambda: matgen.poisson2d(40), 16, 0),
    ("box11-nb64", lambda: matgen.nd_like((11, 10, 9), 2), 64, 0),
    ("p3d14-nb384", lambda: matgen.poisson3d(14), 384, 0),
    ("fe27-nb768", lambda: matgen.fe27((7, 6, 6), 3), 768, 256),
    ("box12-nb512", lambda: matgen.nd_like((10, 12, 12), 3), 512, 256),
    ("box17-nb1024", lambda: matgen.nd_like((12, 17, 16), 3), 1024, 768),
]
NRHS = [1, 5, 16, 17, 32, 33, 100, 128, 300]


@functools.lru_cache(maxsize=None)
def _case(name):
    _, gen, nb, min_width = next(c for c in CASES if c[0] == name)
    A = gen()
    f, val = make_case(A, nb=nb, nemin=16)
    assert int(f.sym("bcol_width").max()) > min_width, "the case degenerated: no wide block column"
    f.factor(val).wait()
    o, rc = oracle_factor(f, val)
    assert rc == 0
    return A, f, val, o


def _rhs(A, nrhs, seed=0):
    X = np.random.default_rng(seed).standard_normal((A.shape[0], nrhs))
    return A @ X


@pytest.mark.parametrize("nrhs", NRHS)
@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_every_vector_meets_the_backward_error_bar(name, nrhs):
    A, f, val, o = _case(name)
    B = _rhs(A, nrhs)
    got = f.solve_many(B if nrhs > 1 else B[:, 0]).reshape(f.n, nrhs)
    assert np.isfinite(got).all()
    errs = [bwd_err(A, got[:, r], B[:, r]) for r in range(nrhs)]
    print(name, nrhs, "max scaled backward error", max(errs))
    assert max(errs) <= 1e-14, (int(np.argmax(errs)), max(errs))
    # against independent solves: the CPU oracle's, and the existing four-per-sweep device solve
    for r in range(nrhs):
        np.testing.assert_allclose(got[:, r], o.solve(B[:, r]), rtol=1e-10, atol=1e-11)
    np.testing.assert_allclose(got, f.solve(B).reshape(f.n, nrhs), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_forward_then_backward_equals_both(name):
    A, f, val, o = _case(name)
    B = _rhs(A, 33, seed=1)
    both = f.solve_many(B)
    y = f.solve_many(B, job=1)
    assert not np.allclose(y, both)
    np.testing.assert_allclose(f.solve_many(y, job=2), both, rtol=1e-12, atol=1e-12)
    # the sweeps are the existing solve's sweeps
    np.testing.assert_allclose(y, f.solve(B, job=1), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("nrhs", [5, 33])
@pytest.mark.parametrize("name", ["box11-nb64", "box17-nb1024"])
def test_layout_padding_and_entry_points(name, nrhs):
    """ldx = n + 7 with a sentinel in the padding and in two extra allocated columns: nothing outside
    [q ldx, q ldx + n) changes; host and device entry points agree; pivot order = user order permuted"""
    import torch
    A, f, val, o = _case(name)
    n, ldx, sentinel = f.n, f.n + 7, -7.25e77
    B = _rhs(A, nrhs, seed=2)
    want = f.solve_many(B)
    # host entry point, through the C interface on a padded array
    xh = np.full((nrhs + 2) * ldx, sentinel)
    for q in range(nrhs):
        xh[q * ldx:q * ldx + n] = B[:, q]
    before = xh.copy()
    rc = f.lib.spllt_hip_solve_many(f.fkeep, nrhs, api._dp(xh), ldx, 0)
    assert rc == 0, f.last_error()
    img = xh.reshape(nrhs + 2, ldx)
    assert np.array_equal(img[:nrhs, n:], before.reshape(nrhs + 2, ldx)[:nrhs, n:])
    assert np.array_equal(img[nrhs:], before.reshape(nrhs + 2, ldx)[nrhs:])
    np.testing.assert_allclose(img[:nrhs, :n].T, want, rtol=1e-12, atol=1e-12)
    # device entry point, user order
    xd = torch.tensor(before, device="cuda")
    torch.cuda.synchronize()
    f.solve_many_dev(xd.data_ptr(), nrhs, ldx=ldx)
    dimg = xd.cpu().numpy().reshape(nrhs + 2, ldx)
    assert np.array_equal(dimg[:nrhs, n:], before.reshape(nrhs + 2, ldx)[:nrhs, n:])
    assert np.array_equal(dimg[nrhs:], before.reshape(nrhs + 2, ldx)[nrhs:])
    np.testing.assert_allclose(dimg[:nrhs, :n].T, want, rtol=1e-12, atol=1e-12)
    # device entry point, pivot order (the layout of solve_dev), ldx = n by default
    order = f.sym("order")
    Bp = np.empty((nrhs, n))
    Bp[:, order] = B.T
    yd = torch.tensor(Bp.ravel(), device="cuda")
    torch.cuda.synchronize()
    f.solve_many_dev(yd.data_ptr(), nrhs, pivot_order=True)
    got = yd.cpu().numpy().reshape(nrhs, n)[:, order].T
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)
    # and the existing device solve on the same pivot-ordered vectors
    zd = torch.tensor(Bp.ravel(), device="cuda")
    torch.cuda.synchronize()
    f.solve_dev(zd.data_ptr(), nrhs)
    np.testing.assert_allclose(zd.cpu().numpy().reshape(nrhs, n)[:, order].T, want, rtol=1e-12, atol=1e-12)


def test_zero_right_hand_sides_is_a_noop():
    A, f, val, o = _case("box11-nb64")
    x = np.full(f.n, 3.0)
    assert f.lib.spllt_hip_solve_many(f.fkeep, 0, api._dp(x), f.n, 0) == 0
    assert (x == 3.0).all()
    assert f.solve_many(np.zeros((f.n, 0))).shape == (f.n, 0)


def test_refactorization_is_picked_up():
    A = matgen.nd_like((10, 10, 9), 2)
    f, val = make_case(A, nb=96, nemin=16)
    f.factor(val).wait()
    B = _rhs(A, 40, seed=3)
    x1 = f.solve_many(B)
    f.factor(4.0 * val).wait()
    x2 = f.solve_many(B)
    np.testing.assert_allclose(x2, x1 / 4.0, rtol=1e-12, atol=1e-12)
    assert max(bwd_err(4.0 * A, x2[:, r], B[:, r]) for r in range(40)) <= 1e-14
    f.close()


@pytest.mark.parametrize("when", ["before", "after"])
def test_selected_inverse_does_not_disturb_it(when):
    A = matgen.nd_like((10, 10, 9), 2)
    f, val = make_case(A, nb=96, nemin=16)
    f.factor(val).wait()
    B = _rhs(A, 33, seed=4)
    if when == "before":
        f.selected_inverse()
        x = f.solve_many(B)
    else:
        x0 = f.solve_many(B)
        f.selected_inverse()
        x = f.solve_many(B)
        np.testing.assert_allclose(x, x0, rtol=1e-12, atol=1e-12)
    assert max(bwd_err(A, x[:, r], B[:, r]) for r in range(33)) <= 1e-14
    Ainv = np.linalg.inv(A.toarray())
    assert np.abs(f.inverse_diag() - np.diag(Ainv)).max() <= 1e-11 * np.abs(np.diag(Ainv)).max()
    f.close()


@pytest.mark.parametrize("variant", ["deterministic", "single_stream", "graph"])
def test_same_solution_under_engine_variants(variant, monkeypatch):
    A = matgen.nd_like((12, 12, 11), 3)
    nb, nemin = 256, 16
    B = _rhs(A, 33, seed=5)
    base, val = make_case(A, nb=nb, nemin=nemin)
    x0 = base.factor(val).wait().solve_many(B)
    base.close()
    flags = {"deterministic": 4096, "single_stream": 2}.get(variant, 0)
    if variant == "graph":
        monkeypatch.setenv("SPLLT_HIP_GRAPH", "2")
    f, val = make_case(A, nb=nb, nemin=nemin, engine_flags=flags)
    x = f.factor(val).wait().solve_many(B)
    np.testing.assert_allclose(x, x0, rtol=1e-12, atol=1e-12)
    assert max(bwd_err(A, x[:, r], B[:, r]) for r in range(33)) <= 1e-14
    f.close()


def test_errors():
    import torch
    A = matgen.poisson2d(32)
    f, val = make_case(A, nb=16, nemin=8)
    b = np.ones((f.n, 3))
    with pytest.raises(api.SplltError) as ei:          # before the first factorization
        f.solve_many(b)
    assert ei.value.flag == -10 and "factorized" in f.last_error()
    xd = torch.ones(3 * f.n, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(api.SplltError) as ei:
        f.solve_many_dev(xd.data_ptr(), 3)
    assert ei.value.flag == -10
    f.factor(val).wait()
    with pytest.raises(api.SplltError) as ei:          # ldx < n
        f.solve_many_dev(xd.data_ptr(), 3, ldx=f.n - 1)
    assert ei.value.flag == -10 and "ldx" in f.last_error()
    assert f.lib.spllt_hip_solve_many(f.fkeep, 3, api._dp(b.ravel()), f.n - 1, 0) == -10
    assert f.lib.spllt_hip_solve_many(f.fkeep, -1, api._dp(b.ravel()), f.n, 0) == -10
    assert f.lib.spllt_hip_solve_many(f.fkeep, 3, api._dp(b.ravel()), f.n, 3) == -10
    assert f.lib.spllt_hip_solve_many(f.fkeep, 3, None, f.n, 0) == -10
    assert f.lib.spllt_hip_solve_many_dev(f.fkeep, 3, None, f.n, 0, 0) == -10
    assert (xd.cpu().numpy() == 1.0).all()
    x = f.solve_many(A @ b)                              # the handle is still good
    np.testing.assert_allclose(x, b, rtol=0, atol=1e-10)
    f.close()


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
            f.solve_many(np.ones((f.n, 2)))
        assert ei.value.flag == -98 and "partitioned" in f.last_error()
        with pytest.raises(api.SplltError) as ei:
            f.solve_many_dev(xd.data_ptr(), 2)
        assert ei.value.flag == -98
    for f in fs:
        f.close()


def test_it_is_the_blocked_path():
    """128 resident vectors: the blocked path (4 sweeps of 32) is not slower than the existing device
    solve (32 sweeps of 4) -- a loose guard against an implementation that loops over the old kernels;
    the measured ratios are in DESIGN.md section 10.  Median of 5 after 2 warm-ups each, alternating."""
    import torch
    A = matgen.nd_like((24, 24, 23), 2)
    f, val = make_case(A, nb=128, nemin=32)
    f.factor(val).wait()
    n, nrhs = f.n, 128
    order = f.sym("order")
    B = _rhs(A, nrhs, seed=6)
    Bp = np.empty((nrhs, n))
    Bp[:, order] = B.T
    src = torch.tensor(Bp.ravel(), device="cuda")
    work = torch.empty_like(src)
    t_old, t_new = [], []
    for it in range(7):
        for which in ("old", "new"):
            work.copy_(src)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if which == "old":
                f.solve_dev(work.data_ptr(), nrhs)
            else:
                f.solve_many_dev(work.data_ptr(), nrhs, pivot_order=True)
            dt = time.perf_counter() - t0
            if it >= 2:
                (t_old if which == "old" else t_new).append(dt)
            if it == 0:
                got = work.cpu().numpy().reshape(nrhs, n)[:, order].T
                assert max(bwd_err(A, got[:, r], B[:, r]) for r in range(nrhs)) <= 1e-14
    old, new = float(np.median(t_old)), float(np.median(t_new))
    print("solve_dev %.3f ms, solve_many_dev %.3f ms, ratio %.2f, one old sweep %.3f ms"
          % (old * 1e3, new * 1e3, old / new, old * 1e3 / 32))
    assert new <= old, (old, new)
    f.close()
