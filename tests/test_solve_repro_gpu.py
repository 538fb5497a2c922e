"""GPU tests of the reproducible solve (spllt_hip_solve_repro*, solve_repro.hip): the substitution program of
spllt_solve without atomic adds.  Accuracy bars: the project's existing ones (scaled backward error 1e-14 per
vector, the tolerances of the solve tests against the CPU oracle and between two device solves).  Determinism
is judged by results only: np.array_equal."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from helpers import bwd_err, make_case, oracle_factor
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


@functools.lru_cache(maxsize=None)
def _case(name):
    _, gen, nb, nemin = next(c for c in CASES if c[0] == name)
    A = gen()
    f, val = make_case(A, nb=nb, nemin=nemin)
    f.factor(val).wait()
    o, rc = oracle_factor(f, val)
    assert rc == 0
    B = A @ np.random.default_rng(0).standard_normal((A.shape[0], 9))
    return A, f, val, o, B


@pytest.mark.parametrize("nrhs", [1, 2, 3, 4, 5, 9])
@pytest.mark.parametrize("name", NAMES)
def test_accuracy(name, nrhs):
    A, f, val, o, B9 = _case(name)
    B = B9[:, :nrhs]
    got = f.solve_reproducible(B if nrhs > 1 else B[:, 0]).reshape(f.n, nrhs)
    assert np.isfinite(got).all()
    errs = [bwd_err(A, got[:, r], B[:, r]) for r in range(nrhs)]
    print(name, nrhs, "max scaled backward error", max(errs))
    assert max(errs) <= 1e-14, (int(np.argmax(errs)), max(errs))
    for r in range(nrhs):
        np.testing.assert_allclose(got[:, r], o.solve(B[:, r]), rtol=1e-10, atol=1e-11)
    np.testing.assert_allclose(got, f.solve(B).reshape(f.n, nrhs), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("name", NAMES)
def test_bit_identity(name):
    A, f, val, o, B = _case(name)
    x = f.solve_reproducible(B)
    for _ in range(2):
        assert np.array_equal(f.solve_reproducible(B), x)
    y = f.solve_reproducible(B, job=1)
    assert not np.allclose(y, x)
    assert np.array_equal(f.solve_reproducible(y, job=2), x)
    assert f.lib.spllt_hip_debug(b"rsolve_poison=1") == 0
    try:
        xp = f.solve_reproducible(B)
    finally:
        assert f.lib.spllt_hip_debug(b"rsolve_poison=0") == 0
    assert np.array_equal(xp, x)


@pytest.mark.parametrize("name", NAMES)
def test_group_independence(name):
    A, f, val, o, B = _case(name)
    x = f.solve_reproducible(B)
    for q in range(9):
        assert np.array_equal(f.solve_reproducible(B[:, q]), x[:, q]), q
    perm = np.random.default_rng(1).permutation(9)
    assert not np.array_equal(perm, np.arange(9))
    assert np.array_equal(f.solve_reproducible(B[:, perm]), x[:, perm])


@pytest.mark.parametrize("name", ["box11-nb64", "box12-nb512"])
def test_entry_points(name):
    import torch
    A, f, val, o, B9 = _case(name)
    nrhs = 5
    B = B9[:, :nrhs]
    n, ldx, sentinel = f.n, f.n + 7, -7.25e77
    want = f.solve_reproducible(B)
    xh = np.full((nrhs + 2) * ldx, sentinel)
    for q in range(nrhs):
        xh[q * ldx:q * ldx + n] = B[:, q]
    before = xh.copy().reshape(nrhs + 2, ldx)
    assert f.lib.spllt_hip_solve_repro(f.fkeep, nrhs, api._dp(xh), ldx, 0) == 0, f.last_error()
    img = xh.reshape(nrhs + 2, ldx)
    assert np.array_equal(img[:nrhs, n:], before[:nrhs, n:]) and np.array_equal(img[nrhs:], before[nrhs:])
    assert np.array_equal(img[:nrhs, :n].T, want)
    # device, user order, padded
    xd = torch.tensor(before.ravel(), device="cuda")
    torch.cuda.synchronize()
    f.solve_reproducible_dev(xd.data_ptr(), nrhs, ldx=ldx)
    dimg = xd.cpu().numpy().reshape(nrhs + 2, ldx)
    assert np.array_equal(dimg[:nrhs, n:], before[:nrhs, n:]) and np.array_equal(dimg[nrhs:], before[nrhs:])
    assert np.array_equal(dimg[:nrhs, :n].T, want)
    # device, pivot order, padded: in place with ldy = ldx
    order = f.sym("order")
    Bp = np.full((nrhs + 2, ldx), sentinel)
    Bp[:nrhs, order] = B.T
    yd = torch.tensor(Bp.ravel(), device="cuda")
    torch.cuda.synchronize()
    f.solve_reproducible_dev(yd.data_ptr(), nrhs, ldx=ldx, pivot_order=True)
    pimg = yd.cpu().numpy().reshape(nrhs + 2, ldx)
    assert np.array_equal(pimg[:nrhs, n:], Bp[:nrhs, n:]) and np.array_equal(pimg[nrhs:], Bp[nrhs:])
    assert np.array_equal(pimg[:nrhs, order].T, want)


def test_two_handles():
    A = matgen.nd_like((11, 10, 9), 2)
    B = A @ np.random.default_rng(2).standard_normal((A.shape[0], 5))
    xs, Ls = [], []
    for _ in range(2):
        f, val = make_case(A, nb=64, nemin=16, engine_flags=4096)
        f.factor(val).wait()
        Ls.append(f.get_factor())
        xs.append(f.solve_reproducible(B))
        f.close()
    assert np.array_equal(Ls[0], Ls[1])
    assert np.array_equal(xs[0], xs[1])
    assert max(bwd_err(A, xs[0][:, r], B[:, r]) for r in range(5)) <= 1e-14


@pytest.mark.parametrize("name", ["box11-nb64", "p3d14-nb384"])
def test_switch(name):
    import torch
    A, f, val, o, B9 = _case(name)
    n = f.n
    B = B9[:, :6]
    x_plain = f.solve(B)
    want = f.solve_reproducible(B)
    assert f.set_reproducible_solve(True) is False
    try:
        assert np.array_equal(f.solve(B), want)
        order = f.sym("order")
        Bp = np.empty((6, n))
        Bp[:, order] = B.T
        yd = torch.tensor(Bp.ravel(), device="cuda")
        torch.cuda.synchronize()
        f.solve_dev(yd.data_ptr(), 6)
        assert np.array_equal(yd.cpu().numpy().reshape(6, n)[:, order].T, want)
        for method in ("ir", "pcg"):
            runs = [f.solve_refined(1.001 * val, B, method=method, tol=1e-14, max_iter=20) for _ in range(2)]
            assert int(runs[0][1].max()) >= 1, "the refined solve did not iterate"
            assert np.array_equal(runs[0][0], runs[1][0]), method
            assert np.array_equal(runs[0][1], runs[1][1]), method
    finally:
        assert f.set_reproducible_solve(False) is True
    np.testing.assert_allclose(f.solve(B), x_plain, rtol=1e-12, atol=1e-12)


def test_state_refactorization_update_and_release():
    A = matgen.nd_like((10, 10, 9), 2)
    f, val = make_case(A, nb=96, nemin=16)
    n = f.n
    b3 = np.ones((n, 3))
    with pytest.raises(api.SplltError) as ei:          # before the first factorization
        f.solve_reproducible(b3)
    assert ei.value.flag == -10 and "factorized" in f.last_error()
    f.factor(val).wait()
    B = A @ np.random.default_rng(3).standard_normal((n, 5))
    x1 = f.solve_reproducible(B)
    f.factor(4.0 * val).wait()
    x2 = f.solve_reproducible(B)
    np.testing.assert_allclose(x2, x1 / 4.0, rtol=1e-12, atol=1e-12)
    # nrhs = 0
    x = np.full(n, 3.0)
    assert f.lib.spllt_hip_solve_repro(f.fkeep, 0, api._dp(x), n, 0) == 0
    assert (x == 3.0).all()
    assert f.solve_reproducible(np.zeros((n, 0))).shape == (n, 0)
    # one admissible update column on an existing entry: the solve sees A + w w^T
    f.factor(val).wait()
    w = sp.csc_matrix(([0.5, -0.5], ([0, 1], [0, 0])), shape=(n, 1))
    A1 = (A + w @ w.T).tocsc()
    f.update(w)
    B1 = A1 @ np.random.default_rng(4).standard_normal((n, 3))
    x3 = f.solve_reproducible(B1)
    assert max(bwd_err(A1, x3[:, r], B1[:, r]) for r in range(3)) <= 1e-14
    # release and use again
    f.release_solve_repro()
    assert np.array_equal(f.solve_reproducible(B1), x3)
    f.close()
