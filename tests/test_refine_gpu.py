"""GPU tests of the refined solves (spllt_hip_matvec, spllt_hip_solve_refined and their _dev twins,
refine.hip): the product on the analysed pattern, iterative refinement and factor-preconditioned CG to a
requested backward error.  Bars: the rounding bound of a sum of products for the operator, the reference
checker's scaled backward error for the solves, and the iteration counts of tests/refine_emulate.py driven by
the CPU oracle's solve."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import refine_emulate as em
from helpers import bwd_err, make_case, oracle_factor
from spllt_amd import api, matgen

pytestmark = pytest.mark.gpu

# the cases of tests/test_solve_many_gpu.py::CASES
CASES = [
    ("p2d40-nb16", lambda: matgen.poisson2d(40), 16),
    ("box11-nb64", lambda: matgen.nd_like((11, 10, 9), 2), 64),
    ("p3d14-nb384", lambda: matgen.poisson3d(14), 384),
    ("fe27-nb768", lambda: matgen.fe27((7, 6, 6), 3), 768),
    ("box12-nb512", lambda: matgen.nd_like((10, 12, 12), 3), 512),
    ("box17-nb1024", lambda: matgen.nd_like((12, 17, 16), 3), 1024),
]
NAMES = [c[0] for c in CASES]
U = 2.0 ** -53
TOL, MAX_ITER = 5e-15, 60
METHOD = {"ir": 0, "pcg": 1}


@functools.lru_cache(maxsize=None)
def _case(name):
    """the matrix A0, a handle with A0 factorized, its values, the CPU oracle's factor of A0"""
    _, gen, nb = next(c for c in CASES if c[0] == name)
    A0 = sp.csc_matrix(gen())
    f, val = make_case(A0, nb=nb, nemin=16)
    f.factor(val).wait()
    o, rc = oracle_factor(f, val)
    assert rc == 0
    return A0, f, val, o


@functools.lru_cache(maxsize=None)
def _system(name, eps, seed=0, ncol=40):
    """A = S A0 S, S = diag(1 + eps u), u uniform(0, 1) seeded: the pattern of A0, val'_k = s_i s_j val_k;
    B = A randn (ncol columns; a test takes the first nrhs)"""
    A0, f, val0, o = _case(name)
    rng = np.random.default_rng(seed)
    n = A0.shape[0]
    s = 1.0 + eps * rng.random(n)
    A = sp.csc_matrix(sp.diags(s) @ A0 @ sp.diags(s))
    n1, ptr, row, val = api.csc_lower_1based(A)
    n0, ptr0, row0, _ = api.csc_lower_1based(A0)
    assert np.array_equal(ptr, ptr0) and np.array_equal(row, row0)
    B = np.asfortranarray(A @ rng.standard_normal((n, ncol)))
    return A, val, B


@functools.lru_cache(maxsize=None)
def _emulated(name, eps, method, q):
    """iterations and convergence of the emulator for column q, with the CPU oracle's solve as M^-1"""
    A0, f, val0, o = _case(name)
    A, val, B = _system(name, eps)
    x, it, err, ok = em.refine(A, B[:, q], lambda v: o.solve(v), METHOD[method], TOL, MAX_ITER)
    return it, err, ok


def exact_product(M, X):
    """M @ X with every row summed in extended precision, |M| |X|, and the entries per row"""
    M = sp.csr_matrix(M)
    X = X.reshape(M.shape[0], -1)
    prod = M.data.astype(np.longdouble)[:, None] * X.astype(np.longdouble)[M.indices]
    nz = np.flatnonzero(np.diff(M.indptr) > 0)
    y = np.zeros((M.shape[0], X.shape[1]), dtype=np.longdouble)
    ya = np.zeros_like(y)
    y[nz] = np.add.reduceat(prod, M.indptr[:-1][nz], axis=0)
    ya[nz] = np.add.reduceat(abs(prod), M.indptr[:-1][nz], axis=0)
    return y, ya, np.diff(M.indptr)


# ---- the operator -------------------------------------------------------------------------------
@pytest.mark.parametrize("nvec", [1, 3, 32, 33, 100])
@pytest.mark.parametrize("name", NAMES)
def test_matvec_accuracy_repetition_and_layout(name, nvec):
    """|y - A x|_i <= 2 (entries in row i) 2^-53 (|A||x|)_i; bit-identical on repetition; padded ldx / ldy with
    sentinels: nothing outside [q ldy, q ldy + n) is written; host and device entry points, user and pivot order"""
    import torch
    A0, f, val0, o = _case(name)
    A, val, _ = _system(name, 0.3)
    n, nnz = f.n, len(val)
    rng = np.random.default_rng(11)
    X = rng.standard_normal((n, nvec))
    want, wabs, nrow = exact_product(A, X)
    bound = 2.0 * nrow[:, None] * U * wabs
    y1 = f.matvec(val, X if nvec > 1 else X[:, 0]).reshape(n, nvec)
    y2 = f.matvec(val, X if nvec > 1 else X[:, 0]).reshape(n, nvec)
    print(name, nvec, "max |y - Ax| / bound", float((abs(y1 - want) / np.maximum(bound, 1e-300)).max()))
    assert (abs(y1 - want) <= bound).all()
    assert np.array_equal(y1, y2)
    # padded arrays with sentinels, host entry point
    ldx, ldy, sentinel = n + 5, n + 7, -7.25e77
    xh = np.full((nvec + 2) * ldx, sentinel)
    for q in range(nvec):
        xh[q * ldx:q * ldx + n] = X[:, q]
    yh = np.full((nvec + 2) * ldy, sentinel)
    x_before = xh.copy()
    assert f.lib.spllt_hip_matvec(f.fkeep, nnz, api._dp(val), nvec, api._dp(xh), ldx, api._dp(yh), ldy) == 0, f.last_error()
    img = yh.reshape(nvec + 2, ldy)
    assert (img[:nvec, n:] == sentinel).all() and (img[nvec:] == sentinel).all() and np.array_equal(xh, x_before)
    assert np.array_equal(img[:nvec, :n].T, y1)
    # device entry point, user order
    dval = torch.tensor(val, device="cuda")
    xd = torch.tensor(x_before, device="cuda")
    yd = torch.full(((nvec + 2) * ldy,), sentinel, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    f.matvec_dev(dval.data_ptr(), nnz, xd.data_ptr(), yd.data_ptr(), nvec, ldx=ldx, ldy=ldy)
    dimg = yd.cpu().numpy().reshape(nvec + 2, ldy)
    assert (dimg[:nvec, n:] == sentinel).all() and (dimg[nvec:] == sentinel).all()
    assert np.array_equal(xd.cpu().numpy(), x_before)
    assert np.array_equal(dimg[:nvec, :n].T, y1)
    # device entry point, pivot order: the same sums on permuted vectors
    order = f.sym("order")
    Xp = np.full((nvec, ldx), sentinel)
    Xp[:, order] = X.T
    xp = torch.tensor(Xp.ravel(), device="cuda")
    yp = torch.full((nvec * ldy,), sentinel, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    f.matvec_dev(dval.data_ptr(), nnz, xp.data_ptr(), yp.data_ptr(), nvec, ldx=ldx, ldy=ldy, pivot_order=True)
    pimg = yp.cpu().numpy().reshape(nvec, ldy)
    assert (pimg[:, n:] == sentinel).all()
    assert np.array_equal(pimg[:, :n][:, order].T, y1)


def test_matvec_needs_no_factor_and_zero_vectors_is_a_noop():
    A = sp.csc_matrix(matgen.nd_like((9, 8, 7), 2))
    f, val = make_case(A, nb=64, nemin=16)
    x = np.random.default_rng(0).standard_normal(f.n)
    y = f.matvec(val, x)
    np.testing.assert_allclose(y, A @ x, rtol=1e-13, atol=1e-13)
    z = np.full(f.n, 3.0)
    assert f.lib.spllt_hip_matvec(f.fkeep, len(val), api._dp(val), 0, api._dp(x), f.n, api._dp(z), f.n) == 0
    assert (z == 3.0).all()
    # the refined solve still asks for a factor
    with pytest.raises(api.SplltError) as ei:
        f.solve_refined(val, A @ x)
    assert ei.value.flag == -10 and "factorized" in f.last_error()
    f.factor(val).wait()
    xs, it, err = f.solve_refined(val, A @ x)
    assert f.refine_status == 0 and it[0] == 0 and bwd_err(A, xs, A @ x) <= 1e-14
    f.close()


# ---- the solves ---------------------------------------------------------------------------------
@pytest.mark.parametrize("nrhs", [1, 4, 5, 33])
@pytest.mark.parametrize("method", ["ir", "pcg"])
@pytest.mark.parametrize("name", NAMES)
def test_same_matrix_takes_no_iteration(name, method, nrhs):
    A0, f, val0, o = _case(name)
    _, _, B = _system(name, 0.0)
    B = B[:, :nrhs]
    x, it, err = f.solve_refined(val0, B if nrhs > 1 else B[:, 0], method=method, tol=TOL, max_iter=MAX_ITER)
    x = x.reshape(f.n, nrhs)
    print(name, method, nrhs, "errors", err.max())
    assert f.refine_status == 0
    assert (it == 0).all()
    assert (err <= 5e-15).all()
    np.testing.assert_allclose(x, f.solve_many(B).reshape(f.n, nrhs), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("nrhs", [1, 7, 40])
@pytest.mark.parametrize("eps,method", [(0.02, "ir"), (0.02, "pcg"), (0.3, "pcg")])
@pytest.mark.parametrize("name", NAMES)
def test_perturbed_matrix_converges_with_the_stale_factor(name, eps, method, nrhs):
    """return 0; reported error <= 5e-15 per vector; host-recomputed bwd_err <= 1e-14 (the project's bar: the
    factor 2 covers the rounding of a residual evaluated twice); iterations within +-2 of the emulator's count
    for the same vector (near the threshold one rounding difference moves the crossing by an iteration)"""
    A0, f, val0, o = _case(name)
    A, val, B = _system(name, eps)
    B = B[:, :nrhs]
    x, it, err = f.solve_refined(val, B if nrhs > 1 else B[:, 0], method=method, tol=TOL, max_iter=MAX_ITER)
    x = x.reshape(f.n, nrhs)
    host = np.array([bwd_err(A, x[:, q], B[:, q]) for q in range(nrhs)])
    emu = np.array([_emulated(name, eps, method, q)[0] for q in range(nrhs)])
    print(name, eps, method, nrhs, "status", f.refine_status, "iterations", it.min(), it.max(), "emulator", emu.min(),
          emu.max(), "max |it - emu|", abs(it - emu).max(), "reported", err.max(), "host", host.max())
    assert all(_emulated(name, eps, method, q)[2] for q in range(nrhs))
    assert f.refine_status == 0, f.last_error()
    assert (err <= 5e-15).all()
    assert (host <= 1e-14).all()
    assert (abs(it - emu) <= 2).all(), (it, emu)


@pytest.mark.parametrize("name", NAMES)
def test_divergent_refinement_returns_the_best_iterate(name):
    """eps = 0.3, refinement, max_iter 20: return 1, every vector's error <= that of M^-1 b alone; a PCG call
    afterwards on the same handle converges"""
    A0, f, val0, o = _case(name)
    A, val, B = _system(name, 0.3)
    B = B[:, :7]
    x0 = f.solve_many(B)
    e0 = np.array([bwd_err(A, x0[:, q], B[:, q]) for q in range(7)])
    x, it, err = f.solve_refined(val, B, method="ir", tol=TOL, max_iter=20)
    host = np.array([bwd_err(A, x[:, q], B[:, q]) for q in range(7)])
    print(name, "M^-1 b", e0, "reported", err, "host", host, "iterations", it)
    assert f.refine_status == 1
    assert (it == 20).all() and (err > TOL).all()
    # the error of M^-1 b, as the device evaluated it, bounds what comes back; the host's evaluations of
    # both agree with the device's to rounding
    assert (err <= e0 * (1 + 1e-10)).all()
    assert (host <= e0 * (1 + 1e-10)).all()
    assert (abs(err - host) <= 1e-10 * host).all()      # the x handed back is the iterate whose error is reported
    x, it, err = f.solve_refined(val, B, method="pcg", tol=TOL, max_iter=MAX_ITER)
    assert f.refine_status == 0 and (err <= 5e-15).all()
    assert max(bwd_err(A, x[:, q], B[:, q]) for q in range(7)) <= 1e-14


def residual_rounding(A, x, b):
    """how far two evaluations of the backward error of the same x may lie apart: each residual entry is a sum
    of (entries in the row) + 1 terms, so |fl(b - A x) - (b - A x)| <= (len + 1) 2^-53 (|b| + |A||x|) per entry,
    once for the device's evaluation and once for the host's"""
    A = sp.csr_matrix(A)
    nrow = np.diff(A.indptr)
    slack = (nrow + 1) * U * (abs(b) + abs(A) @ abs(x))
    return 2.0 * float(np.linalg.norm(slack) / (np.linalg.norm(b) + abs(A).max() * np.linalg.norm(x)))


@pytest.mark.parametrize("method,eps", [("ir", 0.02), ("pcg", 0.3)])
@pytest.mark.parametrize("name", ["box11-nb64", "box12-nb512"])
def test_mixed_group(name, method, eps):
    """One A = S A0 S whose S differs from 1 on a tenth of the variables only, and right-hand sides of different
    difficulty: b = A x with x supported where A and A0 agree (M^-1 b is the solution: 0 iterations), with x
    random (hard), with x = easy + 1e-9 hard and easy + 1e-5 hard (in between), scaled copies and a zero
    vector.  The vectors stop at different iterations -- checked -- so the early ones sit frozen while the others
    iterate.  Per vector: the reported error is that of the x handed back (host-recomputed, to the rounding of
    two residual evaluations); the iteration count is within +-2 of the emulator's; and the vector solved ALONE
    agrees with the group's to rounding (rtol 1e-12, the tolerance between two solves) with a count within +-2.
    Bit-identity with the lone solve is asserted for the zero vector only: a lone vector goes through the
    four-vector substitution, the group through the blocked one, and both add with fp64 atomics."""
    A0, f, val0, o = _case(name)
    n = f.n
    rng = np.random.default_rng(3)
    s = np.ones(n)
    region = np.arange(n) < n // 10
    s[region] = 1.0 + eps * rng.random(int(region.sum()))
    A = sp.csc_matrix(sp.diags(s) @ A0 @ sp.diags(s))
    val = api.csc_lower_1based(A)[3]
    assert len(val) == len(val0)
    far = np.asarray(abs(A - A0).sum(axis=0)).ravel() == 0.0      # columns in which A and A0 agree
    assert far.sum() > n // 4
    xh = rng.standard_normal((n, 3))
    xe = np.where(far, rng.standard_normal(n), 0.0)
    X = np.column_stack([xh[:, 0], xe, np.zeros(n), xe + 1e-9 * xh[:, 1], 2.0 ** 70 * xh[:, 1], 2.0 ** -60 * xe,
                         xe + 1e-5 * xh[:, 2], xh[:, 2], 0.5 * xe + 1e-9 * xh[:, 0]])
    HARD, EASY, ZERO, MID9, MID5 = 0, 1, 2, 3, 6
    B = np.asfortranarray(A @ X)
    nrhs = B.shape[1]
    x, it, err = f.solve_refined(val, B, method=method, tol=TOL, max_iter=MAX_ITER)
    emu = [em.refine(A, B[:, q], lambda v: o.solve(v), METHOD[method], TOL, MAX_ITER) for q in range(nrhs)]
    emu_it = np.array([e[1] for e in emu])
    host = np.array([bwd_err(A, x[:, q], B[:, q]) if q != ZERO else 0.0 for q in range(nrhs)])
    print(name, method, "iterations", it, "emulator", emu_it, "reported", err, "host", host)
    assert f.refine_status == 0 and np.isfinite(x).all() and np.isfinite(err).all()
    assert all(e[3] for e in emu)
    assert (x[:, ZERO] == 0.0).all() and it[ZERO] == 0 and err[ZERO] == 0.0
    assert (err <= 5e-15).all() and (host <= 1e-14).all()
    # the vectors really stop at different iterations
    assert it[EASY] == 0 and it[5] == 0
    assert 0 < it[MID9] < it[HARD] and it[MID9] <= it[MID5] <= it[HARD]
    assert (abs(it - emu_it) <= 2).all(), (it, emu_it)
    # the x handed back is the iterate whose error was recorded
    for q in range(nrhs):
        if q != ZERO:
            assert abs(err[q] - host[q]) <= residual_rounding(A, x[:, q], B[:, q]), (q, err[q], host[q])
    # alone: the same solution to rounding, the same count within 2
    for q in (HARD, EASY, MID9, MID5):
        xa, ita, erra = f.solve_refined(val, B[:, q], method=method, tol=TOL, max_iter=MAX_ITER)
        print(name, method, "column", q, "alone", ita[0], "in the group", it[q], "bitwise equal",
              xa.tobytes() == x[:, q].tobytes(), "max diff", float(abs(xa - x[:, q]).max()))
        assert f.refine_status == 0 and abs(int(ita[0]) - int(it[q])) <= 2
        np.testing.assert_allclose(xa, x[:, q], rtol=1e-12, atol=1e-12)
    xa, ita, erra = f.solve_refined(val, B[:, ZERO], method=method, tol=TOL, max_iter=MAX_ITER)
    assert np.array_equal(xa, x[:, ZERO]) and ita[0] == 0 and erra[0] == 0.0
    # stopped early by max_iter: the hard vectors come back with the error of the iterate that is returned, the
    # easy ones are the same as before
    cap = max(1, int(it[MID9]))
    xc, itc, errc = f.solve_refined(val, B, method=method, tol=TOL, max_iter=cap)
    assert f.refine_status == 1 and itc[EASY] == 0 and itc[HARD] == cap and errc[HARD] > TOL and errc[EASY] <= TOL
    for q in (HARD, 7):
        hq = bwd_err(A, xc[:, q], B[:, q])
        assert abs(errc[q] - hq) <= residual_rounding(A, xc[:, q], B[:, q]) + 1e-10 * hq, (q, errc[q], hq)
    np.testing.assert_allclose(xc[:, EASY], x[:, EASY], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("method", ["ir", "pcg"])
def test_nan_right_hand_side_among_good_ones(method):
    A0, f, val0, o = _case("box11-nb64")
    A, val, B = _system("box11-nb64", 0.02)
    B = B[:, :6].copy()
    B[17, 3] = np.nan
    x, it, err = f.solve_refined(val, B, method=method, tol=TOL, max_iter=MAX_ITER)
    good = [0, 1, 2, 4, 5]
    print(method, "iterations", it, "errors", err)
    assert f.refine_status == 1
    assert not err[3] <= TOL and it[3] == 0          # ended at once, reported not converged
    assert (err[good] <= 5e-15).all() and np.isfinite(x[:, good]).all()
    assert max(bwd_err(A, x[:, q], B[:, q]) for q in good) <= 1e-14
    # a NaN among the values ends every vector at once instead of spinning to max_iter
    bad = val.copy()
    bad[len(bad) // 2] = np.nan
    x, it, err = f.solve_refined(bad, B[:, good], method=method, tol=TOL, max_iter=MAX_ITER)
    assert f.refine_status == 1 and (it == 0).all() and not (err <= TOL).any()


def test_device_entry_point_and_padding():
    import torch
    name = "box12-nb512"
    A0, f, val0, o = _case(name)
    A, val, B = _system(name, 0.02)
    nrhs, n = 35, f.n
    B = B[:, :nrhs]
    ldx, sentinel = n + 3, -7.25e77
    xh = np.full((nrhs + 1) * ldx, sentinel)
    for q in range(nrhs):
        xh[q * ldx:q * ldx + n] = B[:, q]
    dval = torch.tensor(val, device="cuda")
    xd = torch.tensor(xh, device="cuda")
    torch.cuda.synchronize()
    rc, it, err = f.solve_refined_dev(dval.data_ptr(), len(val), xd.data_ptr(), nrhs, ldx=ldx, method="pcg", tol=TOL,
                                      max_iter=MAX_ITER)
    img = xd.cpu().numpy().reshape(nrhs + 1, ldx)
    assert rc == 0 and (err <= 5e-15).all()
    assert (img[:nrhs, n:] == sentinel).all() and (img[nrhs] == sentinel).all()
    assert max(bwd_err(A, img[q, :n], B[:, q]) for q in range(nrhs)) <= 1e-14
    # the host entry point on the same padded layout, NULL for iterations and error
    yh = xh.copy()
    assert f.lib.spllt_hip_solve_refined(f.fkeep, len(val), api._dp(val), nrhs, api._dp(yh), ldx, 1, TOL, MAX_ITER,
                                         None, None) == 0
    himg = yh.reshape(nrhs + 1, ldx)
    assert (himg[:nrhs, n:] == sentinel).all() and (himg[nrhs] == sentinel).all()
    assert max(bwd_err(A, himg[q, :n], B[:, q]) for q in range(nrhs)) <= 1e-14
    # nrhs = 0 is a no-op
    before = yh.copy()
    assert f.lib.spllt_hip_solve_refined(f.fkeep, len(val), api._dp(val), 0, api._dp(yh), ldx, 1, TOL, MAX_ITER,
                                         None, None) == 0
    assert np.array_equal(yh, before)


# ---- housekeeping -------------------------------------------------------------------------------
def test_refactorization_release_and_neighbours():
    """a refactorization on the handle is picked up; selected_inverse and factor_batch in between disturb
    nothing; release_refine followed by another call works"""
    A0 = sp.csc_matrix(matgen.nd_like((10, 10, 9), 2))
    f, val0 = make_case(A0, nb=96, nemin=16)
    f.factor(val0).wait()
    rng = np.random.default_rng(5)
    s = 1.0 + 0.3 * rng.random(f.n)
    A = sp.csc_matrix(sp.diags(s) @ A0 @ sp.diags(s))
    val = api.csc_lower_1based(A)[3]
    B = A @ rng.standard_normal((f.n, 6))
    x, it, err = f.solve_refined(val, B, method="pcg", tol=TOL, max_iter=MAX_ITER)
    assert f.refine_status == 0 and it.min() > 2
    f.selected_inverse()
    assert f.factor_batch(np.stack([val0, 2.0 * val0])) == 0
    x1, it1, err1 = f.solve_refined(val, B, method="pcg", tol=TOL, max_iter=MAX_ITER)
    assert f.refine_status == 0 and (abs(it1 - it) <= 2).all()
    Ainv = np.linalg.inv(A0.toarray())
    assert np.abs(f.inverse_diag() - np.diag(Ainv)).max() <= 1e-11 * np.abs(np.diag(Ainv)).max()
    xb = f.solve_batch(np.stack([B[:, 0], B[:, 0]]))
    assert bwd_err(2.0 * A0, xb[1], B[:, 0]) <= 1e-14
    # the new factor is the exact one: no iteration any more
    f.factor(val).wait()
    x2, it2, err2 = f.solve_refined(val, B, method="pcg", tol=TOL, max_iter=MAX_ITER)
    assert f.refine_status == 0 and (it2 == 0).all() and (err2 <= 5e-15).all()
    f.release_refine()
    f.release_refine()
    x3, it3, err3 = f.solve_refined(val, B, method="ir", tol=TOL, max_iter=MAX_ITER)
    assert f.refine_status == 0 and (it3 == 0).all()
    np.testing.assert_allclose(x3, x2, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(f.matvec(val, x3), B, rtol=1e-10, atol=1e-10)
    assert max(bwd_err(A, f.solve_many(B)[:, q], B[:, q]) for q in range(6)) <= 1e-14
    f.close()


def test_errors():
    import torch
    A = matgen.poisson2d(32)
    f, val = make_case(A, nb=16, nemin=8)
    n, nnz = f.n, len(val)
    b = np.ones((n, 3), order="F")
    with pytest.raises(api.SplltError) as ei:          # before the first factorization
        f.solve_refined(val, b)
    assert ei.value.flag == -10 and "factorized" in f.last_error()
    f.factor(val).wait()
    dval = torch.tensor(val, device="cuda")
    xd = torch.ones(3 * n, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(api.SplltError) as ei:
        f.solve_refined_dev(dval.data_ptr(), nnz, xd.data_ptr(), 3, ldx=n - 1)
    assert ei.value.flag == -10 and "ldx" in f.last_error()
    with pytest.raises(api.SplltError) as ei:
        f.solve_refined_dev(dval.data_ptr(), nnz - 1, xd.data_ptr(), 3)
    assert ei.value.flag == -10 and "nnz" in f.last_error()
    with pytest.raises(api.SplltError) as ei:
        f.solve_refined_dev(dval.data_ptr(), nnz, xd.data_ptr(), 3, tol=0.0)
    assert ei.value.flag == -10 and "tol" in f.last_error()
    with pytest.raises(api.SplltError) as ei:
        f.matvec_dev(dval.data_ptr(), nnz, xd.data_ptr(), xd.data_ptr(), 3, ldy=n - 1)
    assert ei.value.flag == -10 and "ldy" in f.last_error()
    assert f.lib.spllt_hip_solve_refined(f.fkeep, nnz, api._dp(val), 3, api._dp(b), n, 7, 1e-14, 5, None, None) == -10
    assert f.lib.spllt_hip_solve_refined(f.fkeep, nnz, api._dp(val), -1, api._dp(b), n, 1, 1e-14, 5, None, None) == -10
    assert f.lib.spllt_hip_solve_refined_dev(f.fkeep, nnz, None, 3, None, n, 1, 1e-14, 5, None, None) == -10
    assert (xd.cpu().numpy() == 1.0).all() and (b == 1.0).all()
    # max_iter = 0: the first iterate and its error, nothing else
    x, it, err = f.solve_refined(val, A @ b, method="pcg", tol=1e-30, max_iter=0)
    assert f.refine_status == 1 and (it == 0).all() and (err > 0).all() and (err <= 1e-14).all()
    x, it, err = f.solve_refined(val, A @ b)            # the handle is still good
    np.testing.assert_allclose(x, b, rtol=0, atol=1e-10)
    f.close()


def test_partitioned_handle_returns_unimplemented():
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
    yd = torch.ones(2 * fs[0].n, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    for f in fs:
        f.wait()
        with pytest.raises(api.SplltError) as ei:
            f.solve_refined(val, np.ones((f.n, 2)))
        assert ei.value.flag == -98 and "partitioned" in f.last_error()
        with pytest.raises(api.SplltError) as ei:
            f.solve_refined_dev(dval.data_ptr(), len(val), xd.data_ptr(), 2)
        assert ei.value.flag == -98
        with pytest.raises(api.SplltError) as ei:
            f.matvec(val, np.ones((f.n, 2)))
        assert ei.value.flag == -98
        with pytest.raises(api.SplltError) as ei:
            f.matvec_dev(dval.data_ptr(), len(val), xd.data_ptr(), yd.data_ptr(), 2)
        assert ei.value.flag == -98
    for f in fs:
        f.close()
