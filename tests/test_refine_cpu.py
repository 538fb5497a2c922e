"""CPU tests of the refined solves: the operator tables of spllt_hip_program_get ("matvec_*") applied in
numpy, the numpy restatement of the loop (tests/refine_emulate.py) driven by scipy's factor, and the
parameter errors that need no device."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spl

import refine_emulate as em
from helpers import make_case
from spllt_amd import api, matgen

# the six cases of tests/test_solve_many_gpu.py::CASES (generator, nb)
CASES = [
    ("p2d40-nb16", lambda: matgen.poisson2d(40), 16),
    ("box11-nb64", lambda: matgen.nd_like((11, 10, 9), 2), 64),
    ("p3d14-nb384", lambda: matgen.poisson3d(14), 384),
    ("fe27-nb768", lambda: matgen.fe27((7, 6, 6), 3), 768),
    ("box12-nb512", lambda: matgen.nd_like((10, 12, 12), 3), 512),
    ("box17-nb1024", lambda: matgen.nd_like((12, 17, 16), 3), 1024),
]
U = 2.0 ** -53


def random_pattern(seed):
    """a seeded random symmetric pattern with a full diagonal, n between 1 and 400"""
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.integers(1, 400))
    R = sp.random(n, n, density=min(1.0, float(rng.uniform(1.0, 8.0)) / n), random_state=rng, format="csr")
    A = abs(R) + abs(R).T
    return sp.csc_matrix(A + sp.diags(np.asarray(A.sum(axis=1)).ravel() + 1.0))


def full_matrix(f, ptr, row, val):
    """the symmetric matrix of (pattern, val), user order, from the CSC-lower arrays"""
    Lw = sp.csc_matrix((val, row - 1, ptr - 1), shape=(f.n, f.n))
    return sp.csr_matrix(Lw + sp.tril(Lw, -1).T)


def exact_product(M, X):
    """M @ X with every row summed in extended precision, and |M| |X|, the entries per row"""
    M = sp.csr_matrix(M)
    M.sort_indices()
    X = X.reshape(M.shape[0], -1)
    prod = M.data.astype(np.longdouble)[:, None] * X.astype(np.longdouble)[M.indices]
    nz = np.flatnonzero(np.diff(M.indptr) > 0)
    y = np.zeros((M.shape[0], X.shape[1]), dtype=np.longdouble)
    ya = np.zeros_like(y)
    y[nz] = np.add.reduceat(prod, M.indptr[:-1][nz], axis=0)
    ya[nz] = np.add.reduceat(abs(prod), M.indptr[:-1][nz], axis=0)
    return y, ya, np.diff(M.indptr)


def check_tables(A):
    n, ptr, row, _ = api.csc_lower_1based(A)
    f, val0 = make_case(A, nb=64, nemin=16)
    rowptr, col, src = f.matvec_tables()
    nnz = len(val0)
    order = f.sym("order")
    assert rowptr.dtype == np.int64 and col.dtype == np.int32 and src.dtype == np.int32
    assert len(rowptr) == n + 1 and rowptr[0] == 0 and rowptr[-1] == len(col) == len(src) == 2 * nnz - n
    assert (np.diff(rowptr) >= 1).all()
    # every val index once (diagonal) or twice (off-diagonal)
    count = np.bincount(src, minlength=nnz)
    rows_of = np.repeat(np.arange(n), np.diff(rowptr))
    is_diag = np.zeros(nnz, dtype=bool)
    is_diag[src[rows_of == col]] = True
    assert (count[is_diag] == 1).all() and (count[~is_diag] == 2).all() and is_diag.sum() == n
    # columns sorted inside a row, strictly
    inner = np.ones(len(col), dtype=bool)
    inner[rowptr[:-1]] = False
    assert (np.diff(col)[inner[1:]] > 0).all()
    # symmetric structure, the same val behind (p, c) and (c, p)
    S1 = sp.csr_matrix((src + 1, col, rowptr), shape=(n, n))
    assert (S1 != S1.T).nnz == 0
    # the product against (P A P^T) x
    rng = np.random.default_rng(7)
    val = rng.standard_normal(nnz)
    X = rng.standard_normal((n, 3))
    Af = full_matrix(f, ptr, row, val)
    P = sp.csr_matrix((np.ones(n), (order, np.arange(n))), shape=(n, n))
    PAPt = sp.csr_matrix(P @ Af @ P.T)
    Xp = np.empty_like(X)
    Xp[order] = X
    want, wabs, nrow = exact_product(PAPt, Xp)
    got = em.apply_tables(rowptr, col, src, val, Xp)
    assert (abs(got - want) <= 2.0 * nrow[:, None] * U * wabs).all()
    # ... which is A x in the user's order
    np.testing.assert_allclose(got[order], Af @ X, rtol=1e-12, atol=1e-12)
    f.close()


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_operator_tables_of_the_cases(name):
    check_tables(next(c for c in CASES if c[0] == name)[1]())


@pytest.mark.parametrize("seed", range(20))
def test_operator_tables_of_random_patterns(seed):
    check_tables(random_pattern(seed))


# ---- the emulator, driven by scipy's factor ----------------------------------------------------
EMU_CASES = {
    "p2d40": lambda: matgen.poisson2d(40),
    "box11": lambda: matgen.nd_like((11, 10, 9), 2),
    "p3d14": lambda: matgen.poisson3d(14),
    "fe27": lambda: matgen.fe27((7, 6, 6), 3),
    "box12": lambda: matgen.nd_like((10, 12, 12), 3),
}
TOL, MAX_ITER, CAP = 5e-15, 60, 57


def perturbed(A0, eps, seed):
    """A = S A0 S, S = diag(1 + eps u), u uniform(0, 1) seeded: the pattern of A0; and b = A randn"""
    rng = np.random.default_rng(seed)
    n = A0.shape[0]
    s = 1.0 + eps * rng.random(n)
    A = sp.csc_matrix(sp.diags(s) @ sp.csc_matrix(A0) @ sp.diags(s))
    return A, A @ rng.standard_normal(n), s


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("name", list(EMU_CASES))
def test_emulator_converges_where_the_table_says_so(name, seed):
    A0 = sp.csc_matrix(EMU_CASES[name]())
    M = spl.splu(A0, permc_spec="MMD_AT_PLUS_A").solve
    for eps, method in ((0.0, 0), (0.0, 1), (0.02, 0), (0.02, 1), (0.3, 1)):
        A, b, _ = perturbed(A0, eps, seed)
        x, it, err, ok = em.refine(A, b, M, method, TOL, MAX_ITER)
        print(name, seed, "eps", eps, "method", method, "iterations", it, "error", err)
        assert ok and err <= TOL and it <= CAP, (eps, method, it, err)
        if eps == 0.0:
            assert it == 0
        r = b - A @ x
        assert np.linalg.norm(r) / (np.linalg.norm(b) + abs(A).max() * np.linalg.norm(x)) <= 1e-14


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("name", list(EMU_CASES))
def test_emulator_refinement_does_not_converge_at_eps_0p3(name, seed):
    A0 = sp.csc_matrix(EMU_CASES[name]())
    M = spl.splu(A0, permc_spec="MMD_AT_PLUS_A").solve
    A, b, _ = perturbed(A0, 0.3, seed)
    x, it, err, ok = em.refine(A, b, M, 0, TOL, MAX_ITER)
    print(name, seed, "iterations", it, "best error", err)
    assert not ok and it == MAX_ITER and err > TOL
    # the best-iterate rule: never worse than M^-1 b
    x0 = M(b)
    e0 = em.backward_error(b - A @ x0, b, x0, abs(A).max())
    assert err <= e0


def test_emulator_special_vectors():
    A0 = sp.csc_matrix(matgen.poisson2d(12))
    M = spl.splu(A0).solve
    n = A0.shape[0]
    for method in (0, 1):
        x, it, err, ok = em.refine(A0, np.zeros(n), M, method, TOL, MAX_ITER)
        assert ok and it == 0 and err == 0.0 and (x == 0.0).all()
        b = np.ones(n)
        b[3] = np.nan
        x, it, err, ok = em.refine(A0, b, M, method, TOL, MAX_ITER)
        assert not ok and it == 0


# ---- parameter errors that need no device -------------------------------------------------------
def test_parameter_errors_without_a_device():
    A = matgen.poisson2d(16)
    f, val = make_case(A, nb=16, nemin=8)
    n, nnz = f.n, len(val)
    x = np.ones(2 * n)
    y = np.ones(2 * n)
    it = np.zeros(2, dtype=np.int32)
    err = np.zeros(2)
    L = f.lib
    mv = lambda *a: L.spllt_hip_matvec(f.fkeep, *a)
    assert mv(nnz, None, 2, api._dp(x), n, api._dp(y), n) == -10
    assert mv(nnz, api._dp(val), 2, None, n, api._dp(y), n) == -10
    assert mv(nnz, api._dp(val), 2, api._dp(x), n, None, n) == -10
    assert mv(nnz, api._dp(val), -1, api._dp(x), n, api._dp(y), n) == -10
    assert mv(nnz - 1, api._dp(val), 2, api._dp(x), n, api._dp(y), n) == -10 and "nnz" in f.last_error()
    assert mv(nnz, api._dp(val), 2, api._dp(x), n - 1, api._dp(y), n) == -10 and "ldx" in f.last_error()
    assert mv(nnz, api._dp(val), 2, api._dp(x), n, api._dp(y), n - 1) == -10 and "ldy" in f.last_error()
    assert mv(nnz, api._dp(val), 0, api._dp(x), n, api._dp(y), n) == 0          # a no-op
    assert L.spllt_hip_matvec_dev(f.fkeep, nnz, None, 2, None, n, None, n, 0) == -10
    sr = lambda *a: L.spllt_hip_solve_refined(f.fkeep, *a)
    good = (1, 1e-14, 10, api._ip(it), api._dp(err))
    assert sr(nnz, None, 2, api._dp(x), n, *good) == -10
    assert sr(nnz, api._dp(val), 2, None, n, *good) == -10
    assert sr(nnz, api._dp(val), -2, api._dp(x), n, *good) == -10
    assert sr(nnz + 1, api._dp(val), 2, api._dp(x), n, *good) == -10 and "nnz" in f.last_error()
    assert sr(nnz, api._dp(val), 2, api._dp(x), n - 1, *good) == -10 and "ldx" in f.last_error()
    assert sr(nnz, api._dp(val), 2, api._dp(x), n, 2, 1e-14, 10, None, None) == -10 and "method" in f.last_error()
    assert sr(nnz, api._dp(val), 2, api._dp(x), n, 1, 0.0, 10, None, None) == -10 and "tol" in f.last_error()
    assert sr(nnz, api._dp(val), 2, api._dp(x), n, 1, float("nan"), 10, None, None) == -10
    assert sr(nnz, api._dp(val), 2, api._dp(x), n, 1, 1e-14, -1, None, None) == -10 and "max_iter" in f.last_error()
    assert sr(nnz, api._dp(val), 2, api._dp(x), n, *good) == -10 and "factorized" in f.last_error()
    assert sr(nnz, api._dp(val), 0, api._dp(x), n, *good) == 0          # a no-op, factorized or not
    assert L.spllt_hip_solve_refined_dev(f.fkeep, nnz, None, 2, None, n, 1, 1e-14, 10, None, None) == -10
    assert L.spllt_hip_release_refine(f.fkeep) == 0 and L.spllt_hip_release_refine(None) == -10
    assert (x == 1.0).all() and (y == 1.0).all()
    with pytest.raises(api.SplltError):
        f.solve_refined(val, np.ones(n), method="gmres")
    f.close()


def test_partitioned_handle_is_unimplemented_without_a_device():
    A = matgen.poisson2d(32)
    f, val = make_case(A, nb=16, nemin=8, prune=True, ncpu=2)
    f.set_partition(0, 2)
    x = np.ones(f.n)
    y = np.ones(f.n)
    assert f.lib.spllt_hip_matvec(f.fkeep, len(val), api._dp(val), 1, api._dp(x), f.n, api._dp(y), f.n) == -98
    assert "partitioned" in f.last_error()
    assert f.lib.spllt_hip_solve_refined(f.fkeep, len(val), api._dp(val), 1, api._dp(x), f.n, 1, 1e-14, 5, None, None) == -98
    f.close()
