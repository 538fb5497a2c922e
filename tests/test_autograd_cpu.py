"""CPU tests of the differentiable front end: the interface exists in every layer, the (row, column) tables of the
sampled outer product are the analysed pattern, the argument errors that are decided before any device work, the
factor serial of a fresh handle, and the two gradient formulas (dense numpy emulator, the val_k convention) against
central finite differences of numpy.linalg."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import autograd_emulate as em
from helpers import make_case
from spllt_amd import _lib, api, matgen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ("spllt_hip_pattern_outer", "spllt_hip_pattern_outer_dev", "spllt_hip_pattern_outer_batch_dev",
           "spllt_hip_inverse_on_pattern_dev", "spllt_hip_inverse_on_pattern_batch_dev", "spllt_hip_factor_serial")


def test_interface_exists_in_every_layer():
    import spllt_amd
    from spllt_amd import torch_ops
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "spllt_hip.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.HIP_SYMBOLS, name
        assert re.search(r"\b%s\s*\(" % name, header), name
    assert re.search(r"int spllt_hip_pattern_outer_dev\(void \*fkeep, int nvec, const double \*u_dev, int64_t ldu, "
                     r"const double \*v_dev,\s*int64_t ldv, double alpha, double \*out_dev\);", header)
    assert re.search(r"int64_t spllt_hip_factor_serial\(const void \*fkeep, int which\);", header)
    assert '"pattern_row"' in header and '"pattern_col"' in header
    for name in ("pattern_outer", "pattern_outer_dev", "pattern_outer_batch_dev", "pattern_tables",
                 "inverse_on_pattern_dev", "inverse_on_pattern_batch_dev", "factor_serial"):
        assert callable(getattr(api.Factorization, name)), name
    for name in ("solve", "logdet", "solve_batch", "logdet_batch", "pattern_outer"):
        assert callable(getattr(torch_ops.SparseCholesky, name)), name
    assert spllt_amd.SparseCholesky is torch_ops.SparseCholesky
    assert lib.spllt_hip_pattern_outer_dev.argtypes[3] is C.c_int64 and lib.spllt_hip_pattern_outer_dev.argtypes[6] is C.c_double
    assert lib.spllt_hip_pattern_outer_batch_dev.argtypes[9] is C.c_int64
    assert lib.spllt_hip_factor_serial.restype is C.c_int64


@pytest.mark.parametrize("gen", [lambda: matgen.poisson2d(40), lambda: matgen.nd_like((11, 10, 9), 2)],
                         ids=["p2d40", "box11"])
def test_pattern_tables_are_the_analysed_pattern(gen):
    A = gen()
    n, ptr, row, _ = api.csc_lower_1based(A)
    f, _ = make_case(A, nb=64, nemin=16)
    prow, pcol = f.program("pattern_row").view(np.int32), f.program("pattern_col").view(np.int32)
    assert prow.dtype == np.int32 and prow.size == pcol.size == f.nnz
    assert np.array_equal(prow, row - 1)
    assert np.array_equal(pcol, np.repeat(np.arange(n, dtype=np.int32), np.diff(ptr)))
    assert (prow >= pcol).all()
    # a truncated read copies what fits and still reports the full length
    part = np.full(5, -1, dtype=np.int32)
    assert f.lib.spllt_hip_program_get(f.fkeep, b"pattern_row", part.ctypes.data, 12) == 4 * f.nnz
    assert np.array_equal(part[:3], prow[:3]) and (part[3:] == -1).all()
    assert f.lib.spllt_hip_program_get(f.fkeep, b"pattern_val", None, 0) == -1


def test_argument_errors_are_decided_without_a_device():
    f, _ = make_case(matgen.poisson2d(8), nb=8, nemin=4)
    n, nnz = f.n, f.nnz
    x = np.ones(3 * (n + 2))
    out = np.zeros(3 * (nnz + 2))
    host, dev, bat = f.lib.spllt_hip_pattern_outer, f.lib.spllt_hip_pattern_outer_dev, f.lib.spllt_hip_pattern_outer_batch_dev
    xp, op = api._dp(x), api._dp(out)
    for args, word in [((-1, xp, n, xp, n, 1.0, op), "nvec"), ((2, xp, n - 1, xp, n, 1.0, op), "ldu"),
                       ((2, xp, n, xp, n - 1, 1.0, op), "ldv"), ((2, None, n, xp, n, 1.0, op), "null"),
                       ((2, xp, n, None, n, 1.0, op), "null"), ((2, xp, n, xp, n, 1.0, None), "null")]:
        assert host(f.fkeep, *args) == -10
        assert word in f.last_error(), f.last_error()
    # the device entry points take the same checks (a host address is never touched before them)
    xa, oa = x.ctypes.data, out.ctypes.data
    for args, word in [((-1, xa, n, xa, n, 1.0, oa), "nvec"), ((2, xa, n - 1, xa, n, 1.0, oa), "ldu"),
                       ((2, xa, n, xa, n - 1, 1.0, oa), "ldv"), ((2, None, n, xa, n, 1.0, oa), "null"),
                       ((2, xa, n, xa, n, 1.0, None), "null")]:
        assert dev(f.fkeep, *args) == -10
        assert word in f.last_error(), f.last_error()
    for args, word in [((-1, 1, xa, n, xa, n, 1.0, oa, nnz), "nbatch"), ((3, -1, xa, n, xa, n, 1.0, oa, nnz), "nvec"),
                       ((3, 1, xa, n - 1, xa, n, 1.0, oa, nnz), "ldu"), ((3, 1, xa, n, xa, n - 1, 1.0, oa, nnz), "ldv"),
                       ((3, 1, xa, n, xa, n, 1.0, oa, nnz - 1), "ldout"), ((3, 1, None, n, xa, n, 1.0, oa, nnz), "null"),
                       ((3, 1, xa, n, xa, n, 1.0, None, nnz), "null")]:
        assert bat(f.fkeep, *args) == -10
        assert word in f.last_error(), f.last_error()
    assert np.all(x == 1.0) and np.all(out == 0.0)
    # the readers: a null output, and no selected inverse on this handle
    assert f.lib.spllt_hip_inverse_on_pattern_dev(f.fkeep, None) == -10
    assert f.lib.spllt_hip_inverse_on_pattern_batch_dev(f.fkeep, None, nnz) == -10
    assert f.lib.spllt_hip_inverse_on_pattern_batch_dev(f.fkeep, oa, nnz - 1) == -10
    assert "ldout" in f.last_error()
    assert host(None, 1, xp, n, xp, n, 1.0, op) == -10


def test_factor_serial_of_a_fresh_handle():
    f, _ = make_case(matgen.poisson2d(8), nb=8, nemin=4)
    assert f.factor_serial(0) == 0 and f.factor_serial(1) == 0
    assert f.lib.spllt_hip_factor_serial(f.fkeep, 2) == -10 and f.lib.spllt_hip_factor_serial(None, 0) == -10


def _central_difference(fun, val, h):
    g = np.zeros_like(val)
    for k in range(val.size):
        e = np.zeros_like(val)
        e[k] = h
        g[k] = (fun(val + e) - fun(val - e)) / (2.0 * h)
    return g


def test_gradient_formulas_against_finite_differences():
    """The emulator's formulas against central differences of dense numpy.linalg on poisson2d(5).  Step h = 1e-5:
    the truncation error of a central difference is h^2 f''' / 6 ~ 1e-10 relative, its rounding error
    eps |f| / h ~ 1e-10 relative (|f|, |f'| of order one to ten here), so 1e-7 relative to the largest entry of the
    gradient leaves two orders of margin and is still far below the size of any wrong factor or missing term."""
    A = matgen.poisson2d(5)
    n, ptr, row, val = api.csc_lower_1based(A)
    row = (row - 1).astype(np.int64)
    col = np.repeat(np.arange(n), np.diff(ptr))
    rng = np.random.default_rng(5)
    val = val * (1.0 + 0.1 * rng.random(val.size))          # (off the symmetric special case of equal entries)
    B, G = rng.standard_normal((n, 3)), rng.standard_normal((n, 3))
    h = 1e-5

    def loss(v):
        return float((G * np.linalg.solve(em.dense_from_values(n, row, col, v), B)).sum())
    X, gval, gB = em.solve_grads(n, row, col, val, B, G)
    fd = _central_difference(loss, val, h)
    assert np.abs(gval - fd).max() <= 1e-7 * np.abs(fd).max(), np.abs(gval - fd).max()
    fdB = _central_difference(lambda b: float((G * np.linalg.solve(em.dense_from_values(n, row, col, val), b.reshape(n, 3))).sum()),
                              B.ravel(), h).reshape(n, 3)
    assert np.abs(gB - fdB).max() <= 1e-7 * np.abs(fdB).max()

    ld, gld = em.logdet_grad(n, row, col, val)
    fd = _central_difference(lambda v: float(np.linalg.slogdet(em.dense_from_values(n, row, col, v))[1]), val, h)
    assert np.abs(gld - fd).max() <= 1e-7 * np.abs(fd).max(), np.abs(gld - fd).max()
    # the convention matters: without the factor two off the diagonal the formula is wrong by half the entry
    off = row != col
    assert np.abs(gld[off] / 2.0 - fd[off]).max() > 1e-3 * np.abs(fd).max()


def test_reproducible_handle_refuses_the_batch_and_checks_come_first():
    """what the front end decides before any library call needs no device"""
    import torch
    from spllt_amd import SparseCholesky
    chol = SparseCholesky(matgen.poisson2d(6), nb=16, nemin=4, reproducible=True)
    with pytest.raises(NotImplementedError):
        chol.solve_batch(None, None)
    with pytest.raises(NotImplementedError):
        chol.logdet_batch(None)
    val = torch.ones(chol.nnz, dtype=torch.float64)
    with pytest.raises(TypeError):
        chol.logdet(val.float())
    with pytest.raises(TypeError):
        chol.logdet(val.numpy())
    with pytest.raises(ValueError):
        chol.logdet(val)                   # a CPU tensor
    assert chol.f.factor_serial(0) == 0 and chol.device is None
    chol.close()
