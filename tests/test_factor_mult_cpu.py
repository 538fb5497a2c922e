"""CPU tests of the factor products and the samplers: the interface exists in every layer, both product
directions interpreted in numpy in the order of the "rsolve_*" tables equal the dense products, nothing reads the
strict upper triangle of a diagonal tile, the numpy Philox of the noise test passes the published known-answer
vectors, and the argument errors that are decided before any device work."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import scipy.linalg as sl

from factor_mult_emulate import emulate_factor_mult, philox4x32_10, white_noise_reference
from helpers import dense_arena, lower_mask, make_case
from spllt_amd import _lib, api, matgen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = [
    ("p2d12-nb8", lambda: matgen.poisson2d(12), 8, 4),
    ("box11-nb64", lambda: matgen.nd_like((11, 10, 9), 2), 64, 16),
]
NAMES = [c[0] for c in CASES]

SYMBOLS = ("spllt_hip_factor_mult", "spllt_hip_factor_mult_dev", "spllt_hip_release_factor_mult",
           "spllt_hip_sample", "spllt_hip_sample_dev", "spllt_hip_white_noise_dev")


def test_interface_exists_in_every_layer():
    lib = _lib.load()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.HIP_SYMBOLS
    header = open(os.path.join(ROOT, "include", "spllt_hip.h")).read()
    assert re.search(r"int\s+spllt_hip_factor_mult\(void \*fkeep, int nvec, double \*x_host, int64_t ldx, int job\);", header)
    assert re.search(r"int\s+spllt_hip_factor_mult_dev\(void \*fkeep, int nvec, double \*x_dev, int64_t ldx, int job,\s*"
                     r"int pivot_order\);", header)
    assert re.search(r"int\s+spllt_hip_sample_dev\(void \*fkeep, int nsamp, double \*x_dev, int64_t ldx, int kind,\s*"
                     r"uint64_t seed, uint64_t first_sample, const double \*mean_dev\);", header)
    assert re.search(r"int\s+spllt_hip_white_noise_dev\(void \*fkeep, int nsamp, double \*z_dev, int64_t ldz,\s*"
                     r"uint64_t seed, uint64_t first_sample\);", header)
    for m in ("factor_mult", "factor_mult_dev", "sample", "sample_dev", "white_noise", "release_factor_mult"):
        assert callable(getattr(api.Factorization, m)), m
    assert lib.spllt_hip_factor_mult.argtypes[3] is C.c_int64 and lib.spllt_hip_sample.argtypes[5] is C.c_uint64
    from spllt_amd import torch_ops
    assert callable(torch_ops.SparseCholesky.sample)


@functools.lru_cache(maxsize=None)
def _case(name):
    _, gen, nb, nemin = next(c for c in CASES if c[0] == name)
    A = gen()
    f, _val = make_case(A, nb=nb, nemin=nemin)
    arena = dense_arena(f, A)
    n = f.n
    P = np.empty(n, dtype=np.int64)
    P[f.sym("order")] = np.arange(n)
    L = sl.cholesky(A.toarray()[np.ix_(P, P)], lower=True)
    X = np.random.default_rng(0).standard_normal((n, 3))
    return f, arena, L, X


@pytest.mark.parametrize("name", NAMES)
def test_products_in_table_order_equal_the_dense_products(name):
    f, arena, L, X = _case(name)
    for transpose in (False, True):
        got = emulate_factor_mult(f, arena, X, transpose)
        assert np.isfinite(got).all()        # (the scratch starts as NaN: every slot read was written first)
        want = (L.T if transpose else L) @ X
        # rtol 1e-13 of the size of what is summed, (|L| |X|)_ij: two correct fp64 sums of an entry that cancels --
        # this one and the BLAS reference -- differ by a multiple of 2^-53 of THAT, not of the entry (on box11-nb64
        # an elementwise rtol of 1e-13 with atol 0 fails between them while this ratio is 1.5e-15)
        size = np.abs(L.T if transpose else L) @ np.abs(X)
        err = float((np.abs(got - want) / size).max())
        print(name, "transpose" if transpose else "plain", "max |got - want| / (|L| |X|)", err)
        assert err <= 1e-13


@pytest.mark.parametrize("name", NAMES)
def test_strict_upper_triangles_of_diagonal_tiles_are_never_read(name):
    f, arena, L, X = _case(name)
    poisoned = arena.copy()
    upper = ~lower_mask(f)
    assert upper.any()
    poisoned[upper] = np.nan
    for transpose in (False, True):
        assert np.array_equal(emulate_factor_mult(f, poisoned, X, transpose), emulate_factor_mult(f, arena, X, transpose))


def test_numpy_philox_passes_the_known_answer_vectors():
    """the vectors of the Random123 distribution (kat_vectors, philox4x32 10)"""
    z, ff = np.uint32(0), np.uint32(0xFFFFFFFF)
    assert [int(v) for v in philox4x32_10(z, z, z, z, 0, 0)] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert [int(v) for v in philox4x32_10(ff, ff, ff, ff, 0xFFFFFFFF, 0xFFFFFFFF)] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6,
                                                                                   0x6d5451fd]
    got = philox4x32_10(np.uint32(0x243f6a88), np.uint32(0x85a308d3), np.uint32(0x13198a2e), np.uint32(0x03707344),
                        0xa4093822, 0x299f31d0)
    assert [int(v) for v in got] == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]
    Z = white_noise_reference(2000, 8, seed=7)
    assert np.isfinite(Z).all() and abs(Z.mean()) < 0.05 and abs(Z.std() - 1.0) < 0.05
    assert np.array_equal(Z[:, 2:5], white_noise_reference(2000, 3, seed=7, first_sample=2))


def test_argument_errors_on_an_analysed_handle():
    f, val = make_case(matgen.poisson2d(8), nb=8, nemin=4)
    n = f.n
    x = np.ones(3 * (n + 2))
    mult, mult_dev = f.lib.spllt_hip_factor_mult, f.lib.spllt_hip_factor_mult_dev
    for nvec, ptr, ldx, job, word in [(-1, api._dp(x), n, 0, "nrhs"), (3, api._dp(x), n - 1, 0, "ldx"),
                                      (3, api._dp(x), n, 3, "job"), (3, api._dp(x), n, -1, "job"), (3, None, n, 0, "null")]:
        assert mult(f.fkeep, nvec, ptr, ldx, job) == -10
        assert word in f.last_error(), f.last_error()
    addr = x.ctypes.data
    for nvec, ptr, ldx, job, word in [(-1, addr, n, 0, "nrhs"), (3, addr, n - 1, 0, "ldx"), (3, addr, n, 7, "job"),
                                      (3, None, n, 0, "null")]:
        assert mult_dev(f.fkeep, nvec, ptr, ldx, job, 0) == -10
        assert word in f.last_error(), f.last_error()
    for kind in (-1, 2):
        assert f.lib.spllt_hip_sample(f.fkeep, 3, api._dp(x), n, kind, 0, 0, None) == -10
        assert "kind" in f.last_error(), f.last_error()
        assert f.lib.spllt_hip_sample_dev(f.fkeep, 3, addr, n, kind, 0, 0, None) == -10
    assert f.lib.spllt_hip_sample(f.fkeep, 3, api._dp(x), n - 1, 0, 0, 0, None) == -10
    assert f.lib.spllt_hip_white_noise_dev(f.fkeep, -1, addr, n, 0, 0) == -10
    # nothing factorized yet
    assert mult(f.fkeep, 3, api._dp(x), n + 2, 0) == -10 and "factorized" in f.last_error()
    assert mult(f.fkeep, 0, api._dp(x), n, 0) == -10
    assert f.lib.spllt_hip_sample(f.fkeep, 3, api._dp(x), n, 1, 0, 0, None) == -10 and "factorized" in f.last_error()
    assert f.lib.spllt_hip_white_noise_dev(f.fkeep, 3, addr, n, 0, 0) == -10
    with pytest.raises(api.SplltError) as ei:
        f.sample(2, kind="variance")
    assert ei.value.flag == -10
    assert (x == 1.0).all()
    assert mult(None, 3, api._dp(x), n, 0) == -10
    # no engine, no workspace: nothing was created on the way to these errors, and there is nothing to release
    assert not f.device_factor_ptr()
    assert f.lib.spllt_hip_release_factor_mult(f.fkeep) == 0
    assert f.lib.spllt_hip_release_factor_mult(None) == -10
    f.close()
