"""CPU tests of the batched factorization (spllt_hip_factor_batch and friends): the interface exists in
every layer; the batch program -- the single-stream, unfused program with 64-wide panels that
batch.hip implements -- holds only the launch kinds, tile edges and unit modes the batch kernels know,
reproduces the dense factor when tests/emulate.py interprets it, and does not depend on the handle's
engine flags; argument errors that need no device come back as the parameter flag."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from batch_emulate import BatchProgramView, check_batch_program
from emulate import emulate_program
from helpers import dense_arena, lower_mask, make_case, rel_err
from spllt_amd import _lib, api, matgen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "dense_chol_*.npz")))
BATCH_SYMBOLS = ["spllt_hip_factor_batch", "spllt_hip_factor_batch_dev", "spllt_hip_batch_status",
                 "spllt_hip_solve_batch", "spllt_hip_solve_batch_dev", "spllt_hip_get_factor_batch",
                 "spllt_hip_device_factor_batch", "spllt_hip_log_det_batch", "spllt_hip_batch_launches",
                 "spllt_hip_release_batch"]
PROGRAM_NAMES = ["batch_launches", "batch_units", "batch_tiles", "batch_chains", "batch_relpos", "batch_dinv_size"]


def _golden_case(path, **kw):
    g = np.load(path)
    n = int(g["n"])
    low = sp.csc_matrix((g["val"], g["row"] - 1, g["ptr"] - 1), shape=(n, n))
    A = sp.csc_matrix(low + sp.tril(low, -1).T)
    f = api.Factorization(n, g["ptr"], g["row"], nb=16, nemin=4, prune_tree=False, order=g["order_in"], **kw)
    return A, f, np.asarray(g["val"], dtype=np.float64)


def _generated_case(gen, nb, **kw):
    A = gen()
    f, val = make_case(A, nb=nb, nemin=16, **kw)
    return A, f, val


CASES = [(os.path.basename(p), lambda p=p, **kw: _golden_case(p, **kw)) for p in GOLD] + [
    ("box11-nb64", lambda **kw: _generated_case(lambda: matgen.nd_like((11, 10, 9), 2), 64, **kw)),
    ("p3d14-nb384", lambda **kw: _generated_case(lambda: matgen.poisson3d(14), 384, **kw)),
    ("fe27-nb768", lambda **kw: _generated_case(lambda: matgen.fe27((7, 6, 6), 3), 768, **kw)),
]


def test_interface_exists_in_every_layer():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "spllt_hip.h")).read()
    for name in BATCH_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.HIP_SYMBOLS, name
        assert re.search(r"\b%s\s*\(" % name, header), name
    assert "batched factorization (single GPU)" in header
    for name in ("factor_batch", "factor_batch_dev", "batch_status", "solve_batch", "solve_batch_dev",
                 "get_factor_batch", "log_det_batch", "batch_launches", "release_batch"):
        assert callable(getattr(api.Factorization, name)), name
    assert lib.spllt_hip_factor_batch.argtypes[5] is C.c_int64 and lib.spllt_hip_solve_batch.argtypes[3] is C.c_int64


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_batch_program_is_what_the_kernels_implement_and_reproduces_the_dense_factor(name):
    assert len(GOLD) == 3, GOLD        # the three golden patterns are among the cases
    A, f, val = next(c[1] for c in CASES if c[0] == name)()
    if name == "fe27-nb768":
        assert int(f.sym("bcol_width").max()) > 64, "the case degenerated: no block column wider than one panel"
    launches, units, tiles = check_batch_program(f)
    assert len(launches) > 0 and (launches[:, 0] == 4).any()
    # single stream: no launch waits for an event of another stream
    assert (launches[:, 6] == 0).all()
    got = emulate_program(BatchProgramView(f), val)
    err = rel_err(got, dense_arena(f, A), lower_mask(f))
    print(name, "launches", len(launches), "rel_err", err)
    assert err < 1e-13, err
    f.close()


@pytest.mark.parametrize("name", ["box11-nb64", "fe27-nb768", os.path.basename(GOLD[0]) if GOLD else "none"])
def test_batch_program_does_not_depend_on_the_engine_flags(name):
    make = next(c[1] for c in CASES if c[0] == name)
    ref = None
    for flags in (0, 2, 4096):
        A, f, val = make(engine_flags=flags)
        tabs = [np.asarray(f.program(k)).tobytes() if k != "batch_dinv_size" else f.program(k) for k in PROGRAM_NAMES]
        if ref is None:
            ref = tabs
            # ... while the handle's own program does (4096: the deterministic engine buffers its updates)
        else:
            assert tabs == ref, flags
        f.close()
    A, f0, _ = make(engine_flags=0)
    A, f1, _ = make(engine_flags=4096)
    assert np.asarray(f0.program("launches")).tobytes() != np.asarray(f1.program("launches")).tobytes()
    f0.close()
    f1.close()


@pytest.mark.parametrize("name", ["box11-nb64", "fe27-nb768"])
def test_batch_program_does_not_depend_on_the_engine_switches_of_the_environment(name, monkeypatch):
    """SPLLT_CHAIN4=1 / SPLLT_SUBTREES=1 (and the other switches of the program's shape, such as the size limit
    of the fused panels) are switches of the single-handle engine; the batch kernels implement
    neither chain blocks nor subtree tasks, and the batch program keeps its fixed options under them (it used to
    be built WITH them, and factor_batch then refused it with -99)."""
    make = next(c[1] for c in CASES if c[0] == name)
    A, f, val = make()
    ref = [np.asarray(f.program(k)).tobytes() if k != "batch_dinv_size" else f.program(k) for k in PROGRAM_NAMES]
    f.close()
    monkeypatch.setenv("SPLLT_CHAIN4", "1")
    monkeypatch.setenv("SPLLT_SUBTREES", "1")
    monkeypatch.setenv("SPLLT_SUBTREE_US", "300")
    monkeypatch.setenv("SPLLT_FUSED_PANEL_MAX", "1000000")
    A, f, val = make()
    kinds = set(f.program("launches")[:, 0].tolist())
    assert 10 in kinds and (name != "fe27-nb768" or 8 in kinds)      # the handle's own program follows the switches
    check_batch_program(f)
    tabs = [np.asarray(f.program(k)).tobytes() if k != "batch_dinv_size" else f.program(k) for k in PROGRAM_NAMES]
    assert tabs == ref
    f.close()


def test_unknown_batch_program_name():
    f, val = make_case(matgen.poisson2d(8), nb=8, nemin=4)
    with pytest.raises(KeyError):
        f.program("batch_panels")
    with pytest.raises(KeyError):
        f.program("batch_solve_units")
    assert f.program("batch_dinv_size") > 0
    f.close()


def test_argument_errors_on_an_analysed_handle():
    f, val = make_case(matgen.poisson2d(8), nb=8, nemin=4)
    n, nnz = f.n, f.nnz
    vals = np.tile(val, (3, 1))
    vp = C.c_void_p(vals.ctypes.data)
    for fn in (f.lib.spllt_hip_factor_batch, f.lib.spllt_hip_factor_batch_dev):
        for nbatch, nz, ptr, ldval, word in [(3, nnz, None, nnz, "null"), (-1, nnz, vp, nnz, "nbatch"),
                                            (3, nnz + 1, vp, nnz + 1, "nnz"), (3, nnz, vp, nnz - 1, "ldval")]:
            assert fn(f.akeep, f.fkeep, nbatch, nz, ptr, ldval) == -10
            assert word in f.last_error(), f.last_error()
        assert fn(None, f.fkeep, 3, nnz, vp, nnz) == -10
        assert fn(f.akeep, None, 3, nnz, vp, nnz) == -10
        assert fn(f.akeep, f.fkeep, 0, nnz, vp, nnz) == 0          # an empty batch is a no-op
    x = np.ones(3 * 2 * (n + 1))
    xp = C.c_void_p(x.ctypes.data)
    for nrhs, ptr, ldx, job, word in [(-1, xp, n, 0, "nrhs"), (2, xp, n - 1, 0, "ldx"), (2, xp, n, 3, "job"),
                                      (2, xp, n, -1, "job"), (2, None, n, 0, "null")]:
        assert f.lib.spllt_hip_solve_batch(f.fkeep, nrhs, ptr, ldx, job) == -10
        assert word in f.last_error(), f.last_error()
        assert f.lib.spllt_hip_solve_batch_dev(f.fkeep, nrhs, ptr, ldx, job, 0) == -10
        assert word in f.last_error(), f.last_error()
    # good arguments, no batch yet: solves and readers say so
    assert f.lib.spllt_hip_solve_batch(f.fkeep, 2, xp, n + 1, 0) == -10
    assert "no batch" in f.last_error()
    assert (x == 1.0).all()
    out = np.zeros(f.sym_info()["arena"])
    assert f.lib.spllt_hip_get_factor_batch(f.fkeep, 0, api._dp(out), out.size) == -10
    assert f.lib.spllt_hip_get_factor_batch(f.fkeep, 0, None, out.size) == -10
    assert f.lib.spllt_hip_log_det_batch(f.fkeep, api._dp(out)) == -10
    assert f.lib.spllt_hip_log_det_batch(f.fkeep, None) == -10
    stride = C.c_int64(5)
    assert f.lib.spllt_hip_device_factor_batch(f.fkeep, C.byref(stride)) is None and stride.value == 0
    assert f.lib.spllt_hip_batch_status(f.fkeep, None, None, 0) == 0
    assert f.lib.spllt_hip_batch_status(None, None, None, 0) == -10
    assert f.lib.spllt_hip_batch_launches(f.fkeep) == 0
    assert f.lib.spllt_hip_release_batch(f.fkeep) == 0
    assert f.lib.spllt_hip_release_batch(None) == -10
    flags, cols = f.batch_status()
    assert flags.size == 0 and cols.size == 0
    with pytest.raises(api.SplltError) as ei:
        f.solve_batch(np.ones((3, n)))
    assert ei.value.flag == -10
    with pytest.raises(ValueError, match="length"):       # (decided in Python, before the library sees the pointer)
        f.solve_batch(np.ones((3, n + 1)))
    with pytest.raises(ValueError):
        f.solve_batch(np.ones(n))
    with pytest.raises(api.SplltError) as ei:
        f.factor_batch(np.ones((3, nnz + 2)), ldval=nnz - 1)
    assert ei.value.flag == -10
    f.close()


def test_partitioned_handle_is_refused_without_a_device():
    f, val = make_case(matgen.poisson2d(16), nb=16, nemin=8, prune=True, ncpu=2)
    f.set_partition(0, 2)
    vals = np.tile(val, (2, 1))
    with pytest.raises(api.SplltError) as ei:
        f.factor_batch(vals)
    assert ei.value.flag == -98 and "partitioned" in f.last_error()
    x = np.ones(2 * f.n)
    assert f.lib.spllt_hip_solve_batch(f.fkeep, 1, C.c_void_p(x.ctypes.data), f.n, 0) == -98
    f.close()


def test_factor_batch_without_gpu_fails_loudly():
    import torch
    A = matgen.poisson2d(10)
    f, val = make_case(A, nb=8)
    if not torch.cuda.is_available():
        with pytest.raises(api.SplltError) as ei:
            f.factor_batch(np.tile(val, (3, 1)))
        assert ei.value.flag == -30, "factor_batch must fail loudly without a HIP device (no CPU fallback)"
        flags, cols = f.batch_status()
        assert flags.size == 0
        with pytest.raises(api.SplltError) as ei:
            f.solve_batch(np.ones((3, f.n)))
        assert ei.value.flag == -10
    f.close()
    assert f.akeep.value is None and f.fkeep.value is None
