"""CPU tests of the batch's factor adjoint (include/spllt_hip_batch_adjoint.h): the family exists in every layer
under a prototype table of its own; the sweep of tests/factor_adjoint_emulate.py on the batch's selected-inversion
tables ("batch_selinv_*", panels of 64 whatever the handle's panel width) reproduces the dense formula for members
of a batch; the launch count of a sweep follows from the tables; argument errors that need no device come back as
stated; the entry ladder against the recorded rows of the siblings (batch_adjoint_ladder.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import batch_adjoint_emulate as be
import batch_adjoint_ladder as ladder
import capi_ladder
import factor_adjoint_emulate as fe
from helpers import make_case
from selinv_emulate import expected_z
from spllt_amd import _lib, api, matgen, torch_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spllt_hip_batch_adjoint.h")
BAR = 1e-12          # of the emulated batched inversion (tests/test_selinv_batch_cpu.py)
MEMBERS = (0, 1, 2)
_measured = {}


def _declared():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return set(re.findall(r"\b(spllt_\w+)\s*\(", txt))


def test_every_declared_symbol_is_exported_and_has_a_prototype():
    lib = _lib.load()
    names = _declared()
    assert len(names) == 9 and names == set(_lib.BATCH_ADJOINT_SYMBOLS) == set(_lib._BATCH_ADJOINT)
    assert not names & set(_lib.HIP_SYMBOLS) and not names & set(_lib.PROTOTYPES)
    assert set(_lib.PROTOTYPES) == set(_lib.IFACE_SYMBOLS) | set(_lib.HIP_SYMBOLS)
    for s in sorted(names):
        fn = getattr(lib, s)
        assert (fn.restype, list(fn.argtypes)) == (_lib._BATCH_ADJOINT[s][0], _lib._BATCH_ADJOINT[s][1]), s
    assert names == set(ladder.ENTRIES) | {ladder.RELEASE[0]}
    txt = open(HEADER).read()
    assert "<stdint.h>" in txt and 'extern "C"' in txt and "#include \"" not in txt
    assert "folded into" in txt and "spllt_hip.h" in txt
    for name in ("factor_adjoint_seed_batch", "factor_adjoint_seed_batch_dev", "set_factor_adjoint_batch",
                 "get_factor_adjoint_batch", "device_factor_adjoint_batch_ptr", "factor_adjoint_batch",
                 "factor_adjoint_batch_dev", "batch_adjoint_launches", "release_factor_adjoint_batch"):
        assert callable(getattr(api.Factorization, name)), name
    for name in ("factor_apply_batch", "rsample_batch"):
        assert callable(getattr(torch_ops.SparseCholesky, name)), name


def test_debug_hook():
    lib = _lib.load()
    assert lib.spllt_hip_debug(b"batch_fadj_fused=0") == 0 and lib.spllt_hip_debug(b"batch_fadj_fused=1") == 0
    assert lib.spllt_hip_debug(b"batch_fadj_fused=2") == -1 and lib.spllt_hip_debug(b"batch_fadj_fused=") == -1


@pytest.mark.parametrize("name", be.IDS)
def test_emulated_sweep_on_the_batch_tables_matches_the_dense_formula(name):
    c = be.case(name)
    f, mask = c["f"], c["mask"]
    assert f.program("panel_width") != 64
    worst = 0.0
    for b in MEMBERS:
        m = be.member(name, b)
        rng = np.random.default_rng(50 + b)
        seeds = {"random": np.where(mask, rng.standard_normal(m["L"].shape), 0.0),
                 "rank3": fe.outer_seed(f, rng.standard_normal((f.n, 3)), rng.standard_normal((f.n, 3)), 0.7)}
        for what, seed in seeds.items():
            G = be.emulate(name, m["L"], seed)
            assert np.isfinite(G[mask]).all(), "an entry of the pattern was read before it was written"
            err = fe.rel(G, fe.dense_factor_adjoint(f, m["Ld"], seed), mask)
            print(f"{name} member {b} {what}: {err:.2e}")
            worst = max(worst, err)
        G = be.emulate(name, m["L"], fe.logdet_seed(f, m["L"]))
        assert np.isfinite(G[mask]).all()
        err = fe.rel(G, be.logdet_weight(f) * expected_z(f, m["A"]), mask)
        print(f"{name} member {b} logdet against (2 - delta) inv(A_b): {err:.2e}")
        worst = max(worst, err)
    _measured[name] = worst
    print(f"{name}: e_max = {worst:.3e}")
    assert worst <= BAR, worst
    assert worst <= be.E_MAX, "the recorded e_max of batch_adjoint_emulate.py is below what this run measures"


# (fused-eligible steps, steps, largest K-slice count) of the batch program per case
STEP_COUNTS = {"p2d12-nb4": (15, 15), "p2d16-nb8-pw32": (11, 11), "p2d32-nb16": (21, 22), "p2d64-nb100-pw32": (6, 9),
               "p3d10-nb48": (4, 9), "box8-nb96": (2, 9), "box12-nb256": (2, 20), "fe27-nb64": (2, 5),
               "box11-nb100-pw48": (2, 17)}


@pytest.mark.parametrize("name", be.IDS)
def test_launch_counts_follow_from_the_tables(name):
    t = be.case(name)["t"]
    st = be.steps(t)
    assert (sum(ok for _, ok in st), len(st)) == STEP_COUNTS[name]
    fused, unfused = be.expected_launches(t, True), be.expected_launches(t, False)
    assert unfused == sum(1 for r in t["launches"] if int(r[3]) > 0) + 1
    assert fused == unfused - sum(sum(1 for i in idx if int(t["launches"][i][3]) > 0) - 1 for idx, ok in st if ok)
    assert all(1 <= sum(1 for i in idx if int(t["launches"][i][3]) > 0) <= 3 for idx, _ in st)
    if name == "p2d12-nb4":
        assert fused == len(st) + 1 < unfused
    if name == fe.KSLICE_CASE:
        assert int(t["units"]["nsplit"].max()) == 4
    if name == "box11-nb100-pw48":
        assert int(t["units"]["nsplit"].max()) == 3


def test_argument_errors_on_an_analysed_handle():
    f, val = make_case(matgen.poisson2d(8), nb=8, nemin=4)
    n, nnz, lib, arena = f.n, f.nnz, f.lib, f.sym_info()["arena"]
    out = np.zeros(3 * max(nnz, arena) + 8)
    op, vp = api._dp(out), C.c_void_p(out.ctypes.data)
    seed = lib.spllt_hip_factor_adjoint_seed_batch
    seed_dev = lib.spllt_hip_factor_adjoint_seed_batch_dev
    # null handle
    assert seed(None, 1, op, op, n, 1.0, 0, 0) == -10 and seed_dev(None, 1, vp, vp, n, 1.0, 0, 0) == -10
    assert lib.spllt_hip_set_factor_adjoint_batch(None, op, arena) == -10
    assert lib.spllt_hip_get_factor_adjoint_batch(None, 0, op, 4) == -10
    assert lib.spllt_hip_factor_adjoint_batch(None, op, nnz) == -10
    assert lib.spllt_hip_factor_adjoint_batch_dev(None, vp, nnz) == -10
    assert lib.spllt_hip_batch_adjoint_launches(None) == -10
    assert lib.spllt_hip_release_factor_adjoint_batch(None) == -10
    # null pointer, negative count, short leading dimension, then "no batch yet"
    for fn, a in ((seed, op), (seed_dev, vp)):
        assert fn(f.fkeep, 1, None, a, n, 1.0, 0, 0) == -10 and "null" in f.last_error()
        assert fn(f.fkeep, 1, a, None, n, 1.0, 0, 0) == -10 and "null" in f.last_error()
        assert fn(f.fkeep, -1, a, a, n, 1.0, 0, 0) == -10 and "nvec < 0" in f.last_error()
        assert fn(f.fkeep, 1, a, a, n - 1, 1.0, 0, 0) == -10 and "ld < n" in f.last_error()
        assert fn(f.fkeep, 1, a, a, n, 1.0, 2, 0) == -10 and "accumulate" in f.last_error()
        assert fn(f.fkeep, 1, a, a, n, 1.0, 0, 4) == -10 and "order_flags" in f.last_error()
        assert fn(f.fkeep, 1, a, a, n, 1.0, 0, 0) == -10 and "no batch" in f.last_error()
    for fn, a in ((lib.spllt_hip_factor_adjoint_batch, op), (lib.spllt_hip_factor_adjoint_batch_dev, vp)):
        assert fn(f.fkeep, None, nnz) == -10 and "null" in f.last_error()
        assert fn(f.fkeep, a, nnz - 1) == -10 and "ldout < nnz" in f.last_error()
        assert fn(f.fkeep, a, nnz) == -10 and "no batch" in f.last_error()
    sa = lib.spllt_hip_set_factor_adjoint_batch
    assert sa(f.fkeep, None, arena) == -10 and "null" in f.last_error()
    assert sa(f.fkeep, op, arena - 1) == -10 and "ldarena" in f.last_error()
    assert sa(f.fkeep, op, arena) == -10 and "no batch" in f.last_error()
    ga = lib.spllt_hip_get_factor_adjoint_batch
    assert ga(f.fkeep, 0, None, 4) == -10 and "null" in f.last_error()
    assert ga(f.fkeep, 0, op, -1) == -10 and "count" in f.last_error()
    assert ga(f.fkeep, 0, op, 4) == -10 and "no batch" in f.last_error()
    assert f.last_error().startswith("spllt_hip_get_factor_adjoint_batch: ")
    stride = C.c_int64(5)
    assert lib.spllt_hip_device_factor_adjoint_batch(f.fkeep, C.byref(stride)) is None and stride.value == 0
    assert lib.spllt_hip_device_factor_adjoint_batch(None, C.byref(stride)) is None
    assert lib.spllt_hip_batch_adjoint_launches(f.fkeep) == 0
    assert lib.spllt_hip_release_factor_adjoint_batch(f.fkeep) == 0
    assert (out == 0.0).all()
    for call in (f.factor_adjoint_batch, lambda: f.get_factor_adjoint_batch(0),
                 lambda: f.factor_adjoint_seed_batch(np.zeros((1, n)), np.zeros((1, n))),
                 lambda: f.set_factor_adjoint_batch(np.zeros((1, arena)))):
        with pytest.raises(api.SplltError) as ei:
            call()
        assert ei.value.flag == -10
    with pytest.raises(ValueError):
        f.factor_adjoint_seed_batch(np.zeros((1, n)), np.zeros((1, n + 1)))
    assert f.device_factor_adjoint_batch_ptr() == (None, 0) and f.batch_adjoint_launches() == 0
    f.release_factor_adjoint_batch()
    f.close()


def test_partitioned_handle_is_refused_without_a_device():
    f, val = make_case(matgen.poisson2d(16), nb=16, nemin=8, prune=True, ncpu=2)
    f.set_partition(0, 2)
    out = np.ones(max(f.nnz, f.sym_info()["arena"]) + f.n)
    for call in (f.factor_adjoint_batch, lambda: f.get_factor_adjoint_batch(0),
                 lambda: f.factor_adjoint_seed_batch(np.zeros((1, f.n)), np.zeros((1, f.n))),
                 lambda: f.set_factor_adjoint_batch(np.zeros((1, f.sym_info()["arena"])))):
        with pytest.raises(api.SplltError) as ei:
            call()
        assert ei.value.flag == -98 and "partitioned" in f.last_error()
    assert f.lib.spllt_hip_factor_adjoint_batch(f.fkeep, api._dp(out), f.nnz) == -98
    assert (out == 1.0).all()
    f.close()


@pytest.mark.parametrize("state", capi_ladder.CPU_STATES)
def test_ladder_without_a_device(state):
    c = capi_ladder.Ctx(_lib.load(), False)
    rows = ladder.check_state(c, state, ladder.golden(False))
    assert rows == ladder.ROWS_PER_STATE
