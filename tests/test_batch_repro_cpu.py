"""CPU tests of the bit-reproducible batch (include/spllt_hip_batch_repro.h): the interface exists in every layer; the
deterministic batch program ("batch_det_*") holds only what batch_repro.hip implements, reproduces the dense factor
when tests/emulate.py interprets it and does not depend on the handle's engine flags or the environment; the default
batch program is byte for byte what it was; the tables of the batch's reproducible sweep ("batch_rsolve_*") keep the
invariants tests/test_solve_repro_cpu.py checks for "rsolve_*" and solve the system in numpy from a scratch full of
NaN; every case of the GPU tests really has the conflicts the deterministic forms resolve; and the argument errors
that are decided before any device work."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import batch_repro_ladder as ladder
import capi_ladder
import test_solve_repro_cpu as single
from batch_emulate import BatchProgramView, check_batch_program
from batch_repro_emulate import CASES, MODE_BUFFER, MODE_SCATTER, BatchSweepView, DetProgramView, check_det_program, entry_hazard
from emulate import emulate_program
from helpers import dense_arena, lower_mask, make_case, rel_err
from solve_repro_emulate import emulate_solve_repro, tables
from spllt_amd import _lib, api, matgen
from test_factor_batch_cpu import CASES as FACTOR_CASES, GOLD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spllt_hip_batch_repro.h")
NAMES = [c[0] for c in CASES]
DET_NAMES = ["launches", "units", "tiles", "chains", "relpos", "dinv_size", "potrf", "scratch_size", "gather_tiles",
             "gather_items"]
RSOLVE_NAMES = ["fslot", "bfirst", "gptr", "gsrc", "bslot", "frows", "bsize"]
BATCH_NAMES = ["batch_launches", "batch_units", "batch_tiles", "batch_chains", "batch_relpos", "batch_dinv_size",
               "batch_potrf", "batch_scratch_size"]


def _bytes(f, names):
    return [np.asarray(f.program(k)).tobytes() for k in names]


def test_interface_exists_in_every_layer():
    import inspect
    from spllt_amd.torch_ops import SparseCholesky
    lib = _lib.load()
    header = open(HEADER).read()
    names = set(re.findall(r"^int\s+(spllt_hip_\w+)\s*\(", header, re.M))     # (the declarations)
    assert len(names) == 5 and names == set(_lib.BATCH_REPRO_SYMBOLS) == set(_lib._BATCH_REPRO)
    for name in names:
        assert hasattr(lib, name), name
    assert re.search(r"int\s+spllt_hip_solve_repro_batch\(void \*fkeep, int nrhs, double \*x_host, int64_t ldx, int job\);", header)
    assert re.search(r"int\s+spllt_hip_solve_repro_batch_dev\(void \*fkeep, int nrhs, double \*x_dev, int64_t ldx, int job,\s*"
                     r"int pivot_order\);", header)
    assert re.search(r"int\s+spllt_hip_batch_repro_info\(void \*fkeep, int64_t out\[6\]\);", header)
    assert lib.spllt_hip_solve_repro_batch.argtypes[3] is C.c_int64 and lib.spllt_hip_solve_repro_batch_dev.argtypes[3] is C.c_int64
    for m in ("set_batch_reproducible", "solve_reproducible_batch", "solve_reproducible_batch_dev", "batch_repro_info",
              "release_batch_repro"):
        assert callable(getattr(api.Factorization, m)), m
    assert inspect.signature(SparseCholesky.__init__).parameters["batch_reproducible"].default is False
    makefile = open(os.path.join(ROOT, "spllt_amd", "csrc", "Makefile")).read()
    plain = re.search(r"^PLAIN_OBJS = (.*)$", makefile, re.M).group(1).split()
    atomic = re.search(r"^ATOMIC_OBJS = (.*)$", makefile, re.M).group(1).split()
    assert "batch_repro.o" in plain and "batch_repro.o" not in atomic
    for src in ("batch_repro.hip", "rsm_body.hpp", "bu_body.hpp"):
        assert "atomicAdd(" not in open(os.path.join(ROOT, "spllt_amd", "csrc", src)).read(), src


@pytest.mark.parametrize("name", [c[0] for c in FACTOR_CASES])
def test_det_program_is_what_the_kernels_implement_and_reproduces_the_dense_factor(name):
    assert len(GOLD) == 3, GOLD
    A, f, val = next(c[1] for c in FACTOR_CASES if c[0] == name)()
    launches, units, tiles = check_det_program(f)
    kinds = set(launches[launches[:, 3] > 0, 0].tolist())
    assert 4 in kinds and 1 in kinds
    assert (launches[:, 6] == 0).all()                   # single stream
    assert (6 in kinds) == (units["mode"] == MODE_BUFFER).any() == (f.program("batch_det_scratch_size") > 0)
    # the same inter-node work as the default batch program: a BUFFER unit for every SCATTER unit
    assert (units["mode"] == MODE_BUFFER).sum() == (f.program("batch_units")["mode"] == MODE_SCATTER).sum()
    assert f.program("batch_det_dinv_size") == f.program("batch_dinv_size")
    got = emulate_program(DetProgramView(f), val)
    err = rel_err(got, dense_arena(f, A), lower_mask(f))
    print(name, "launches", len(launches), "rel_err", err)
    assert err < 1e-13, err
    f.close()


@pytest.mark.parametrize("name", ["box11-nb64", "fe27-nb768", os.path.basename(GOLD[0]) if GOLD else "none"])
def test_programs_do_not_depend_on_the_engine_flags_or_the_environment(name, monkeypatch):
    make = next(c[1] for c in FACTOR_CASES if c[0] == name)
    names = ["batch_det_" + k for k in DET_NAMES] + ["batch_rsolve_" + k for k in RSOLVE_NAMES] + BATCH_NAMES
    A, f, val = make()
    ref = _bytes(f, names)
    f.close()
    for flags in (2, 4096):
        A, f, val = make(engine_flags=flags)
        assert _bytes(f, names) == ref, flags
        f.close()
    for k, v in (("SPLLT_CHAIN4", "1"), ("SPLLT_SUBTREES", "1"), ("SPLLT_SUBTREE_US", "300"),
                 ("SPLLT_FUSED_PANEL_MAX", "1000000"), ("SPLLT_BUFFER_LEVELS", "2")):
        monkeypatch.setenv(k, v)
    A, f, val = make()
    check_det_program(f)
    check_batch_program(f)
    assert _bytes(f, names) == ref
    f.close()


@pytest.mark.parametrize("name", [c[0] for c in FACTOR_CASES])
def test_default_batch_program_is_untouched_by_the_deterministic_one(name):
    """"batch_*" before and after "batch_det_*" has been built on the same handle, and on a handle that never built it;
    it still holds SCATTER units and no gather"""
    make = next(c[1] for c in FACTOR_CASES if c[0] == name)
    A, f, val = make()
    before = _bytes(f, BATCH_NAMES)
    f.program("batch_det_launches")
    assert _bytes(f, BATCH_NAMES) == before
    assert f.program("batch_scratch_size") == 0 and len(f.program("batch_potrf")) == 0
    launches, units, _ = check_batch_program(f)
    assert 6 not in set(launches[:, 0].tolist()) and (units["mode"] != MODE_BUFFER).all()
    got = emulate_program(BatchProgramView(f), val)
    assert rel_err(got, dense_arena(f, A), lower_mask(f)) < 1e-13
    with pytest.raises(KeyError):
        f.program("batch_gather_tiles")
    with pytest.raises(KeyError):
        f.program("batch_det_panels")
    with pytest.raises(KeyError):
        f.program("batch_rsolve_units")
    f.close()


@functools.lru_cache(maxsize=None)
def _case(name):
    _, gen, nb, nemin = next(c for c in CASES if c[0] == name)
    A = gen()
    f, val = make_case(A, nb=nb, nemin=nemin)
    prog = {k: f.program(k) for k in ("solve_units", "solve_list", "solve_tiles", "solve_fwd", "solve_bwd")}
    return f, prog, tables(BatchSweepView(f)), A, val


@pytest.mark.parametrize("name", NAMES)
def test_batch_rsolve_table_invariants(name, monkeypatch):
    """the invariants of tests/test_solve_repro_cpu.py, by its own test, on the batch's tables: gsrc a permutation of
    the slots, sources ascending, the writer launch before the reader launch, the backward ranges disjoint"""
    f, prog, t, _A, _val = _case(name)
    monkeypatch.setattr(single, "_case", lambda _name: (f, prog, t))
    single.test_table_invariants(name)


@pytest.mark.parametrize("name", NAMES)
def test_batch_rsolve_tables_do_not_follow_the_handles_panel_width(name):
    """the batch's solve program has pw = cb = 64 whatever the handle's"""
    f, _prog, t, A, _val = _case(name)
    _, gen, nb, nemin = next(c for c in CASES if c[0] == name)
    f8, _ = make_case(A, nb=nb, nemin=nemin, panel_width=16)
    for k in RSOLVE_NAMES:
        assert np.array_equal(f8.program("batch_rsolve_" + k), t[k]), k
    f8.close()


@pytest.mark.parametrize("name", NAMES)
def test_numpy_sweep_from_a_poisoned_scratch_equals_the_dense_solve(name):
    f, _prog, _t, A, _val = _case(name)
    L = dense_arena(f, A)
    n = f.n
    X = np.random.default_rng(0).standard_normal((n, 3))
    B = A @ X
    pos = f.sym("order")
    Y = np.zeros((3, n))
    Y[:, pos] = B.T
    emulate_solve_repro(BatchSweepView(f), L, Y)
    assert np.isfinite(Y).all()          # (the scratch starts as NaN: every slot read was written first)
    np.testing.assert_allclose(Y[:, pos].T, X, rtol=0, atol=1e-9)
    Y2 = np.zeros((3, n))
    Y2[:, pos] = B.T
    emulate_solve_repro(BatchSweepView(f), L, Y2, job=1)
    emulate_solve_repro(BatchSweepView(f), L, Y2, job=2)
    np.testing.assert_allclose(Y2, Y, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("name", NAMES)
def test_every_gpu_case_has_the_hazards(name):
    """not vacuous: two distinct units write one destination entry in one launch of the default program; a row has two
    entries in its gather list; a block column has two strips"""
    f, prog, t, _A, _val = _case(name)
    assert entry_hazard(f), "no destination entry receives from two units of one launch"
    assert int(np.diff(t["gptr"]).max()) >= 2, "no row has two entries in its gather list"
    strips = np.bincount(prog["solve_tiles"]["unit"], minlength=len(prog["solve_units"])).max()
    assert strips >= 2, "no block column has two strips"


def test_the_replaced_case_lacks_the_backward_hazard():
    """why p2d12-nb8 of tests/test_batch_mult_gpu.py is not among the cases"""
    f, _val = make_case(matgen.poisson2d(12), nb=8, nemin=4)
    tiles = f.program("solve_tiles")
    assert np.bincount(tiles["unit"]).max() == 1
    f.close()


def test_argument_errors_and_the_switch_on_an_analysed_handle():
    f, val = make_case(matgen.poisson2d(8), nb=8, nemin=4)
    n = f.n
    x = np.ones(3 * 2 * (n + 1))
    xp = C.c_void_p(x.ctypes.data)
    for nrhs, ptr, ldx, job, word in [(-1, xp, n, 0, "nrhs"), (2, xp, n - 1, 0, "ldx"), (2, xp, n, 3, "job"),
                                      (2, xp, n, -1, "job"), (2, None, n, 0, "null")]:
        assert f.lib.spllt_hip_solve_repro_batch(f.fkeep, nrhs, ptr, ldx, job) == -10
        assert word in f.last_error(), f.last_error()
        assert f.lib.spllt_hip_solve_repro_batch_dev(f.fkeep, nrhs, ptr, ldx, job, 0) == -10
        assert word in f.last_error(), f.last_error()
    assert f.lib.spllt_hip_solve_repro_batch(f.fkeep, 2, xp, n + 1, 0) == -10      # good arguments, no batch yet
    assert "no batch" in f.last_error() and (x == 1.0).all()
    assert f.lib.spllt_hip_solve_repro_batch(None, 2, xp, n, 0) == -10
    # the switch lives on the handle and needs no device
    assert f.lib.spllt_hip_set_batch_reproducible(f.fkeep, 1) == 0
    assert f.lib.spllt_hip_set_batch_reproducible(f.fkeep, 1) == 1
    assert f.batch_repro_info() == dict(on=1, deterministic_factor=0, factor_launches=0, sweep_rb=0,
                                        factor_scratch_bytes=0, sweep_scratch_bytes=0)
    assert f.set_batch_reproducible(False) is True and f.set_batch_reproducible(False) is False
    assert f.batch_repro_info()["on"] == 0
    assert f.lib.spllt_hip_set_batch_reproducible(None, 1) == -10
    assert f.lib.spllt_hip_batch_repro_info(None, None) == -10 and f.lib.spllt_hip_batch_repro_info(f.fkeep, None) == -10
    assert f.lib.spllt_hip_release_batch_repro(f.fkeep) == 0
    assert f.lib.spllt_hip_release_batch_repro(None) == -10
    assert f.lib.spllt_hip_debug(b"batch_repro_poison=1") == 0 and f.lib.spllt_hip_debug(b"batch_repro_poison=0") == 0
    assert f.lib.spllt_hip_debug(b"batch_repro_poison=2") == -1
    f.close()


def test_partitioned_handle_refuses_the_switch():
    f, val = make_case(matgen.poisson2d(16), nb=16, nemin=8, prune=True, ncpu=2)
    f.set_partition(0, 2)
    assert f.lib.spllt_hip_set_batch_reproducible(f.fkeep, 1) == -98 and "partitioned" in f.last_error()
    assert f.lib.spllt_hip_set_batch_reproducible(f.fkeep, 0) == 0
    assert f.batch_repro_info()["on"] == 0
    x = np.ones(2 * f.n)
    assert f.lib.spllt_hip_solve_repro_batch(f.fkeep, 1, C.c_void_p(x.ctypes.data), f.n, 0) == -98
    f.close()


@pytest.mark.parametrize("state", capi_ladder.CPU_STATES)
def test_ladder_without_a_device(state):
    names = set(re.findall(r"^int\s+(spllt_hip_\w+)\s*\(", open(HEADER).read(), re.M))
    assert names == set(ladder.ENTRIES) | {ladder.RELEASE[0]}     # every function of the family has its rows
    c = capi_ladder.Ctx(_lib.load(), False)
    assert ladder.check_state(c, state, ladder.golden(False)) == ladder.ROWS


def test_torch_keyword_without_a_device(monkeypatch):
    from spllt_amd.torch_ops import SparseCholesky
    calls = []
    real = api.Factorization.set_batch_reproducible
    monkeypatch.setattr(api.Factorization, "set_batch_reproducible", lambda self, on: (calls.append(on), real(self, on))[1])
    A = matgen.poisson2d(8)
    off = SparseCholesky(A, nb=8)
    assert calls == [] and off.batch_reproducible is False and off.f.batch_repro_info()["on"] == 0
    on = SparseCholesky(A, nb=8, batch_reproducible=True)
    assert calls == [True] and on.batch_reproducible is True and on.f.batch_repro_info()["on"] == 1
    only = SparseCholesky(A, nb=8, reproducible=True)
    with pytest.raises(NotImplementedError, match="batch_reproducible=True"):
        only.logdet_batch(None)
