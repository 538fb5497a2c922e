"""CPU tests of the hard linear constraints of a batch (include/spllt_hip_constrain_batch.h): the dense emulation per
member against the KKT system, the ABI of the family's own header and prototype table, its entry ladder in the handle
states that need no device (against the recorded rows of the siblings, constrain_batch_ladder.py), and the argument
checks of the Python wrappers."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import capi_ladder
import constrain_batch_emulate as bemu
import constrain_batch_ladder as ladder
import constrain_emulate as emu
from spllt_amd import _lib, api, matgen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spllt_hip_constrain_batch.h")


@pytest.mark.parametrize("name,k", bemu.CASES)
def test_emulated_members_solve_their_kkt_systems(name, k):
    bc = bemu.batch(name, k, 5)          # (members 0 .. 4: those of the GPU tests, the five-member batch included)
    n = bc.n
    rng = np.random.default_rng(k)
    B = rng.standard_normal((5, 5, n))
    # the rows are far from dependent in every member: with a smallest relative pivot of S_b above 1e-3 the reference
    # itself loses at most three of its sixteen digits (and the library refuses below 2^-26 only)
    assert bc.min_relative_pivot().min() >= 1e-3
    for e in (None, rng.standard_normal(k), rng.standard_normal((5, 5, k))):
        x, lam = bc.solve_constrained(B, e)
        xk, lk = bc.kkt_solve(B, e)
        np.testing.assert_allclose(x, xk, rtol=1e-12, atol=1e-12)      # (the project's bar between two solves)
        np.testing.assert_allclose(lam, lk, rtol=1e-12, atol=1e-12)
        for b, E in enumerate(bc.targets(e, 5)):
            assert np.abs(bc.C @ x[b].T - E).max() <= emu.residual_bar(bc.C, x[b], None if e is None else E)
    # the members differ (one C, five matrices), and member b is constrain_emulate on A_b alone
    assert np.abs(x[0] - x[1]).max() > 1e-3 * np.abs(x[0]).max()
    one = emu.Constraints(bemu.matrix(name).member(2)[0], bc.C).solve_constrained(B[2].T, None)[0]
    assert np.array_equal(one.T, bc.solve_constrained(B, None)[0][2])


@pytest.mark.parametrize("name,k", bemu.CASES)
def test_emulated_variances_are_the_diagonals_of_the_conditional_covariances(name, k):
    bc = bemu.batch(name, k)
    v, d = bc.variances(), bc.conditional_cov_diag()
    for b, m in enumerate(bc.members):
        assert np.abs(v[b] - d[b]).max() <= 1e-11 * np.abs(np.linalg.inv(m.A)).max()
    assert (v > 0).all()


def _declared():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return set(re.findall(r"\b(spllt_\w+)\s*\(", txt))


def test_every_declared_symbol_is_exported_and_has_a_prototype():
    lib = _lib.load()
    names = _declared()
    assert len(names) == 11 and names == set(_lib.CONSTRAIN_BATCH_SYMBOLS) == set(_lib._CONSTRAIN_BATCH)
    assert not names & set(_lib.HIP_SYMBOLS) and not names & set(_lib.PROTOTYPES)
    assert not names & (set(_lib.BATCH_MULT_SYMBOLS) | set(_lib.BATCH_SOLVE_MANY_SYMBOLS) | set(_lib.BATCH_ADJOINT_SYMBOLS) |
                        set(_lib.BATCH_REFINE_SYMBOLS) | set(_lib.CONSTRAIN_SYMBOLS))
    for s in sorted(names):
        fn = getattr(lib, s)
        assert (fn.restype, list(fn.argtypes)) == (_lib._CONSTRAIN_BATCH[s][0], _lib._CONSTRAIN_BATCH[s][1]), s
    # every function of the family takes the handle first and has its rows in the ladder of this family
    assert names == set(ladder.ENTRIES) | {ladder.RELEASE[0]}
    # the prototypes have the arguments of the header, one by one: the count, and the C type of each against its ctype
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    ctype = {"int": C.c_int, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32}
    for s in sorted(names):
        params = [p.strip() for p in re.search(r"\b" + s + r"\s*\(([^)]*)\)", txt).group(1).split(",")]
        argtypes = _lib._CONSTRAIN_BATCH[s][1]
        assert len(params) == len(argtypes), (s, params)
        assert re.match(r"void\s*\*\s*fkeep$", params[0]), (s, params[0])
        for p, t in zip(params, argtypes):
            if "*" in p or "[" in p:       # a pointer: void* (integers for device pointers) or a typed pointer
                assert t is C.c_void_p or issubclass(t, C._Pointer), (s, p, t)
            else:
                assert t is ctype[p.split()[-2]], (s, p, t)
    # the header stands alone; spllt_hip.h and the single handle's header do not know the family
    txt = open(HEADER).read()
    assert "<stdint.h>" in txt and 'extern "C"' in txt and "#include \"" not in txt
    assert "constrain" not in open(os.path.join(ROOT, "include", "spllt_hip.h")).read()
    assert "_batch" not in re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spllt_hip_constrain.h")).read(),
                                  flags=re.S)


@pytest.mark.parametrize("state", capi_ladder.CPU_STATES)
def test_ladder_without_a_device(state):
    c = capi_ladder.Ctx(_lib.load(), False)
    assert ladder.check_state(c, state, ladder.golden(False)) == ladder.ROWS


def test_partitioned_handle_returns_unimplemented():
    c = capi_ladder.Ctx(_lib.load(), False)
    h = c.handle("partitioned")
    try:
        for name in ladder.ENTRIES:
            if name == "spllt_hip_constraints_batch_info":
                continue
            rc, err = ladder.call(c, name, h[1], {})
            assert rc == -98 and err == f"{name}: not available on a partitioned (multi-GPU) handle", (name, rc, err)
        assert c.lib.spllt_hip_release_constraints_batch(h[1]) == 0
    finally:
        c.free(h)


def test_argument_order_of_the_ladder_without_a_device():
    """what no device is needed for: the arguments are named before the handle's state is looked at, in the order of
    the header; then "no batch yet"."""
    c = capi_ladder.Ctx(_lib.load(), False)
    h = c.handle("analysed")
    try:
        for changes, word in (({1: None}, "null"), ({0: -1}, "k < 0"), ({0: 65}, "k > 64"), ({2: c.n - 1}, "ldc < n")):
            rc, err = ladder.call(c, "spllt_hip_set_constraints_batch", h[1], changes)
            assert rc == -10 and word in err, (changes, rc, err)
        # k = 0 needs no rows; like every other variant it is refused on a handle without a batch
        rc, err = ladder.call(c, "spllt_hip_set_constraints_batch", h[1], {0: 0, 1: None})
        assert rc == -10 and "no batch has been factorized" in err
        # the sampler's own arguments, in the words of spllt_hip_sample_batch
        for changes, word in (({6: 2}, "stream_step is not 0"), ({7: c.H(1), 8: c.n - 1}, "ldmean is neither 0")):
            rc, err = ladder.call(c, "spllt_hip_sample_constrained_batch", h[1], changes)
            assert rc == -10 and word in err, (changes, rc, err)
        out, stat = np.full(4, 7, dtype=np.int64), np.full(2, 7.0)
        i64p = out.ctypes.data_as(C.POINTER(C.c_int64))
        assert c.lib.spllt_hip_constraints_batch_info(h[1], i64p, api._dp(stat), 2) == 0
        assert not out.any() and (stat == 7.0).all()      # (no batch: no member's row is written)
        assert c.lib.spllt_hip_constraints_batch_info(h[1], i64p, None, 0) == 0           # stat may be null
        assert c.lib.spllt_hip_constraints_batch_info(h[1], i64p, api._dp(stat), 1) == -10   # ldstat >= 2
    finally:
        c.free(h)


def test_python_wrappers_reject_wrong_shapes_before_any_library_call():
    n, ptr, row, val = api.csc_lower_1based(matgen.poisson2d(6))
    f = api.Factorization(n, ptr, row, nb=8)
    with pytest.raises(ValueError):
        f.set_constraints_batch(np.zeros((2, n + 1)))
    with pytest.raises(ValueError):
        f.constrain_batch(np.zeros(n))                     # (B, n) or (B, nvec, n)
    with pytest.raises(ValueError):
        f.constrain_batch(np.zeros((2, n + 1)))
    with pytest.raises(ValueError):
        f.solve_constrained_batch(np.zeros((2, 3, n)), e=np.zeros(3))     # k = 0 here: (0,) or (2, 3, 0)
    with pytest.raises(ValueError):
        f.solve_constrained_batch(np.zeros((2, 3, n)), e=np.zeros((2, 3, 1)))
    with pytest.raises(ValueError):
        f.sample_constrained_batch(2, mean=np.zeros(n - 1))
    with pytest.raises(ValueError):
        f.sample_constrained_batch(2, e=np.zeros(2))
    with pytest.raises(ValueError):
        f.sample_constrained_batch(-1)
    assert f.last_error() == ""                            # (no library call was refused: none was made)
    # without a batch the library refuses, by name
    with pytest.raises(api.SplltError) as ei:
        f.set_constraints_batch(np.ones((1, n)))
    assert ei.value.flag == -10 and "spllt_hip_set_constraints_batch: no batch has been factorized" in f.last_error()
    info = f.constraints_batch_info()
    assert {k: v for k, v in info.items() if np.ndim(v) == 0} == {"k": 0, "rebuilds": 0, "device_bytes": 0, "launches": 0}
    assert info["log_det_s"].size == 0 and info["min_relative_pivot"].size == 0
    f.release_constraints_batch()
    f.close()
