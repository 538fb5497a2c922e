"""CPU tests of the hard linear constraints (include/spllt_hip_constrain.h): the dense emulation against the KKT
system, the ABI of the family's own header and prototype table, its entry ladder in the handle states that need no
device (against the recorded rows of the siblings, constrain_ladder.py), and the argument checks of the Python
wrappers."""
import os
import re

import numpy as np
import pytest

import capi_ladder
import constrain_emulate as emu
import constrain_ladder as ladder
from spllt_amd import _lib, api, matgen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spllt_hip_constrain.h")
CASES = [(m, k) for m in ("p2d8", "p2d12", "p3d5") for k in (1, 3, 16, 17, 33, 64) if not (m == "p2d8" and k == 64)]


@pytest.mark.parametrize("name,k", CASES)
def test_emulated_correction_solves_the_kkt_system(name, k):
    A = emu.case_matrix(name)[0].toarray()
    n = A.shape[0]
    con = emu.Constraints(A, emu.constraint_rows(k, n))
    rng = np.random.default_rng(k)
    B = rng.standard_normal((n, 5))
    # the rows are far from dependent: with a smallest relative pivot of S above 1e-3 the reference itself loses at
    # most three of its sixteen digits, 2e-13 against the bar of 1e-12 (and the library refuses below 2^-26 only)
    assert con.min_relative_pivot() >= 1e-3
    for e in (None, rng.standard_normal(k), rng.standard_normal((k, 5))):
        x, lam = con.solve_constrained(B, e)
        xk, lk = con.kkt_solve(B, e)
        np.testing.assert_allclose(x, xk, rtol=1e-12, atol=1e-12)      # (the project's bar between two solves)
        np.testing.assert_allclose(lam, lk, rtol=1e-12, atol=1e-12)
        E = con.targets(e, 5)
        assert np.abs(con.C @ x - E).max() <= emu.residual_bar(con.C, x, e)
    # one vector, as a vector
    x1, l1 = con.correct(np.linalg.solve(A, B[:, 0]))
    assert x1.shape == (n,) and l1.shape == (k,) and np.array_equal(x1, con.solve_constrained(B[:, :1])[0][:, 0])


@pytest.mark.parametrize("name,k", CASES)
def test_emulated_variances_are_the_diagonal_of_the_conditional_covariance(name, k):
    A = emu.case_matrix(name)[0].toarray()
    con = emu.Constraints(A, emu.constraint_rows(k, A.shape[0]))
    cov = con.conditional_cov()
    v = con.variances()
    assert np.abs(v - np.diag(cov)).max() <= 1e-11 * np.abs(np.linalg.inv(A)).max()
    assert (v > 0).all()
    # the conditional covariance has C in its null space, and log det S is that of the Cholesky factor
    assert np.abs(con.C @ cov).max() <= 1e-11 * np.abs(con.C).sum(axis=1).max() * np.abs(cov).max()
    assert abs(con.log_det_s() - 2.0 * np.log(np.diag(con.G)).sum()) <= 1e-12 * max(1.0, abs(con.log_det_s()))


def _declared():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return set(re.findall(r"\b(spllt_\w+)\s*\(", txt))


def test_every_declared_symbol_is_exported_and_has_a_prototype():
    lib = _lib.load()
    names = _declared()
    assert len(names) == 11 and names == set(_lib.CONSTRAIN_SYMBOLS) == set(_lib._CONSTRAIN)
    assert not names & set(_lib.HIP_SYMBOLS) and not names & set(_lib.PROTOTYPES)
    assert not names & (set(_lib.BATCH_MULT_SYMBOLS) | set(_lib.BATCH_SOLVE_MANY_SYMBOLS) | set(_lib.BATCH_ADJOINT_SYMBOLS) |
                        set(_lib.BATCH_REFINE_SYMBOLS))
    for s in sorted(names):
        fn = getattr(lib, s)
        assert (fn.restype, list(fn.argtypes)) == (_lib._CONSTRAIN[s][0], _lib._CONSTRAIN[s][1]), s
    # every function of the family takes the handle first and has its rows in the ladder of this family
    assert names == set(ladder.ENTRIES) | {ladder.RELEASE[0]}
    # the prototypes have the arguments of the header, one by one
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for s in sorted(names):
        params = re.search(r"\b" + s + r"\s*\(([^)]*)\)", txt).group(1).split(",")
        assert len(params) == len(_lib._CONSTRAIN[s][1]), (s, params)
        assert re.match(r"\s*void\s*\*\s*fkeep\s*$", params[0]), (s, params[0])
    # the header stands alone, and spllt_hip.h does not know the family
    txt = open(HEADER).read()
    assert "<stdint.h>" in txt and 'extern "C"' in txt and "#include \"" not in txt
    assert "constrain" not in open(os.path.join(ROOT, "include", "spllt_hip.h")).read()


@pytest.mark.parametrize("state", capi_ladder.CPU_STATES)
def test_ladder_without_a_device(state):
    c = capi_ladder.Ctx(_lib.load(), False)
    assert ladder.check_state(c, state, ladder.golden(False)) == ladder.ROWS


def test_partitioned_handle_returns_unimplemented():
    c = capi_ladder.Ctx(_lib.load(), False)
    h = c.handle("partitioned")
    try:
        for name in ladder.ENTRIES:
            if name == "spllt_hip_constraints_info":
                continue
            word = "factor" if name == "spllt_hip_inverse_diag_constrained" else "handle"     # (the sibling's word)
            rc, err = ladder.call(c, name, h[1], {})
            assert rc == -98 and err == f"{name}: not available on a partitioned (multi-GPU) {word}", (name, rc, err)
    finally:
        c.free(h)


def test_argument_order_of_the_ladder_without_a_device():
    """what no device is needed for: k and ldc are named before the handle's state is looked at"""
    c = capi_ladder.Ctx(_lib.load(), False)
    h = c.handle("analysed")
    try:
        for changes, word in (({1: None}, "null"), ({0: -1}, "k < 0"), ({0: 65}, "k > 64"), ({2: c.n - 1}, "ldc < n")):
            rc, err = ladder.call(c, "spllt_hip_set_constraints", h[1], changes)
            assert rc == -10 and word in err, (changes, rc, err)
        # k = 0 needs no rows; like every other variant it is refused on a handle without a factor
        rc, err = ladder.call(c, "spllt_hip_set_constraints", h[1], {0: 0, 1: None})
        assert rc == -10 and "nothing has been factorized" in err
        out, stat = np.full(4, 7, dtype=np.int64), np.full(2, 7.0)
        assert c.lib.spllt_hip_constraints_info(h[1], out.ctypes.data_as(capi_ladder.C.POINTER(capi_ladder.C.c_int64)),
                                                api._dp(stat)) == 0
        assert not out.any() and not stat.any()
    finally:
        c.free(h)


def test_python_wrappers_reject_wrong_shapes_before_any_library_call():
    n, ptr, row, val = api.csc_lower_1based(matgen.poisson2d(6))
    f = api.Factorization(n, ptr, row, nb=8)
    with pytest.raises(ValueError):
        f.set_constraints(np.zeros((2, n + 1)))
    with pytest.raises(ValueError):
        f.constrain(np.zeros(n + 1))
    with pytest.raises(ValueError):
        f.solve_constrained(np.zeros((n, 2)), e=np.zeros(3))
    with pytest.raises(ValueError):
        f.sample_constrained(2, mean=np.zeros(n - 1))
    # without a factorization the library refuses, by name
    with pytest.raises(api.SplltError) as ei:
        f.set_constraints(np.ones((1, n)))
    assert ei.value.flag == -10 and "spllt_hip_set_constraints: nothing has been factorized" in f.last_error()
    assert f.constraints_info() == {"k": 0, "rebuilds": 0, "device_bytes": 0, "launches": 0, "log_det_s": 0.0,
                                    "min_relative_pivot": 0.0}
    f.release_constraints()
    f.close()
