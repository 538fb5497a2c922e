"""CPU tests of the product and the refined solves of a batch (include/spllt_hip_batch_refine.h): the ABI of the
family's own header and prototype table, its entry ladder in the handle states that need no device (against the
recorded rows of the siblings, batch_refine_ladder.py), and the argument checks of the Python wrappers."""
import os
import re

import numpy as np
import pytest

import batch_refine_ladder as ladder
import capi_ladder
from spllt_amd import _lib, api, matgen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spllt_hip_batch_refine.h")


def _declared():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return set(re.findall(r"\b(spllt_\w+)\s*\(", txt))


def test_every_declared_symbol_is_exported_and_has_a_prototype():
    lib = _lib.load()
    names = _declared()
    assert len(names) == 6 and names == set(_lib.BATCH_REFINE_SYMBOLS) == set(_lib._BATCH_REFINE)
    assert not names & set(_lib.HIP_SYMBOLS) and not names & set(_lib.PROTOTYPES)
    assert not names & (set(_lib.BATCH_MULT_SYMBOLS) | set(_lib.BATCH_SOLVE_MANY_SYMBOLS) | set(_lib.BATCH_ADJOINT_SYMBOLS))
    for s in sorted(names):
        fn = getattr(lib, s)
        assert (fn.restype, list(fn.argtypes)) == (_lib._BATCH_REFINE[s][0], _lib._BATCH_REFINE[s][1]), s
    # every function of the family takes the handle first and has its rows in the ladder of this family
    assert names == set(ladder.ENTRIES) | {ladder.RELEASE[0]}
    # the prototypes have the arguments of the header, one by one
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for s in sorted(names):
        params = re.search(r"\b" + s + r"\s*\(([^)]*)\)", txt).group(1).split(",")
        assert len(params) == len(_lib._BATCH_REFINE[s][1]), (s, params)
    # the header stands alone and says where it is going
    txt = open(HEADER).read()
    assert "<stdint.h>" in txt and 'extern "C"' in txt and "#include \"" not in txt
    assert "folded into" in txt and "spllt_hip.h" in txt


def test_the_older_tables_are_untouched():
    assert set(_lib.PROTOTYPES) == set(_lib.IFACE_SYMBOLS) | set(_lib.HIP_SYMBOLS)
    assert not [s for s in _lib.PROTOTYPES if "refined_batch" in s or "matvec_batch" in s or "refine_batch" in s]
    assert len(_lib.BATCH_MULT_SYMBOLS) == 6 and len(_lib.BATCH_SOLVE_MANY_SYMBOLS) == 5 and len(_lib.BATCH_ADJOINT_SYMBOLS) == 9


@pytest.mark.parametrize("state", capi_ladder.CPU_STATES)
def test_ladder_without_a_device(state):
    c = capi_ladder.Ctx(_lib.load(), False)
    rows = ladder.check_state(c, state, ladder.golden(False))
    # (the accepted product on an analysed handle creates the engine: as for its sibling, no such row without a GPU)
    assert rows == ladder.ROWS - (2 if state == "analysed" else 0)


def test_partitioned_handle_returns_unimplemented():
    c = capi_ladder.Ctx(_lib.load(), False)
    h = c.handle("partitioned")
    try:
        for name in ("spllt_hip_matvec_batch", "spllt_hip_matvec_batch_dev", "spllt_hip_solve_refined_batch",
                     "spllt_hip_solve_refined_batch_dev"):
            rc, err = ladder.call(c, name, h[1], {})
            assert rc == -98 and err == name + ": not available on a partitioned (multi-GPU) handle", (name, rc, err)
    finally:
        c.free(h)


def test_python_wrappers_reject_wrong_shapes_before_any_library_call():
    n, ptr, row, val = api.csc_lower_1based(matgen.poisson2d(6))
    f = api.Factorization(n, ptr, row, nb=8)
    nnz = len(val)
    vals = np.stack([val, 2.0 * val])

    class _NoCall:
        def __getattr__(self, name):
            raise AssertionError("library call " + name)
    lib, f.lib = f.lib, _NoCall()
    try:
        for X in (np.zeros(n), np.zeros((2, 3, n, 1)), np.zeros((2, n + 1)), np.zeros((2, 3, n - 1)), np.zeros((3, n))):
            with pytest.raises(ValueError):
                f.matvec_batch(vals, X)
        for V in (val, np.zeros((2, nnz + 1)), np.zeros((2, 1, nnz))):
            with pytest.raises(ValueError):
                f.matvec_batch(V, np.zeros((2, n)))
            with pytest.raises(ValueError):
                f.solve_refined_batch(V, np.zeros((2, n)))
        with pytest.raises(api.SplltError):
            f.solve_refined_batch(vals, np.zeros((2, n)), method="gmres")
        with pytest.raises(ValueError):
            f.solve_refined_batch_dev(0, 0, -1)
    finally:
        f.lib = lib
    for X in (np.zeros(n), np.zeros((2, n + 1)), np.zeros((3, n))):
        with pytest.raises(ValueError):
            f.solve_refined_batch(vals, X)
    # without a batch the library refuses, by name
    with pytest.raises(api.SplltError) as ei:
        f.solve_refined_batch(vals, np.zeros((2, n)))
    assert ei.value.flag == -10 and "spllt_hip_solve_refined_batch: no batch" in f.last_error()
    assert f.refine_status == -10
    # the counters and the release need neither a batch nor a device
    assert f.solve_refined_batch_info() == {"width": 0, "passes": 0, "launches": 0, "workspace_bytes": 0}
    f.release_refine_batch()
    f.close()
