"""CPU tests of the blocked batch solve (include/spllt_hip_batch_solve_many.h): the ABI of the family's own header
and prototype table, its entry ladder in the handle states that need no device (against the recorded rows of the
siblings, batch_solve_many_ladder.py), and the argument checks of the Python wrappers."""
import os
import re

import numpy as np
import pytest

import batch_solve_many_ladder as ladder
import capi_ladder
from spllt_amd import _lib, api, matgen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spllt_hip_batch_solve_many.h")


def _declared():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return set(re.findall(r"\b(spllt_\w+)\s*\(", txt))


def test_every_declared_symbol_is_exported_and_has_a_prototype():
    lib = _lib.load()
    names = _declared()
    assert len(names) == 5 and names == set(_lib.BATCH_SOLVE_MANY_SYMBOLS) == set(_lib._BATCH_SOLVE_MANY)
    assert not names & set(_lib.HIP_SYMBOLS) and not names & set(_lib.PROTOTYPES)
    assert not names & set(_lib.BATCH_MULT_SYMBOLS)
    for s in sorted(names):
        fn = getattr(lib, s)
        assert (fn.restype, list(fn.argtypes)) == (_lib._BATCH_SOLVE_MANY[s][0], _lib._BATCH_SOLVE_MANY[s][1]), s
    # every function of the family takes the handle first and has its rows in the ladder of this family
    assert names == set(ladder.ENTRIES) | {ladder.RELEASE[0]}
    # the header stands alone and says where it is going
    txt = open(HEADER).read()
    assert "<stdint.h>" in txt and 'extern "C"' in txt and "#include \"" not in txt
    assert "folded into" in txt and "spllt_hip.h" in txt


def test_the_older_tables_are_untouched():
    assert set(_lib.PROTOTYPES) == set(_lib.IFACE_SYMBOLS) | set(_lib.HIP_SYMBOLS)
    assert not [s for s in _lib.PROTOTYPES if "many_batch" in s or "blocked" in s]
    assert len(_lib.BATCH_MULT_SYMBOLS) == 6


@pytest.mark.parametrize("state", capi_ladder.CPU_STATES)
def test_ladder_without_a_device(state):
    c = capi_ladder.Ctx(_lib.load(), False)
    rows = ladder.check_state(c, state, ladder.golden(False))
    assert rows == 2 * 6 + 2 + 2 + 2


def test_python_wrappers_reject_wrong_shapes_before_any_library_call():
    n, ptr, row, val = api.csc_lower_1based(matgen.poisson2d(6))
    f = api.Factorization(n, ptr, row, nb=8)

    class _NoCall:
        def __getattr__(self, name):
            raise AssertionError("library call " + name)
    lib, f.lib = f.lib, _NoCall()
    try:
        for X in (np.zeros(n), np.zeros((2, 3, n, 1)), np.zeros((2, n + 1)), np.zeros((2, 3, n - 1))):
            with pytest.raises(ValueError):
                f.solve_many_batch(X)
        with pytest.raises(ValueError):
            f.solve_many_batch_dev(0, -1)
    finally:
        f.lib = lib
    # without a batch the library refuses, by name
    with pytest.raises(api.SplltError) as ei:
        f.solve_many_batch(np.zeros((2, n)))
    assert ei.value.flag == -10 and "spllt_hip_solve_many_batch: no batch" in f.last_error()
    # the switch and the counters need neither a batch nor a device
    assert f.set_batch_blocked_solve(True) is False and f.set_batch_blocked_solve(False) is True
    assert f.solve_many_batch_info() == {"rb": 0, "blocks": 0, "launches": 0, "workspace_bytes": 0}
    f.release_solve_many_batch()
    f.close()
