"""CPU tests of the batched factor products and samplers (include/spllt_hip_batch_mult.h): the ABI of the family's
own header and prototype table, its entry ladder in the handle states that need no device (against the recorded
rows of the siblings, batch_mult_ladder.py), the numpy definition of the noise with a stream word, and the
argument checks of the Python wrappers."""
import os
import re

import numpy as np
import pytest

import batch_mult_ladder as ladder
import capi_ladder
from batch_mult_ladder import noise_reference as _noise
from factor_mult_emulate import white_noise_reference
from spllt_amd import _lib, api, matgen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    txt = open(os.path.join(ROOT, "include", "spllt_hip_batch_mult.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(spllt_\w+)\s*\(", txt))


def test_every_declared_symbol_is_exported_and_has_a_prototype():
    lib = _lib.load()
    names = _declared()
    assert len(names) == 6 and names == set(_lib.BATCH_MULT_SYMBOLS) == set(_lib._BATCH_MULT)
    assert not names & set(_lib.HIP_SYMBOLS) and not names & set(_lib.PROTOTYPES)
    for s in sorted(names):
        fn = getattr(lib, s)
        assert (fn.restype, list(fn.argtypes)) == (_lib._BATCH_MULT[s][0], _lib._BATCH_MULT[s][1]), s
    # every function of the family takes the handle first and has its rows in the ladder of this family
    assert names == set(ladder.ENTRIES) | {ladder.RELEASE[0]}
    # the header stands alone and says where it is going
    txt = open(os.path.join(ROOT, "include", "spllt_hip_batch_mult.h")).read()
    assert "<stdint.h>" in txt and 'extern "C"' in txt and "#include \"" not in txt
    assert "folded into" in txt and "spllt_hip.h" in txt


def test_the_older_tables_are_untouched():
    assert set(_lib.PROTOTYPES) == set(_lib.IFACE_SYMBOLS) | set(_lib.HIP_SYMBOLS)
    assert not [s for s in _lib.PROTOTYPES if "mult_batch" in s or "sample_batch" in s or "noise_batch" in s]


@pytest.mark.parametrize("state", capi_ladder.CPU_STATES)
def test_ladder_without_a_device(state):
    c = capi_ladder.Ctx(_lib.load(), False)
    rows = ladder.check_state(c, state, ladder.golden(False))
    assert rows >= 5 * 5 + 1


def test_noise_reference_with_a_stream_word():
    for seed, first in ((7, 0), ((1 << 40) + 12345, (1 << 33) + 1)):
        z0 = _noise(50, 4, seed, 0, first)
        assert np.array_equal(z0, white_noise_reference(50, 4, seed, first))
        z1 = _noise(50, 4, seed, 1, first)
        assert np.isfinite(z1).all() and not np.array_equal(z1, z0)
        assert not np.array_equal(_noise(50, 4, seed, 2, first), z1)
    z = _noise(4000, 8, 3, 5)              # a stream is standard normal noise like stream 0
    assert abs(z.mean()) < 0.03 and abs(z.std() - 1.0) < 0.03


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
                f.factor_mult_batch(X)
        for m in (np.zeros(n + 1), np.zeros((2, n + 1)), np.zeros((2, 2, n))):
            with pytest.raises(ValueError):
                f.sample_batch(2, mean=m)
        with pytest.raises(ValueError):
            f.sample_batch(-1)
        with pytest.raises(ValueError):
            f.white_noise_batch(-1, seed=0)
    finally:
        f.lib = lib
    # without a batch the library refuses, by name
    with pytest.raises(api.SplltError) as ei:
        f.factor_mult_batch(np.zeros((2, n)))
    assert ei.value.flag == -10 and "spllt_hip_factor_mult_batch: no batch" in f.last_error()
    with pytest.raises(api.SplltError) as ei:
        f.sample_batch(2, mean=np.zeros(n))
    assert ei.value.flag == -10 and "spllt_hip_sample_batch: no batch" in f.last_error()
    f.close()
