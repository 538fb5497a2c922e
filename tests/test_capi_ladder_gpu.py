"""The entry ladder of the C boundary on the GPU (tests/capi_ladder.py): every entry point in the states a handle
goes through -- engine without a factor, factored, not positive definite, factor lost to a failed downdate, a batch
with a failed member, inverses valid and stale, the adjoint seeded and swept -- compared exactly with the recorded
table."""
import json

import pytest

import capi_ladder as L
from spllt_amd import _lib

pytestmark = pytest.mark.gpu


def test_rows_match_the_recorded_table():
    want = L.unpack(json.load(open(L.GOLDEN[True])))
    got = L.run_table(_lib.load(), gpu=True)
    assert set(got) == set(want)
    wrong = {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert not wrong, wrong
