"""The entry ladder of the C boundary without a GPU (tests/capi_ladder.py): every row that returns before an engine
is created or a device is touched, on a null handle, a handle whose analysis failed, an analysed handle and a
partitioned one (rank 0 of 2), compared exactly with the recorded table."""
import json

import capi_ladder as L
from spllt_amd import _lib


def test_rows_match_the_recorded_table():
    want = L.unpack(json.load(open(L.GOLDEN[False])))
    got = L.run_table(_lib.load(), gpu=False)
    assert set(got) == set(want)
    wrong = {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert not wrong, wrong


def test_every_entry_point_with_a_handle_has_a_row():
    """a new spllt_hip_* function that takes an fkeep cannot skip the table (CPU or GPU file)"""
    names = L.takes_fkeep()
    assert names and names <= set(_lib.HIP_SYMBOLS)
    rows = set()
    for gpu in (False, True):
        rows |= {k.split("|")[0] for k in L.unpack(json.load(open(L.GOLDEN[gpu])))}
    assert rows == set(L.ENTRIES)
    assert not names - rows, sorted(names - rows)
