"""The counters and the ledger of the sparse right-hand-side family against the recorded table (tests/ss_sequence.py):
return code, every field of solve_sparse_info / solve_sparse_batch_info and program("owned") after each call, for the
handle, a batch with a member that is not positive definite, and that batch with its launches split into ranges of
members -- compared exactly with what the commit before the one call sequence (ss_driver.hpp) returned.  The table
runs in one process of its own: the ledger counts bytes, which are only reproducible with the process-wide cache of
released device buffers switched off, and that switch is read once per process."""
import json
import os
import subprocess
import sys

import pytest

import ss_sequence as Q

pytestmark = pytest.mark.gpu


def test_rows_match_the_recorded_table(tmp_path):
    doc = json.load(open(Q.GOLDEN))
    assert doc["recorded_from_commit"]
    want = doc["rows"]
    assert set(want) == {f"{o}|{k}|{v}" for o in Q.OWNERS for k in Q.KS for v in Q.VARIANTS}
    out = str(tmp_path / "rows.json")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(Q.ROOT, "tests", "ss_sequence.py"),
                                                                          "--out", out]
    ran = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=dict(os.environ, **Q.ENV))
    assert ran.returncode == 0, ran.stdout + ran.stderr
    got = json.load(open(out))["rows"]
    assert set(got) == set(want)
    for key in want:
        print(key, got[key])
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong
