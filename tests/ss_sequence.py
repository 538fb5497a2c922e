"""The recorded counters of the sparse right-hand-side family: solve_sparse / gram of a handle and
solve_sparse_batch / gram_batch of a batch (spllt_amd/csrc/ss_driver.hpp and its two backends in engine_solve.cpp).

A row is one call -> [return code, the fields of the info reader, program("owned") after the call].  All of it is
computed on the host and deterministic (the results themselves are not: the sweeps add with atomics).  The ledger
of device buffers pins the storage policy: what a call takes, and that it keeps it.  The rows below are shared by the
recorder and by tests/test_ss_sequence_gpu.py, which compares exactly against tests/golden/ss_sequence_gpu.json.  The
golden file is recorded from the library of the commit BEFORE a change of the sequence, never from the code under
test, and names that commit:

    python tests/ss_sequence.py --record --lib path/to/the/old/libspllt_hip.so --commit <its hash>

Matrix: matgen.poisson2d(40), nb=16, nemin=16 (n = 1600).  Owners: "handle", one factorization; "batch", 3 members
whose middle one is not positive definite (fields 6 and 7: 2 served, 1 flagged; every call returns -20);
"batch_limit7", the same with batch_grid_limit=7 (the launches split into ranges of members).  Per owner one handle
of its own, and on it k = 1, 17, 33, 48 columns (one group of 16, one of 32, two groups) times: all entries, three
selected rows, job 1, job 2, gram.  Column q of B has an entry in row (37 q + 11) mod n, every third column a
second one; the members of the batch have their own values.

The ledger counts bytes, and a buffer that comes out of the process-wide cache of released buffers keeps its old
size: the table runs in a process of its own with that cache switched off (SPLLT_HIP_CACHE_MB=0, read once).
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "ss_sequence_gpu.json")
ENV = {"SPLLT_HIP_CACHE_MB": "0"}
KS = (1, 17, 33, 48)
VARIANTS = ("all", "rows3", "job1", "job2", "gram")
OWNERS = ("handle", "batch", "batch_limit7")
NBATCH = 3


def columns(n, k):
    import scipy.sparse as sp
    rows, cols, vals = [], [], []
    for q in range(k):
        for j, r in enumerate([(37 * q + 11) % n] + ([(113 * q + 5) % n] if q % 3 == 1 else [])):
            rows.append(r), cols.append(q), vals.append((1.0 + q / 10.0) * (-1.0 if j else 1.0))
    B = sp.csc_matrix((vals, (rows, cols)), shape=(n, k))
    B.sum_duplicates()
    B.sort_indices()
    return B


def run_table(lib):
    """every row, in order: {"owner|k|variant": [rc, [info ...], [ledger entries, ledger bytes]]}"""
    from spllt_amd import api, matgen
    assert os.environ.get("SPLLT_HIP_CACHE_MB") == "0", "the ledger is recorded with the buffer cache switched off"
    A = matgen.poisson2d(40)
    n, ptr, row, val = api.csc_lower_1based(A)
    cols = np.repeat(np.arange(n), np.diff(ptr))
    diag = np.flatnonzero(np.asarray(row) - 1 == cols)
    bad = 1.5 * val
    bad[diag[n // 2]] = -1.0                         # a negative diagonal entry: not positive definite
    vals3 = np.ascontiguousarray(np.stack([val, bad, 2.0 * val]))
    sel = np.array([0, n // 2, n - 1])
    out = {}
    for owner in OWNERS:
        f = api.Factorization(n, ptr, row, nb=16, nemin=16)
        try:
            if owner == "handle":
                f.factor(val).wait()
            else:
                assert f.factor_batch(vals3) == -20
                if owner == "batch_limit7":
                    assert lib.spllt_hip_debug(b"batch_grid_limit=7") == 0
            for k in KS:
                B = columns(n, k)
                bv = np.stack([B.data * (1.0 + b / 2.0) for b in range(NBATCH)])
                for variant in VARIANTS:
                    rows, job = (sel if variant == "rows3" else None), {"job1": 1, "job2": 2}.get(variant, 0)
                    if owner == "handle":
                        f.gram(B) if variant == "gram" else f.solve_sparse(B, rows=rows, job=job)
                        rc, info = 0, f.solve_sparse_info()           # (any other code raises)
                    else:
                        f.gram_batch(B, vals=bv) if variant == "gram" else f.solve_sparse_batch(B, rows=rows, job=job, vals=bv)
                        rc, info = f.solve_sparse_batch_status, f.solve_sparse_batch_info()
                    out[f"{owner}|{k}|{variant}"] = [int(rc), [int(v) for v in info.values()],
                                                     [int(v) for v in f.program("owned")]]
        finally:
            lib.spllt_hip_debug(b"batch_grid_limit=0")
            f.close()
    return out


def pack(table, commit):
    lines = ['{"recorded_from_commit": %s, "rows": {' % json.dumps(commit)]
    lines.append(",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in table.items()))
    return "\n".join(lines) + "\n}}\n"


def load_library(path=None):
    from spllt_amd import _lib
    if path:
        _lib.LIB_PATH = os.path.abspath(path)
    return _lib.load()


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", action="store_true")
    ap.add_argument("--lib", default=None, help="the library to record from (of the commit before the change)")
    ap.add_argument("--commit", default=None, help="the commit that library was built from (--record)")
    ap.add_argument("--out", default=None, help="where the table goes (default with --record: the golden file)")
    a = ap.parse_args()
    os.environ.setdefault("SPLLT_CHAIN_GRAPH_SERIAL", "0")   # (as tests/conftest.py sets it)
    os.environ.update(ENV)
    table = run_table(load_library(a.lib))
    print(f"{len(table)} rows")
    if a.record:
        assert a.commit, "--record needs --commit: the golden file names the commit it was recorded from"
    if a.record or a.out:
        with open(a.out or GOLDEN, "w") as fh:
            fh.write(pack(table, a.commit))
