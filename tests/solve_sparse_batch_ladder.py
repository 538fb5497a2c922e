"""The entry ladder of the sparse right-hand-side solves of a batch (include/spllt_hip_solve_sparse_batch.h).  The
family is not in the recorded table of tests/capi_ladder.py (its header says why); as in updown_batch_ladder.py the
return code of a call in a handle state has to be the one RECORDED in tests/golden/capi_ladder_{cpu,gpu}.json for a
sibling with the same needs of its handle:

    spllt_hip_solve_sparse_batch(_dev)      spllt_hip_solve_batch -- the recorded sibling of spllt_hip_solve_many_batch
    spllt_hip_gram_sparse_batch(_dev)       (SINGLE | WAIT_IGNORE | BATCH, serves every member of the batch)
    spllt_hip_solve_sparse_batch_info       spllt_hip_solve_sparse_info (a plain reader of int64 counters)
    spllt_hip_release_solve_sparse_batch    spllt_hip_release_batch

and every argument refusal of spllt_hip_solve_sparse (null arrays, k < 0, unsorted rows, row or wanted variable out
of range, bad job, output too narrow) plus a member stride that is neither 0 nor large enough returns
SPLLT_ERROR_PARAMETER in every state that reaches the argument rung (an analysed handle, partitioned or not: the
arguments are looked at before the device is)."""
import ctypes as C

import numpy as np

import batch_solve_many_ladder as base

golden = base.golden
SOLVE = ("spllt_hip_solve_sparse_batch", "spllt_hip_solve_sparse_batch_dev")
GRAM = ("spllt_hip_gram_sparse_batch", "spllt_hip_gram_sparse_batch_dev")
SIBLING = "spllt_hip_solve_batch"


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def solve_args(c):
    """two columns (variables 1 and 3), three members' values with ldb = 2, wanted variables 2 and 1, ldx = 2"""
    bptr = np.array([1, 2, 3], dtype=np.int32)
    brow = np.array([1, 3, 0], dtype=np.int32)
    vals = np.array([0.5, 1.0, 0.25, 2.0, 0.125, 3.0])
    sel = np.array([2, 1, 0], dtype=np.int32)
    return dict(k=2, bptr=bptr, brow=brow, bval=vals, ldb=2, nsel=2, sel=sel, x=c.host[0], ld=2, job=0)


def solve_variants(c):
    n = c.n
    i32 = lambda a: np.array(a, dtype=np.int32)   # noqa: E731
    return {
        "null_ptr": dict(bptr=None), "null_row": dict(brow=None), "null_val": dict(bval=None), "null_out": dict(x=None),
        "negative": dict(k=-1), "unsorted": dict(bptr=i32([1, 3, 3]), brow=i32([3, 1, 0])),
        "row_range": dict(brow=i32([1, n + 5, 0])), "sel_range": dict(sel=i32([2, n + 1, 0])),
        "job": dict(job=3), "short_ld": dict(ld=1), "short_ldb": dict(ldb=1), "negative_ldb": dict(ldb=-2),
    }


def gram_variants(c):
    v = solve_variants(c)
    for name in ("sel_range", "job"):     # (gram has neither argument)
        del v[name]
    return v


def call(c, name, fk, a):
    p = lambda v, conv: None if v is None else conv(v)   # noqa: E731
    out = None if a["x"] is None else C.c_void_p(a["x"].ctypes.data)
    head = (fk, a["k"], p(a["bptr"], _ip), p(a["brow"], _ip), p(a["bval"], _dp), a["ldb"])
    if name in SOLVE:
        rc = getattr(c.lib, name)(*head, a["nsel"], p(a["sel"], _ip), out if name.endswith("_dev") else p(a["x"], _dp),
                                  a["ld"], a["job"])
    else:
        rc = getattr(c.lib, name)(*head, out if name.endswith("_dev") else p(a["x"], _dp), a["ld"])
    rc = int(rc)
    return rc, (c.lib.spllt_hip_last_error(fk) or b"").decode() if rc < 0 else None


def check_state(c, state, table):
    """every entry point on one handle in `state`; returns the number of rows checked"""
    assert not c.gpu, "the rows hand host arrays to the _dev forms: they are for the states without a device"
    h = c.handle(state)
    rows = 0
    reaches_arguments = state not in ("null", "unanalysed")
    try:
        for names, variants in ((SOLVE, solve_variants(c)), (GRAM, gram_variants(c))):
            for name in names:
                for variant, change in variants.items():
                    before = c.host[0].copy()
                    rc, err = call(c, name, h[1], dict(solve_args(c), **change))
                    assert rc == -10, (name, state, variant, rc, err)
                    if reaches_arguments:
                        assert err.startswith(name + ": "), (name, state, variant, err)
                    assert np.array_equal(before, c.host[0]), (name, state, variant)
                    rows += 1
                rc, err = call(c, name, h[1], solve_args(c))
                want_rc, want_err = table[f"{SIBLING}|{state}|good"]
                assert rc == want_rc, (name, state, rc, err, want_rc)
                if want_err and want_err.startswith(SIBLING + ":"):
                    assert err == want_err.replace(SIBLING + ":", name + ":"), (name, state, err)
                rows += 1
        i64 = c.i64.ctypes.data_as(C.POINTER(C.c_int64))
        for variant, arg in (("null", None), ("good", i64)):
            rc = int(c.lib.spllt_hip_solve_sparse_batch_info(h[1], arg))
            assert rc == table[f"spllt_hip_solve_sparse_info|{state}|{variant}"][0], (state, variant, rc)
            rows += 1
        for variant in ("good", "fresh"):
            rc = int(c.lib.spllt_hip_release_solve_sparse_batch(h[1]))
            assert rc == table[f"spllt_hip_release_batch|{state}|{variant}"][0], (state, variant, rc)
            rows += 1
    finally:
        c.free(h)
    return rows


ROWS = 2 * (12 + 1) + 2 * (10 + 1) + 2 + 2
