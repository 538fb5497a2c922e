"""The entry ladder of the update / downdate of a batch (include/spllt_hip_updown_batch.h).  The family is not in
the recorded table of tests/capi_ladder.py (its header says why); as in batch_repro_ladder.py the return code of a
call in a handle state has to be the one RECORDED for its sibling in tests/golden/capi_ladder_{cpu,gpu}.json:

    spllt_hip_updown_batch(_dev)       spllt_hip_selected_inverse_batch (SINGLE | WAIT_IGNORE | BATCH, changes the batch)
    spllt_hip_updown_batch_info        spllt_hip_solve_sparse_info (a plain reader of int64 counters)
    spllt_hip_updown_batch_time        spllt_hip_updown_time (a plain reader of one double)
    spllt_hip_release_updown_batch     spllt_hip_release_batch

and every argument refusal of spllt_hip_updown (null arrays, k < 0, bad sign, unsorted rows, row out of range,
inadmissible column) plus ldw too small returns SPLLT_ERROR_PARAMETER in every state that reaches the argument
rung (an analysed handle, partitioned or not: the arguments are looked at before the device is)."""
import ctypes as C

import numpy as np

import batch_solve_many_ladder as base

golden = base.golden
UPDOWN = ("spllt_hip_updown_batch", "spllt_hip_updown_batch_dev")


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def good_args(c):
    """one column 0.5 e_1 (variable 1), three members' values with ldw = 2"""
    wptr, wrow, _ = c.one_col
    vals = np.array([0.5, 0.0, 0.25, 0.0, 0.125, 0.0])
    return [1, wptr, wrow, vals, 2, 1]


def inadmissible(c):
    """the first pivots of two leaves of the elimination tree: never adjacent in L"""
    from spllt_amd import api
    f = api.Factorization(c.n, c.ptr, c.row, nb=int(c.opt.nb), nemin=int(c.opt.nemin))
    sptr, sparent, order = f.sym("sptr"), f.sym("sparent"), f.sym("order")
    inv = np.empty(c.n, dtype=np.int64)
    inv[order] = np.arange(c.n)
    leaves = sorted(set(range(len(sparent))) - set(int(p) for p in sparent))
    rows = sorted(int(inv[sptr[s]]) + 1 for s in leaves[:2])
    f.close()
    return np.array(rows + [0], dtype=np.int32)


def variants(c):
    """name -> changed argument list"""
    g = good_args(c)
    two = np.array([1, 3], dtype=np.int32)
    vals2 = np.array([0.5, 0.25, 0.5, 0.25, 0.5, 0.25])

    def ch(**kw):
        a = list(g)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return a
    return {
        "null_ptr": ch(a1=None), "null_row": ch(a2=None), "null_val": ch(a3=None), "negative": ch(a0=-1),
        "sign": ch(a5=0), "sign2": ch(a5=2),
        "unsorted": ch(a1=two, a2=np.array([2, 1, 0], dtype=np.int32), a3=vals2),
        "row_range": ch(a2=c.bad_row),
        "inadmissible": ch(a1=two, a2=inadmissible(c), a3=vals2),
        "short_ldw": ch(a4=0),
    }


def call(c, name, fk, args):
    k, wptr, wrow, vals, ldw, sign = args
    rc = int(getattr(c.lib, name)(fk, k, None if wptr is None else _ip(wptr), None if wrow is None else _ip(wrow),
                                  None if vals is None else C.c_void_p(vals.ctypes.data), ldw, sign))
    return rc, (c.lib.spllt_hip_last_error(fk) or b"").decode() if rc < 0 else None


def check_state(c, state, table):
    """every entry point on one handle in `state`; returns the number of rows checked"""
    assert not c.gpu, "the rows hand host arrays to the _dev form: they are for the states without a device"
    h = c.handle(state)
    rows = 0
    reaches_arguments = state not in ("null", "unanalysed")
    try:
        for name in UPDOWN:
            for variant, args in variants(c).items():
                rc, err = call(c, name, h[1], args)
                assert rc == -10, (name, state, variant, rc, err)
                if reaches_arguments:
                    assert err.startswith(name + ": "), (name, state, variant, err)
                rows += 1
            rc, err = call(c, name, h[1], good_args(c))
            want_rc, want_err = table[f"spllt_hip_selected_inverse_batch|{state}|good"]
            assert rc == want_rc, (name, state, rc, err, want_rc)
            if want_err and want_err.startswith("spllt_hip_selected_inverse_batch:"):
                assert err == want_err.replace("spllt_hip_selected_inverse_batch:", name + ":"), (name, state, err)
            rows += 1
        i64 = c.i64.ctypes.data_as(C.POINTER(C.c_int64))
        for variant, arg in (("null", None), ("good", i64)):
            rc = int(c.lib.spllt_hip_updown_batch_info(h[1], arg))
            assert rc == table[f"spllt_hip_solve_sparse_info|{state}|{variant}"][0], (state, variant, rc)
            rows += 1
        for variant, arg in (("null", None), ("good", C.byref(c.dbl))):
            rc = int(c.lib.spllt_hip_updown_batch_time(h[1], arg))
            assert rc == table[f"spllt_hip_updown_time|{state}|{variant}"][0], (state, variant, rc)
            rows += 1
        for variant in ("good", "fresh"):
            rc = int(c.lib.spllt_hip_release_updown_batch(h[1]))
            assert rc == table[f"spllt_hip_release_batch|{state}|{variant}"][0], (state, variant, rc)
            rows += 1
    finally:
        c.free(h)
    return rows


ROWS = 2 * (10 + 1) + 2 + 2 + 2
