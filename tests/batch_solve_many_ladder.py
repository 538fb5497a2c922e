"""The entry ladder of the blocked batch solve (include/spllt_hip_batch_solve_many.h), shared by
tests/test_solve_many_batch_cpu.py and tests/test_solve_many_batch_gpu.py.  The family is not in the recorded table
of tests/capi_ladder.py (its header says why); the purpose of that table is met here as in batch_mult_ladder.py:
every entry point is called in every handle state with every argument variant, and the return code has to be the
one RECORDED for the same variant of its sibling in tests/golden/capi_ladder_{cpu,gpu}.json:

    spllt_hip_solve_many_batch          spllt_hip_solve_batch
    spllt_hip_solve_many_batch_dev      spllt_hip_solve_batch_dev
    spllt_hip_set_batch_blocked_solve   spllt_hip_set_reproducible_solve (a plain setter that returns the previous
                                        setting and refuses "on" on a partitioned handle)
    spllt_hip_solve_many_batch_info     spllt_hip_solve_sparse_info (a plain reader of int64 counters)
    spllt_hip_release_solve_many_batch  spllt_hip_release_batch

Handles, arrays and the matrix are those of capi_ladder.Ctx; nothing of capi_ladder is modified."""
import ctypes as C
import json

import capi_ladder

_vec = {"null": {1: None}, "negative": {0: -1}, "short_ld": {2: lambda c: c.n - 1}, "empty": {0: 0}}
_job = dict(_vec, job={3: 3})


def _H(c):
    return C.c_void_p(c.host[0].ctypes.data)


def _I64(c):
    return c.i64.ctypes.data_as(C.POINTER(C.c_int64))


# name -> (arguments after fkeep of the accepted call, variants, sibling).  The variants of a sibling are run in the
# order in which they were recorded on its shared handle (list(bad) + ["good"]): the setter returns the previous
# setting, so its "good" row (off) after its "on" row returns 1 where the handle accepted "on".
ENTRIES = {
    "spllt_hip_solve_many_batch": (lambda c: [2, _H(c), c.n, 0], _job, "spllt_hip_solve_batch"),
    "spllt_hip_solve_many_batch_dev": (lambda c: [2, c.D(), c.n, 0, 0], _job, "spllt_hip_solve_batch_dev"),
    "spllt_hip_set_batch_blocked_solve": (lambda c: [0], {"on": {0: 1}}, "spllt_hip_set_reproducible_solve"),
    "spllt_hip_solve_many_batch_info": (lambda c: [_I64(c)], {"null": {0: None}}, "spllt_hip_solve_sparse_info"),
}
RELEASE = ("spllt_hip_release_solve_many_batch", "spllt_hip_release_batch")


def golden(gpu):
    return capi_ladder.unpack(json.load(open(capi_ladder.GOLDEN[gpu])))


def call(c, name, fk, changes):
    args = ENTRIES[name][0](c)
    for pos, v in changes.items():
        args[pos] = v(c) if callable(v) else v
    rc = int(getattr(c.lib, name)(fk, *args))
    return rc, (c.lib.spllt_hip_last_error(fk) or b"").decode() if rc < 0 else None


def check_state(c, state, table):
    """every entry point x variant on one handle in `state`, against the sibling's recorded rows; returns the number
    of rows checked"""
    h = c.handle(state)
    rows = 0
    try:
        for name, (_, bad, sibling) in ENTRIES.items():
            for variant in list(bad) + ["good"]:
                c.reset()
                # (as the recorder: with a GPU the accepted call of state "analysed" runs on a handle of its own)
                fresh = c.gpu and state == "analysed" and variant == "good"
                hv = c.handle(state) if fresh else h
                try:
                    rc, err = call(c, name, hv[1], bad.get(variant, {}))
                finally:
                    if fresh:
                        c.free(hv)
                want_rc, want_err = table[f"{sibling}|{state}|{variant}"]
                assert rc == want_rc, (name, state, variant, rc, err, want_rc)
                # a refusal with a message names the entry point that was called, not its sibling
                # (a recorded message that does not name the sibling is the handle's message of an earlier row: the
                # plain setters and readers refuse without one, and return code 1 is the setter's "it was on")
                if want_err and want_rc < 0 and want_err.startswith(sibling + ":"):
                    assert err.startswith(name + ": "), (name, state, variant, err)
                    if rc != -20:
                        assert err == want_err.replace(sibling + ":", name + ":"), (name, state, variant, err)
                rows += 1
        for variant in ("good", "fresh"):     # (twice on this handle: the second finds nothing to release)
            rc = int(getattr(c.lib, RELEASE[0])(h[1]))
            assert rc == table[f"{RELEASE[1]}|{state}|{variant}"][0], (RELEASE[0], state, variant, rc)
            rows += 1
    finally:
        c.free(h)
    return rows
