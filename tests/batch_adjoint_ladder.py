"""The entry ladder of the batch's factor adjoint (include/spllt_hip_batch_adjoint.h), shared by
tests/test_batch_adjoint_cpu.py and tests/test_batch_adjoint_gpu.py.  The family is not in the recorded table of
tests/capi_ladder.py (its header says why); the purpose of that table is met here as in batch_solve_many_ladder.py:
every entry point is called in every handle state with every argument variant, and the return code has to be the
one RECORDED for the same variant of its sibling in tests/golden/capi_ladder_{cpu,gpu}.json:

    spllt_hip_factor_adjoint_seed_batch(_dev)   spllt_hip_factor_adjoint_seed(_dev)
    spllt_hip_set_factor_adjoint_batch          spllt_hip_set_factor_adjoint
    spllt_hip_factor_adjoint_batch(_dev)        spllt_hip_factor_adjoint(_dev)
    spllt_hip_get_factor_adjoint_batch          spllt_hip_get_inverse_batch (without its "failed_member" row: the
                                                adjoint arena of a failed member is readable, it is what was put in)
    spllt_hip_device_factor_adjoint_batch       spllt_hip_device_inverse_batch
    spllt_hip_batch_adjoint_launches            spllt_hip_batch_selinv_launches
    spllt_hip_release_factor_adjoint_batch      spllt_hip_release_inverse_batch

and, on a handle without a batch (states analysed, engine, partitioned), the accepted call of every entry point that
needs one returns the code and the words RECORDED for spllt_hip_selected_inverse_batch in that state.

Without a device the states are those of capi_ladder.CPU_STATES.  With one, the batch takes the place the single
factor has for the siblings of the first three lines, and the adjoint arenas the place of the inverse arenas for the
others: a state of this ladder is compared with the sibling's rows of the state SIBLING_STATE names.  The batches of
these states hold three positive definite members (a sweep of the recorded "batch" state, which has a failed
member, returns -20 where the single sweep returns 0).  Arrays and the matrix are those of capi_ladder.Ctx; nothing
of capi_ladder is modified."""
import ctypes as C
import json

import numpy as np

import capi_ladder

_seed = {"null": {1: None}, "negative": {0: -1}, "short_ld": {3: lambda c: c.n - 1}, "accumulate": {5: 2}, "flags": {6: 4}}
_member = {"null": {1: None}, "negative": {2: -1}, "member": {0: 7}}


def _I64(c):
    return c.i64.ctypes.data_as(C.POINTER(C.c_int64))


# name -> (arguments after fkeep of the accepted call, variants, sibling, kind, flags): kind picks the column of
# SIBLING_STATE; flags "m": an accepted call changes the state of the handle (it runs on a fresh one), "p": returns
# a pointer (compared as 0 / 1)
ENTRIES = {
    "spllt_hip_factor_adjoint_seed_batch": (lambda c: [2, c.H(0), c.H(1), c.n, 1.0, 0, 0], _seed,
                                            "spllt_hip_factor_adjoint_seed", "adjoint", "m"),
    "spllt_hip_factor_adjoint_seed_batch_dev": (lambda c: [2, c.D(0), c.D(1), c.n, 1.0, 0, 0], _seed,
                                                "spllt_hip_factor_adjoint_seed_dev", "adjoint", "m"),
    "spllt_hip_set_factor_adjoint_batch": (lambda c: [c.H(), c.arena], {"null": {0: None}, "short": {1: lambda c: c.arena - 1}},
                                           "spllt_hip_set_factor_adjoint", "adjoint", "m"),
    "spllt_hip_get_factor_adjoint_batch": (lambda c: [0, c.H(), c.arena], _member, "spllt_hip_get_inverse_batch", "arena", ""),
    "spllt_hip_device_factor_adjoint_batch": (lambda c: [_I64(c)], {}, "spllt_hip_device_inverse_batch", "arena", "p"),
    "spllt_hip_factor_adjoint_batch": (lambda c: [c.H(), c.nnz], {"null": {0: None}}, "spllt_hip_factor_adjoint", "adjoint", "m"),
    "spllt_hip_factor_adjoint_batch_dev": (lambda c: [c.D(), c.nnz], {"null": {0: None}}, "spllt_hip_factor_adjoint_dev",
                                           "adjoint", "m"),
    "spllt_hip_batch_adjoint_launches": (lambda c: [], {}, "spllt_hip_batch_selinv_launches", "count", ""),
}
RELEASE = ("spllt_hip_release_factor_adjoint_batch", "spllt_hip_release_inverse_batch")
ROWS_PER_STATE = sum(len(e[1]) + 1 for e in ENTRIES.values()) + 2

NO_BATCH_SIBLING = "spllt_hip_selected_inverse_batch"
NO_BATCH_STATES = ("analysed", "engine", "partitioned")
GPU_STATES = ("analysed", "engine", "batch", "batch_seeded", "batch_swept")
# state of this ladder -> the sibling's recorded state, per kind (None: no recorded row says the same thing)
# ("engine": the single seed runs on an engine without a factor, which it does not read; the batch family refuses "no
# batch yet" like spllt_hip_selected_inverse_batch, so its rows are those of the single family without an engine)
SIBLING_STATE = {
    "engine": {"adjoint": "analysed"},
    "batch": {"adjoint": "factored", "arena": "batch", "count": "batch", "release": "batch"},
    "batch_seeded": {"adjoint": "adjoint_seeded", "arena": "batch_inverse", "count": "batch", "release": "batch_inverse"},
    "batch_swept": {"adjoint": "adjoint_swept", "arena": "batch_inverse", "count": None, "release": "batch_inverse"},
}


def golden(gpu):
    return capi_ladder.unpack(json.load(open(capi_ladder.GOLDEN[gpu])))


def handle(c, state):
    """(akeep, fkeep) in `state`; the batch states are built on capi_ladder's "engine" handle"""
    if not state.startswith("batch"):
        return c.handle(state)
    h = c.handle("engine")
    vals = np.ascontiguousarray(np.stack([c.val, 2.0 * c.val, 0.5 * c.val]))
    assert c.lib.spllt_hip_factor_batch(h[0], h[1], 3, c.nnz, vals.ctypes.data, c.nnz) == 0
    if state in ("batch_seeded", "batch_swept"):
        assert c.lib.spllt_hip_factor_adjoint_seed_batch(h[1], 1, c.H(0), c.H(1), c.n, 1.0, 0, 0) == 0
    if state == "batch_swept":
        assert c.lib.spllt_hip_factor_adjoint_batch(h[1], c.H(2), c.nnz) == 0
    return h


def call(c, name, fk, changes):
    good, _, _, _, flags = ENTRIES[name]
    args = good(c)
    for pos, v in changes.items():
        args[pos] = v(c) if callable(v) else v
    rc = getattr(c.lib, name)(fk, *args)
    rc = int(bool(rc)) if "p" in flags else int(rc)
    return rc, (c.lib.spllt_hip_last_error(fk) or b"").decode() if rc < 0 else None


def check_state(c, state, table):
    """every entry point x variant on one handle in `state`, against the sibling's recorded rows; returns the number
    of rows run"""
    h = handle(c, state)
    rows = 0
    try:
        for name, (_, bad, sibling, kind, flags) in ENTRIES.items():
            sstate = SIBLING_STATE.get(state, {}).get(kind, state)
            for variant in list(bad) + ["good"]:
                c.reset()
                fresh = variant == "good" and ("m" in flags or (c.gpu and state == "analysed"))
                hv = handle(c, state) if fresh else h
                try:
                    rc, err = call(c, name, hv[1], bad.get(variant, {}))
                finally:
                    if fresh:
                        c.free(hv)
                rows += 1
                if sstate is None:      # (the launch count of a sweep: checked against the tables by the GPU test)
                    assert rc > 0, (name, state, rc)
                    continue
                want_rc, want_err = table[f"{sibling}|{sstate}|{variant}"]
                assert rc == want_rc, (name, state, variant, rc, err, sibling, sstate, want_rc)
                # a refusal with a message names the entry point that was called, not its sibling
                if want_err and want_rc < 0 and want_err.startswith(sibling + ":"):
                    assert err.startswith(name + ": "), (name, state, variant, err)
                # the "no batch yet" rung (and the partitioned one before it): code AND words of the recorded row of
                # spllt_hip_selected_inverse_batch, whose order of rungs this family has
                if variant == "good" and state in NO_BATCH_STATES and kind != "count" and "p" not in flags:
                    b_rc, b_err = table[f"{NO_BATCH_SIBLING}|{state}|good"]
                    assert rc == b_rc, (name, state, rc, b_rc)
                    if b_err and b_err.startswith(NO_BATCH_SIBLING + ":"):
                        assert err == b_err.replace(NO_BATCH_SIBLING + ":", name + ":"), (name, state, err, b_err)
        for variant in ("good", "fresh"):     # (twice on this handle: the second finds nothing to release)
            rc = int(getattr(c.lib, RELEASE[0])(h[1]))
            sstate = SIBLING_STATE.get(state, {}).get("release", state)
            assert rc == table[f"{RELEASE[1]}|{sstate}|{variant}"][0], (RELEASE[0], state, variant, rc)
            rows += 1
    finally:
        c.free(h)
    return rows
