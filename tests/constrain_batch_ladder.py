"""The entry ladder of the hard linear constraints of a batch (include/spllt_hip_constrain_batch.h), shared by
tests/test_constrain_batch_cpu.py and tests/test_constrain_batch_gpu.py.  The family is not in the recorded table of
tests/capi_ladder.py (its header says why); the purpose of that table is met here as in constrain_ladder.py and
batch_refine_ladder.py: every entry point is called in every handle state with every argument variant, and the return
code has to be the one RECORDED for the matching variant of a sibling in tests/golden/capi_ladder_{cpu,gpu}.json:

    spllt_hip_set_constraints_batch(_dev)   spllt_hip_solve_batch(_dev): C has the layout of the vectors (k for nrhs,
                                            ldc for ldx; k = 65 against the sibling's other refused argument, job = 3);
                                            the accepted call needs a batch and returns the -20 of a batch with a
                                            member that is not positive definite, as every batch call does
    spllt_hip_constrain_batch(_dev), spllt_hip_solve_constrained_batch(_dev), spllt_hip_sample_constrained_batch(_dev)
                                            spllt_hip_solve_batch(_dev) for the vector arguments, the empty and the
                                            accepted call, message for message (spllt_hip_solve_many_batch(_dev) and
                                            spllt_hip_sample_batch(_dev) are checked against the same rows)
    spllt_hip_inverse_diag_constrained_batch    spllt_hip_inverse_diag_batch
    spllt_hip_constraints_batch_info        spllt_hip_solve_sparse_info (a plain reader of counters)
    spllt_hip_release_constraints_batch     spllt_hip_release_batch

Within a state the rows run in the order of ENTRIES on one handle and "good" is the last variant of an entry, so the
accepted spllt_hip_set_constraints_batch (one row of ones) has stored its constraint before the first call that needs
one.  GPU_STATES leaves out "batch_inverse": there the variances of this family return the -20 of the batch's failed
member where spllt_hip_inverse_diag_batch returns 0 (tests/test_constrain_batch_gpu.py checks that call by itself).
Handles, arrays and the matrix are those of capi_ladder.Ctx; nothing of capi_ladder is modified."""
import ctypes as C
import json

import capi_ladder


def _I64(c):
    return c.i64.ctypes.data_as(C.POINTER(C.c_int64))


def _H(c, i=0):
    return C.c_void_p(c.host[i].ctypes.data)


def _short_n(c):
    return c.n - 1


# arguments after fkeep: set_constraints_batch  0 k 1 c 2 ldc
def _set(sib):
    return {"null": ({1: None}, sib, "null"), "negative": ({0: -1}, sib, "negative"), "too_many": ({0: 65}, sib, "job"),
            "short_ld": ({2: _short_n}, sib, "short_ld"), "good": ({}, sib, "good")}


# constrain_batch / solve_constrained_batch / sample_constrained_batch  0 nvec 1 x 2 ldx ...
def _vec(sib):
    return {"null": ({1: None}, sib, "null"), "negative": ({0: -1}, sib, "negative"),
            "short_ld": ({2: _short_n}, sib, "short_ld"), "empty": ({0: 0}, sib, "empty"), "good": ({}, sib, "good")}


_SB, _SBD = "spllt_hip_solve_batch", "spllt_hip_solve_batch_dev"
# name -> (arguments after fkeep of the accepted call, {variant: (changes, sibling, the sibling's variant)},
#          whether a refusal's message is the sibling's word for word)
ENTRIES = {
    "spllt_hip_set_constraints_batch": (lambda c: [1, c.H(0), c.n], _set(_SB), False),
    "spllt_hip_set_constraints_batch_dev": (lambda c: [1, c.D(0), c.n], _set(_SBD), False),
    "spllt_hip_constrain_batch": (lambda c: [2, _H(c, 0), c.n, _H(c, 1), 0, _H(c, 2), 1], _vec(_SB), True),
    "spllt_hip_constrain_batch_dev": (lambda c: [2, c.D(0), c.n, c.D(1), 0, c.D(2), 1], _vec(_SBD), True),
    "spllt_hip_solve_constrained_batch": (lambda c: [2, _H(c, 0), c.n, _H(c, 1), 0, _H(c, 2), 1], _vec(_SB), True),
    "spllt_hip_solve_constrained_batch_dev": (lambda c: [2, c.D(0), c.n, c.D(1), 0, c.D(2), 1], _vec(_SBD), True),
    "spllt_hip_sample_constrained_batch": (lambda c: [2, _H(c, 0), c.n, 1, 0, 0, 1, None, 0, None], _vec(_SB), True),
    "spllt_hip_sample_constrained_batch_dev": (lambda c: [2, c.D(0), c.n, 1, 0, 0, 1, None, 0, None], _vec(_SBD), True),
    "spllt_hip_inverse_diag_constrained_batch": (lambda c: [c.H(0), c.n],
                                                 {"null": ({0: None}, "spllt_hip_inverse_diag_batch", "null"),
                                                  "short_ld": ({1: _short_n}, "spllt_hip_inverse_diag_batch", "short_ld"),
                                                  "good": ({}, "spllt_hip_inverse_diag_batch", "good")}, True),
    "spllt_hip_constraints_batch_info": (lambda c: [_I64(c), c.H(1), 2],
                                         {"null": ({0: None}, "spllt_hip_solve_sparse_info", "null"),
                                          "good": ({}, "spllt_hip_solve_sparse_info", "good")}, True),
}
RELEASE = ("spllt_hip_release_constraints_batch", "spllt_hip_release_batch")
ROWS = 2 * 5 + 6 * 5 + 3 + 2 + 2
GPU_STATES = ("engine", "factored", "not_posdef", "downdate_failed", "batch")


def golden(gpu):
    return capi_ladder.unpack(json.load(open(capi_ladder.GOLDEN[gpu])))


def call(c, name, fk, changes):
    args = ENTRIES[name][0](c)
    for pos, v in changes.items():
        args[pos] = v(c) if callable(v) else v
    rc = int(getattr(c.lib, name)(fk, *args))
    return rc, (c.lib.spllt_hip_last_error(fk) or b"").decode() if rc < 0 else None


def check_state(c, state, table):
    """every entry point x variant on one handle in `state`, against the siblings' recorded rows; returns the number
    of rows checked"""
    h = c.handle(state)
    rows = 0
    try:
        for name, (_, variants, exact) in ENTRIES.items():
            for variant, (changes, sibling, sib_variant) in variants.items():
                c.reset()
                rc, err = call(c, name, h[1], changes)
                want_rc, want_err = table[f"{sibling}|{state}|{sib_variant}"]
                assert rc == want_rc, (name, state, variant, rc, err, want_rc)
                # a refusal with a message names the entry point that was called, not its sibling (-20 is the batch's
                # failed member: every family words that in its own way)
                if want_err and want_rc < 0 and want_err.startswith(sibling + ":"):
                    assert err.startswith(name + ": "), (name, state, variant, err)
                    if exact and rc != -20:
                        assert err == want_err.replace(sibling + ":", name + ":"), (name, state, variant, err)
                rows += 1
        for variant in ("good", "fresh"):     # (twice on this handle: the second finds nothing to release)
            rc = int(getattr(c.lib, RELEASE[0])(h[1]))
            assert rc == table[f"{RELEASE[1]}|{state}|{variant}"][0], (RELEASE[0], state, variant, rc)
            rows += 1
    finally:
        c.free(h)
    return rows
