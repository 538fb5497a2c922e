"""The entry ladder of the product and the refined solves of a batch (include/spllt_hip_batch_refine.h), shared by
tests/test_refine_batch_cpu.py and tests/test_refine_batch_gpu.py.  The family is not in the recorded table of
tests/capi_ladder.py (its header says why); the purpose of that table is met here as in batch_solve_many_ladder.py:
every entry point is called in every handle state with every argument variant, and the return code has to be the
one RECORDED for the matching variant of a sibling in tests/golden/capi_ladder_{cpu,gpu}.json.  A call of this
family has the arguments of two older ones, so the sibling is chosen per variant:

    spllt_hip_matvec_batch(_dev)         spllt_hip_matvec(_dev) for the vectors, the count of vectors, nnz and the
                                         accepted call; spllt_hip_factor_batch(_dev) for nbatch < 0 and ldval < nnz
    spllt_hip_solve_refined_batch(_dev)  spllt_hip_solve_refined(_dev) for the values, the vectors, method, tol and
                                         max_iter; spllt_hip_factor_batch(_dev) for ldval < nnz;
                                         spllt_hip_solve_batch(_dev) for the accepted and the empty call (which need
                                         a batch, not a factorization)
    spllt_hip_solve_refined_batch_info   spllt_hip_solve_sparse_info (a plain reader of int64 counters)
    spllt_hip_release_refine_batch       spllt_hip_release_batch

Handles, arrays and the matrix are those of capi_ladder.Ctx; nothing of capi_ladder is modified."""
import ctypes as C
import json

import capi_ladder


def _H(c, i=0):
    return c.H(i)


def _VALS(c):
    return c.api._dp(c.vals3)


def _I64(c):
    return c.i64.ctypes.data_as(C.POINTER(C.c_int64))


def _short_n(c):
    return c.n - 1


# arguments after fkeep: matvec_batch  0 nbatch 1 nnz 2 val 3 ldval 4 nvec 5 x 6 ldx 7 y 8 ldy (9 pivot_order)
def _mv(sib, fb):
    return {"null_val": ({2: None}, sib, "null_val"), "null_x": ({5: None}, sib, "null_x"),
            "null_y": ({7: None}, sib, "null_y"), "negative": ({4: -1}, sib, "negative"),
            "negative_batch": ({0: -1}, fb, "negative"), "nnz": ({1: lambda c: c.nnz + 1}, sib, "nnz"),
            "short_ldval": ({3: lambda c: c.nnz - 1}, fb, "short_ld"), "short_ldx": ({6: _short_n}, sib, "short_ldx"),
            "short_ldy": ({8: _short_n}, sib, "short_ldy"), "empty": ({4: 0}, sib, "empty"),
            "empty_batch": ({0: 0}, sib, "empty"), "good": ({}, sib, "good")}


# solve_refined_batch  0 nnz 1 val 2 ldval 3 nrhs 4 x 5 ldx 6 method 7 tol 8 max_iter 9 iterations 10 error
def _rf(sib, fb, sb):
    return {"null_val": ({1: None}, sib, "null_val"), "null_x": ({4: None}, sib, "null_x"),
            "negative": ({3: -1}, sib, "negative"), "nnz": ({0: lambda c: c.nnz + 1}, sib, "nnz"),
            "short_ldval": ({2: lambda c: c.nnz - 1}, fb, "short_ld"), "short_ld": ({5: _short_n}, sib, "short_ld"),
            "method": ({6: 2}, sib, "method"), "tol": ({7: 0.0}, sib, "tol"), "max_iter": ({8: -1}, sib, "max_iter"),
            "empty": ({3: 0}, sb, "empty"), "good": ({}, sb, "good")}


def _rf_args(c, val, x):
    return [c.nnz, val, c.nnz, 2, x, c.n, 1, 1e-10, 20, c.api._ip(c.i32), c.H(1)]


# name -> (arguments after fkeep of the accepted call, {variant: (changes, sibling, the sibling's variant)})
ENTRIES = {
    "spllt_hip_matvec_batch": (lambda c: [3, c.nnz, _VALS(c), c.nnz, 2, _H(c, 0), c.n, _H(c, 1), c.n],
                               _mv("spllt_hip_matvec", "spllt_hip_factor_batch")),
    "spllt_hip_matvec_batch_dev": (lambda c: [3, c.nnz, c.DVALS3(), c.nnz, 2, c.D(0), c.n, c.D(1), c.n, 0],
                                   _mv("spllt_hip_matvec_dev", "spllt_hip_factor_batch_dev")),
    "spllt_hip_solve_refined_batch": (lambda c: _rf_args(c, _VALS(c), _H(c)),
                                      _rf("spllt_hip_solve_refined", "spllt_hip_factor_batch", "spllt_hip_solve_batch")),
    "spllt_hip_solve_refined_batch_dev": (lambda c: _rf_args(c, c.DVALS3(), c.D()),
                                          _rf("spllt_hip_solve_refined_dev", "spllt_hip_factor_batch_dev",
                                              "spllt_hip_solve_batch_dev")),
    "spllt_hip_solve_refined_batch_info": (lambda c: [_I64(c)],
                                           {"null": ({0: None}, "spllt_hip_solve_sparse_info", "null"),
                                            "good": ({}, "spllt_hip_solve_sparse_info", "good")}),
}
RELEASE = ("spllt_hip_release_refine_batch", "spllt_hip_release_batch")
ROWS = 2 * 12 + 2 * 11 + 2 + 2


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
        for name, (_, variants) in ENTRIES.items():
            for variant, (changes, sibling, sib_variant) in variants.items():
                # (a sibling's accepted call that would create the engine has no recorded row without a GPU: nor is the
                # call made here)
                if f"{sibling}|{state}|{sib_variant}" not in table:
                    assert not c.gpu and variant == "good", (name, state, variant)
                    continue
                c.reset()
                # (as the recorder: with a GPU the accepted call of state "analysed" runs on a handle of its own)
                fresh = c.gpu and state == "analysed" and variant == "good"
                hv = c.handle(state) if fresh else h
                try:
                    rc, err = call(c, name, hv[1], changes)
                finally:
                    if fresh:
                        c.free(hv)
                want_rc, want_err = table[f"{sibling}|{state}|{sib_variant}"]
                assert rc == want_rc, (name, state, variant, rc, err, want_rc)
                # a refusal with a message names the entry point that was called, not its sibling
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
