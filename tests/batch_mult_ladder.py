"""The entry ladder of the batched factor products and samplers (include/spllt_hip_batch_mult.h), shared by
tests/test_batch_mult_cpu.py and tests/test_batch_mult_gpu.py.  The family is not in the recorded table of
tests/capi_ladder.py (its header says why); the purpose of that table is met here: every entry point is called
in every handle state with every argument variant, and the return code has to be the one RECORDED for the same
variant of its sibling -- spllt_hip_solve_batch for the host functions, spllt_hip_solve_batch_dev for the device
functions, spllt_hip_release_batch for the release -- in tests/golden/capi_ladder_{cpu,gpu}.json.  Handles, arrays
and the matrix are those of capi_ladder.Ctx; nothing of capi_ladder is modified."""
import ctypes as C
import json

import numpy as np

import capi_ladder
from factor_mult_emulate import philox4x32_10

_vec = {"null": {1: None}, "negative": {0: -1}, "short_ld": {2: lambda c: c.n - 1}, "empty": {0: 0}}
_job = dict(_vec, job={3: 3})
_kind = dict(_vec, kind={3: 2})


def _H(c):
    return C.c_void_p(c.host[0].ctypes.data)


# name -> (arguments after fkeep of the accepted call, variants, sibling); variant "kind" is the sibling's "job"
ENTRIES = {
    "spllt_hip_factor_mult_batch": (lambda c: [2, _H(c), c.n, 0], _job, "spllt_hip_solve_batch"),
    "spllt_hip_factor_mult_batch_dev": (lambda c: [2, c.D(), c.n, 0, 0], _job, "spllt_hip_solve_batch_dev"),
    "spllt_hip_white_noise_batch_dev": (lambda c: [2, c.D(), c.n, 1, 0, 0, 1], _vec, "spllt_hip_solve_batch_dev"),
    "spllt_hip_sample_batch": (lambda c: [2, _H(c), c.n, 1, 1, 0, 0, 1, None, 0], _kind, "spllt_hip_solve_batch"),
    "spllt_hip_sample_batch_dev": (lambda c: [2, c.D(), c.n, 1, 1, 0, 0, 1, None, 0], _kind, "spllt_hip_solve_batch_dev"),
}
# positions of stream_step and (mean, ldmean) for the two checks the siblings do not have
EXTRA = {
    "spllt_hip_white_noise_batch_dev": {"stream_step": {6: 2}},
    "spllt_hip_sample_batch": {"stream_step": {7: 2}, "ldmean": {8: _H, 9: lambda c: c.n - 1}},
    "spllt_hip_sample_batch_dev": {"stream_step": {7: 2}, "ldmean": {8: lambda c: c.D(1), 9: lambda c: c.n - 1}},
}
RELEASE = ("spllt_hip_release_factor_mult_batch", "spllt_hip_release_batch")


def golden(gpu):
    return capi_ladder.unpack(json.load(open(capi_ladder.GOLDEN[gpu])))


def call(c, name, fk, changes):
    args = ENTRIES[name][0](c)
    for pos, v in changes.items():
        args[pos] = v(c) if callable(v) else v
    rc = int(getattr(c.lib, name)(fk, *args))
    return rc, (c.lib.spllt_hip_last_error(fk) or b"").decode() if rc else None


def check_state(c, state, table):
    """every entry point x variant on one handle in `state`, against the sibling's recorded rows; returns the number
    of rows checked"""
    h = c.handle(state)
    rows = 0
    try:
        for name, (_, bad, sibling) in ENTRIES.items():
            for variant in list(bad) + ["good"]:
                c.reset()
                rc, err = call(c, name, h[1], bad.get(variant, {}))
                want_rc, want_err = table[f"{sibling}|{state}|{'job' if variant == 'kind' else variant}"]
                assert rc == want_rc, (name, state, variant, rc, err, want_rc)
                # a refusal with a message names the entry point that was called, not its sibling
                if want_err:
                    assert err.startswith(name + ": "), (name, state, variant, err)
                    if variant != "kind" and rc != -20:
                        assert err == want_err.replace(sibling + ":", name + ":"), (name, state, variant, err)
                rows += 1
            if state not in ("null", "unanalysed"):
                for variant, changes in EXTRA.get(name, {}).items():
                    rc, err = call(c, name, h[1], changes)
                    assert rc == -10 and err.startswith(name + ": ") and variant in err, (name, state, variant, rc, err)
                    rows += 1
        rc = int(getattr(c.lib, RELEASE[0])(h[1]))
        assert rc == table[f"{RELEASE[1]}|{state}|good"][0], (RELEASE[0], state, rc)
        rows += 1
    finally:
        c.free(h)
    return rows


def noise_reference(n, nsamp, seed, stream, first_sample=0):
    """the definition in include/spllt_hip_batch_mult.h, in numpy: white_noise_reference with counter word 1"""
    p = np.arange(n, dtype=np.uint32)[:, None]
    s = (np.arange(nsamp, dtype=np.uint64) + np.uint64(first_sample))[None, :]
    w = philox4x32_10(p, np.uint32(stream), (s & np.uint64(0xFFFFFFFF)).astype(np.uint32),
                      (s >> np.uint64(32)).astype(np.uint32), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    a = ((w[1].astype(np.uint64) << np.uint64(32)) | w[0].astype(np.uint64)) >> np.uint64(11)
    b = ((w[3].astype(np.uint64) << np.uint64(32)) | w[2].astype(np.uint64)) >> np.uint64(11)
    return np.sqrt(-2.0 * np.log((a + np.uint64(1)).astype(np.float64) * 2.0 ** -53)) * \
        np.cos((2.0 * np.pi) * (b.astype(np.float64) * 2.0 ** -53))
