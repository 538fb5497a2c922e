"""The recorded table of the entry ladder of the C boundary (spllt_amd/csrc/capi.cpp).

A row is (entry point, handle state, argument variant) -> [rc, last_error when rc < 0 or rc == 1].  The rows below
are shared by the recorder and by tests/test_capi_ladder_{cpu,gpu}.py, which compare exactly against
tests/golden/capi_ladder_{cpu,gpu}.json.  The golden files are recorded from the library of the commit
BEFORE a change of the boundary, never from the code under test:

    python tests/capi_ladder.py --record --lib path/to/the/old/libspllt_hip.so [--gpu]

Matrix: matgen.poisson2d(8), nb=16, nemin=8.  Variant "good" is the accepted call, every other variant changes
one argument into one that the entry point's own checks name.  Within a state the rows run in the order
of ENTRIES on one shared handle; an accepted call that would change the state runs on a fresh handle of that
state, and the eight releases run last (each also on a fresh handle, variant "fresh").
"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = {False: os.path.join(ROOT, "tests", "golden", "capi_ladder_cpu.json"),
          True: os.path.join(ROOT, "tests", "golden", "capi_ladder_gpu.json")}
CPU_STATES = ("null", "unanalysed", "analysed", "partitioned")
GPU_STATES = ("analysed", "engine", "factored", "not_posdef", "downdate_failed", "batch", "batch_inverse",
              "inverse", "inverse_stale", "adjoint_seeded", "adjoint_swept")
BUF = 1 << 16   # doubles in every scratch array: far above anything a row reads or writes (asserted in Ctx)


class Ctx:
    """the arrays every row draws its arguments from; device arrays are torch tensors on the GPU and stand-in
    host arrays without one (the CPU rows return before anything is read through them)"""

    def __init__(self, lib, gpu):
        from spllt_amd import api, matgen
        self.lib, self.gpu, self.api = lib, gpu, api
        self.n, self.ptr, self.row, self.val = api.csc_lower_1based(matgen.poisson2d(8))
        self.nnz = len(self.val)
        self.opt = api.spllt_options_t.default()
        self.opt.nb, self.opt.nemin = 16, 8
        self.bad_val = self.val.copy()
        self.bad_val[self.ptr[10] - 1] = -1.0            # a negative diagonal entry: not positive definite
        self.vals3 = np.ascontiguousarray(np.stack([self.val, self.bad_val, 2.0 * self.val]))
        self.host = [np.ones(BUF) for _ in range(3)]
        self.one_col = (np.array([1, 2], dtype=np.int32), np.array([1, 0], dtype=np.int32), np.array([0.5, 0.0]))
        self.big_col = np.array([10.0, 0.0])              # A - 100 e_0 e_0^T is not positive definite
        self.bad_row = np.array([self.n + 5, 0], dtype=np.int32)
        self.i32 = np.zeros(64, dtype=np.int32)
        self.i64 = np.zeros(64, dtype=np.int64)
        self.f32 = np.zeros(BUF, dtype=np.float32)
        self.dbl = C.c_double()
        if gpu:
            import torch
            self.dev = [torch.ones(BUF, dtype=torch.float64, device="cuda") for _ in range(3)]
            self.dval = torch.tensor(self.val, device="cuda")
            self.dvals3 = torch.tensor(self.vals3, device="cuda")
        h = self.handle("analysed")
        si = api.spllt_hip_sym_info_t()
        assert lib.spllt_hip_sym_info(h[0], C.byref(si)) == 0
        self.arena = int(si.arena)
        assert 3 * max(self.arena, 2 * self.n, self.nnz) <= BUF and lib.spllt_hip_program_get(h[1], b"launches", None, 0) // 96 < BUF
        self.free(h)

    # ---- argument values ---------------------------------------------------
    def H(self, i=0):
        return self.host[i].ctypes.data_as(C.POINTER(C.c_double))

    def D(self, i=0):
        return C.c_void_p(self.dev[i].data_ptr() if self.gpu else self.host[i].ctypes.data)

    def DVAL(self):
        return C.c_void_p(self.dval.data_ptr() if self.gpu else self.val.ctypes.data)

    def DVALS3(self):
        return C.c_void_p(self.dvals3.data_ptr() if self.gpu else self.vals3.ctypes.data)

    def reset(self):
        for a in self.host:
            a.fill(1.0)
        if self.gpu:
            for d in self.dev:
                d.fill_(1.0)

    # ---- handles -------------------------------------------------------------
    def handle(self, state):
        """(akeep, fkeep) in `state`"""
        api, lib = self.api, self.lib
        ak, fk, info = C.c_void_p(None), C.c_void_p(None), api.spllt_inform_t()
        if state == "null":
            return ak, fk
        order = np.zeros(self.n, dtype=np.int32)
        ptr = self.ptr if state != "unanalysed" else np.zeros_like(self.ptr)   # (refused: ptr[0] != 1)
        lib.spllt_analyse(C.byref(ak), C.byref(fk), C.byref(self.opt), self.n, api._ip(ptr), api._ip(self.row),
                          C.byref(info), api._ip(order))
        assert info.flag == (-10 if state == "unanalysed" else 0) and fk.value
        if state in ("unanalysed", "analysed"):
            return ak, fk
        if state == "partitioned":
            assert lib.spllt_hip_set_partition(fk, 0, 2, None) == 0
            return ak, fk
        assert self.gpu, state
        if state == "engine":
            assert lib.spllt_hip_engine_stream(fk)
            return ak, fk
        val = self.bad_val if state == "not_posdef" else self.val
        lib.spllt_factor(ak, fk, C.byref(self.opt), self.nnz, api._dp(val), C.byref(info))
        assert info.flag == 0
        if state == "not_posdef":
            return ak, fk                    # (still pending: the first row that waits meets the failure)
        assert lib.spllt_hip_wait(fk) == 0
        w = self.one_col
        if state == "downdate_failed":
            assert lib.spllt_hip_updown(fk, 1, api._ip(w[0]), api._ip(w[1]), api._dp(self.big_col), -1) == -20
        if state in ("batch", "batch_inverse"):
            assert lib.spllt_hip_factor_batch(ak, fk, 3, self.nnz, self.vals3.ctypes.data, self.nnz) == -20
        if state == "batch_inverse":
            assert lib.spllt_hip_selected_inverse_batch(fk) == -20
        if state in ("inverse", "inverse_stale"):
            assert lib.spllt_hip_selected_inverse(fk) == 0
        if state == "inverse_stale":
            lib.spllt_factor(ak, fk, C.byref(self.opt), self.nnz, api._dp(self.val), C.byref(info))
            assert info.flag == 0 and lib.spllt_hip_wait(fk) == 0
        if state in ("adjoint_seeded", "adjoint_swept"):
            assert lib.spllt_hip_factor_adjoint_seed(fk, 1, self.H(0), self.H(1), self.n, 1.0, 0, 0) == 0
        if state == "adjoint_swept":
            assert lib.spllt_hip_factor_adjoint(fk, self.H(2)) == 0
        return ak, fk

    def free(self, h):
        st = C.c_int()
        if h[1]:
            self.lib.spllt_deallocate_fkeep(C.byref(h[1]), C.byref(st))
        if h[0]:
            self.lib.spllt_deallocate_akeep(C.byref(h[0]), C.byref(st))


# ---- the entry points -------------------------------------------------------------------------------------
# name -> (good, bad, flags): good(c) gives the arguments after fkeep; bad maps a variant to {position: value}
# (a value may be a function of c).  Flags: "m" an accepted call changes the handle's state (it gets a fresh
# handle); "e" an accepted call creates the engine although the handle is partitioned, "s" only on an
# unpartitioned handle (both: no such row without a GPU); "a" akeep goes in front of fkeep; "p" returns a
# pointer (recorded as 0 / 1); "r" a release (runs last).
ENTRIES = {}


def entry(name, good, bad=None, flags=""):
    ENTRIES["spllt_hip_" + name] = (good, bad or {}, flags)


_vec = {"null": {1: None}, "negative": {0: -1}, "short_ld": {2: lambda c: c.n - 1}}
_job = dict(_vec, job={3: 3})
for _n in ("solve_many", "solve_repro", "factor_mult"):
    entry(_n, lambda c: [2, c.H(), c.n, 0], _job)
    entry(_n + "_dev", lambda c: [2, c.D(), c.n, 0, 0], _job)
entry("sample", lambda c: [2, c.H(), c.n, 0, 1, 0, None], dict(_vec, kind={3: 2}))
entry("sample_dev", lambda c: [2, c.D(), c.n, 0, 1, 0, None], dict(_vec, kind={3: 2}))
entry("white_noise_dev", lambda c: [2, c.D(), c.n, 1, 0], _vec)
entry("set_reproducible_solve", lambda c: [0], {"on": {0: 1}})

_fb = {"null": {2: None}, "negative": {0: -1}, "nnz": {1: lambda c: c.nnz - 1}, "short_ld": {3: lambda c: c.nnz - 1},
       "empty": {0: 0}}
entry("factor_batch", lambda c: [3, c.nnz, C.c_void_p(c.vals3.ctypes.data), c.nnz], _fb, "mas")
entry("factor_batch_dev", lambda c: [3, c.nnz, c.DVALS3(), c.nnz], _fb, "mas")
entry("batch_status", lambda c: [None, None, 0])
entry("solve_batch", lambda c: [2, C.c_void_p(c.host[0].ctypes.data), c.n, 0], dict(_job, empty={0: 0}))
entry("solve_batch_dev", lambda c: [2, c.D(), c.n, 0, 0], dict(_job, empty={0: 0}))
_member = {"null": {1: None}, "negative": {2: -1}, "member": {0: 7}}
entry("get_factor_batch", lambda c: [0, c.H(), c.arena], _member)
entry("device_factor_batch", lambda c: [c.i64.ctypes.data_as(C.POINTER(C.c_int64))], flags="p")
entry("log_det_batch", lambda c: [c.H()], {"null": {0: None}})
entry("batch_launches", lambda c: [])
entry("selected_inverse_batch", lambda c: [], flags="m")
entry("get_inverse_batch", lambda c: [0, c.H(), c.arena], dict(_member, failed_member={0: 1}))
entry("device_inverse_batch", lambda c: [c.i64.ctypes.data_as(C.POINTER(C.c_int64))], flags="p")
entry("inverse_diag_batch", lambda c: [c.H(), c.n], {"null": {0: None}, "short_ld": {1: lambda c: c.n - 1}})
entry("inverse_on_pattern_batch", lambda c: [c.H(), c.nnz], {"null": {0: None}, "short_ld": {1: lambda c: c.nnz - 1}})
entry("inverse_on_pattern_batch_dev", lambda c: [c.D(), c.nnz], {"null": {0: None}, "short_ld": {1: lambda c: c.nnz - 1}})
entry("batch_selinv_launches", lambda c: [])

_mv = {"null_val": {1: None}, "null_x": {3: None}, "null_y": {5: None}, "negative": {2: -1},
       "short_ldx": {4: lambda c: c.n - 1}, "short_ldy": {6: lambda c: c.n - 1}, "nnz": {0: lambda c: c.nnz + 1},
       "empty": {2: 0}}
entry("matvec", lambda c: [c.nnz, c.api._dp(c.val), 2, c.H(0), c.n, c.H(1), c.n], _mv, "s")
entry("matvec_dev", lambda c: [c.nnz, c.DVAL(), 2, c.D(0), c.n, c.D(1), c.n, 0], _mv, "s")
_rf = {"null_val": {1: None}, "null_x": {3: None}, "negative": {2: -1}, "short_ld": {4: lambda c: c.n - 1},
       "method": {5: 2}, "tol": {6: 0.0}, "max_iter": {7: -1}, "nnz": {0: lambda c: c.nnz + 1}, "empty": {2: 0}}
entry("solve_refined", lambda c: [c.nnz, c.api._dp(c.val), 2, c.H(), c.n, 1, 1e-10, 20, c.api._ip(c.i32), c.H(1)], _rf)
entry("solve_refined_dev", lambda c: [c.nnz, c.DVAL(), 2, c.D(), c.n, 1, 1e-10, 20, c.api._ip(c.i32), c.H(1)], _rf)

_w = lambda c: [1, c.api._ip(c.one_col[0]), c.api._ip(c.one_col[1])]   # noqa: E731
_badrow = {2: lambda c: c.api._ip(c.bad_row)}
entry("updown_plan", lambda c: _w(c) + [None, 0], {"row": _badrow})
entry("updown", lambda c: _w(c) + [c.api._dp(c.one_col[2]), 1], {"sign": {4: 0}, "null": {3: None}, "row": _badrow}, "ms")
entry("updown_time", lambda c: [C.byref(c.dbl)], {"null": {0: None}})
entry("updown_info", lambda c: [c.i64.ctypes.data_as(C.POINTER(C.c_int64))], {"null": {0: None}})
_sp = lambda c: _w(c) + [c.api._dp(c.one_col[2]), -1, None]   # noqa: E731
_spbad = {"null": {6: None}, "job": {8: 3}, "row": _badrow, "null_val": {3: None}, "short_ld": {7: lambda c: c.n - 1}}
entry("solve_sparse", lambda c: _sp(c) + [c.H(), c.n, 0], _spbad, "s")
entry("solve_sparse_dev", lambda c: _sp(c) + [c.D(), c.n, 0], _spbad, "s")
entry("gram_sparse", lambda c: _w(c) + [c.api._dp(c.one_col[2]), c.H(), 1],
      {"null": {4: None}, "row": _badrow, "null_val": {3: None}, "short_ld": {5: 0}}, "s")
entry("solve_sparse_plan", lambda c: _w(c) + [-1, None, 0, None, 0, None, 0, c.i64.ctypes.data_as(C.POINTER(C.c_int64))],
      {"null": {10: None}, "job": {5: 3}, "row": _badrow})
entry("solve_sparse_info", lambda c: [c.i64.ctypes.data_as(C.POINTER(C.c_int64))], {"null": {0: None}})

entry("selected_inverse", lambda c: [], flags="m")
entry("get_inverse", lambda c: [c.H(), c.arena], {"null": {0: None}})
entry("device_inverse", lambda c: [], flags="p")
entry("inverse_diag", lambda c: [c.H(), c.n], {"null": {0: None}, "n": {1: lambda c: c.n - 1}})
entry("inverse_on_pattern", lambda c: [c.H()], {"null": {0: None}})
entry("inverse_on_pattern_dev", lambda c: [c.D()], {"null": {0: None}})
entry("log_det", lambda c: [C.byref(c.dbl)], {"null": {0: None}})
entry("factor_serial", lambda c: [0], {"which": {0: 2}})
_po = {"null": {1: None}, "null_out": {6: None}, "negative": {0: -1}, "short_ldu": {2: lambda c: c.n - 1},
       "short_ldv": {4: lambda c: c.n - 1}}
entry("pattern_outer", lambda c: [2, c.H(0), c.n, c.H(1), c.n, 1.0, c.H(2)], _po, "s")
entry("pattern_outer_dev", lambda c: [2, c.D(0), c.n, c.D(1), c.n, 1.0, c.D(2)], _po, "s")
entry("pattern_outer_batch_dev", lambda c: [2, 2, c.D(0), c.n, c.D(1), c.n, 1.0, c.D(2), c.nnz],
      {"null": {2: None}, "null_out": {7: None}, "negative_batch": {0: -1}, "negative": {1: -1},
       "short_ldu": {3: lambda c: c.n - 1}, "short_ldout": {8: lambda c: c.nnz - 1}, "empty": {0: 0}}, "s")

_seed = {"null": {1: None}, "negative": {0: -1}, "short_ld": {3: lambda c: c.n - 1}, "accumulate": {5: 2}, "flags": {6: 4}}
entry("factor_adjoint_seed", lambda c: [2, c.H(0), c.H(1), c.n, 1.0, 0, 0], _seed, "m")
entry("factor_adjoint_seed_dev", lambda c: [2, c.D(0), c.D(1), c.n, 1.0, 0, 0], _seed, "m")
entry("set_factor_adjoint", lambda c: [c.H(), c.arena], {"null": {0: None}, "short": {1: lambda c: c.arena - 1}}, "m")
entry("get_factor_adjoint", lambda c: [c.H(), c.arena], {"null": {0: None}})
entry("device_factor_adjoint", lambda c: [], flags="p")
entry("factor_adjoint", lambda c: [c.H()], {"null": {0: None}}, "m")
entry("factor_adjoint_dev", lambda c: [c.D()], {"null": {0: None}}, "m")

# the plain setters and getters: one accepted call (and the argument their own check names)
entry("factor_dev", None, {"null": None, "nnz": None}, "mae")     # (through info->flag: see call())
entry("wait", lambda c: [])
entry("get_factor", lambda c: [c.H(), c.arena], {"null": {0: None}})
entry("device_factor", lambda c: [], flags="p")
entry("factor_times", lambda c: [None, None, None, None])
entry("program_get", lambda c: [b"launches", None, 0], {"name": {0: b"nonsense"}, "null": {0: None}})
entry("partition_get", lambda c: [b"owner", None, 0], {"name": {0: b"nonsense"}, "null": {0: None}})
entry("solve_dev", lambda c: [c.D(), 1, 0, -1], {"null": {0: None}})
entry("set_engine", lambda c: [0, 0, 0], flags="m")
entry("set_chain_block", lambda c: [1], {"zero": {0: 0}}, "m")
entry("set_partition", lambda c: [0, 1, None], {"nranks": {1: 0}, "rank": {0: 1}}, "m")
entry("set_exchange_buffer", lambda c: [None])
entry("set_communicator", lambda c: [None], flags="e")
entry("engine_stream", lambda c: [], flags="pe")
entry("exchange_stream", lambda c: [], flags="pe")
entry("pending_exchange", lambda c: [])
entry("continue", lambda c: [], flags="m")     # (a refused call leaves its flag in last_flag)
_prof = {"null": {0: None}}
entry("profile", lambda c: [c.api._dp(c.val), c.nnz, c.f32.ctypes.data_as(C.POINTER(C.c_float)), BUF], _prof, "me")
entry("profile_in_program", lambda c: [c.api._dp(c.val), c.nnz, c.f32.ctypes.data_as(C.POINTER(C.c_float)), BUF], _prof, "me")
entry("timeline", lambda c: [c.api._dp(c.val), c.nnz, c.f32.ctypes.data_as(C.POINTER(C.c_float)), BUF], _prof, "me")
entry("last_flag", lambda c: [])
entry("last_error", lambda c: [], flags="p")
for _n in ("solve_repro", "factor_mult", "refine", "solve_sparse", "batch", "inverse_batch", "inverse", "factor_adjoint"):
    # ("fresh": on a handle of its own, whose factorization -- failed in state not_posdef -- may still be pending)
    entry("release_" + _n, lambda c: [], {"fresh": {}}, flags="r")


def takes_fkeep():
    """the spllt_hip_* functions of include/spllt_hip.h with a `void* fkeep` parameter"""
    import re
    txt = open(os.path.join(ROOT, "include", "spllt_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    txt = re.sub(r"//[^\n]*", "", txt)
    return {m.group(1) for m in re.finditer(r"\b(spllt_hip_\w+)\s*\(([^;{]*)\)\s*;", txt)
            if re.search(r"\bvoid\s*\*\s*fkeep\b", m.group(2))}


def call(c, name, h, variant):
    """one row: [rc, last_error or None]"""
    good, bad, flags = ENTRIES[name]
    lib, fk = c.lib, h[1]
    if name == "spllt_hip_factor_dev":
        info = c.api.spllt_inform_t()
        lib.spllt_hip_factor_dev(h[0], fk, C.byref(c.opt), c.nnz - 1 if variant == "nnz" else c.nnz,
                                 None if variant == "null" else c.DVAL(), C.byref(info))
        rc = int(info.flag)
        if fk:
            lib.spllt_hip_wait(fk)
    else:
        args = good(c)
        for pos, v in bad.get(variant, {}).items():
            args[pos] = v(c) if callable(v) else v
        rc = getattr(lib, name)(*(([h[0]] if "a" in flags else []) + [fk] + args))
        rc = int(bool(rc)) if "p" in flags else int(rc)
    err = (lib.spllt_hip_last_error(fk) or b"").decode() if (rc < 0 or rc == 1) and "p" not in flags else None
    return [rc, err]


def runs(name, state, variant, gpu):
    """whether the row exists: without a GPU none that would create an engine"""
    flags = ENTRIES[name][2]
    if gpu or variant != "good":
        return True
    return not (("e" in flags and state in ("analysed", "partitioned")) or ("s" in flags and state == "analysed"))


def run_table(lib, gpu):
    """every row of the CPU or of the GPU table, in order: {"entry|state|variant": [rc, last_error]}"""
    c = Ctx(lib, gpu)
    out = {}
    for state in (GPU_STATES if gpu else CPU_STATES):
        shared = c.handle(state)
        order = [n for n in ENTRIES if "r" not in ENTRIES[n][2]] + [n for n in ENTRIES if "r" in ENTRIES[n][2]]
        for name in order:
            _, bad, flags = ENTRIES[name]
            for variant in list(bad) + ["good"]:
                if not runs(name, state, variant, gpu):
                    continue
                c.reset()
                fresh = variant == "fresh" or (variant == "good" and ("m" in flags or (gpu and state == "analysed")))
                h = c.handle(state) if fresh else shared
                out[f"{name}|{state}|{variant}"] = call(c, name, h, variant)
                if fresh:
                    c.free(h)
        c.free(shared)
    return out


def pack(table):
    """the table as it is stored: every distinct message once, one line per (state, entry point)"""
    msgs = sorted({e for _, e in table.values() if e is not None})
    rows = {}
    for key, (rc, err) in table.items():
        name, state, variant = key.split("|")
        rows.setdefault(state, {}).setdefault(name, {})[variant] = rc if err is None else [rc, msgs.index(err)]
    lines = ['{"messages": [\n' + ",\n".join(json.dumps(m) for m in msgs) + '\n], "rows": {']
    for i, (state, ents) in enumerate(rows.items()):
        body = ",\n".join(f"{json.dumps(n)}: {json.dumps(v)}" for n, v in ents.items())
        lines.append(f"{json.dumps(state)}: {{\n{body}\n}}" + ("," if i + 1 < len(rows) else ""))
    return "\n".join(lines) + "\n}}\n"


def unpack(doc):
    """the stored table as run_table() returns it"""
    return {f"{name}|{state}|{variant}": [v, None] if isinstance(v, int) else [v[0], doc["messages"][v[1]]]
            for state, ents in doc["rows"].items() for name, vs in ents.items() for variant, v in vs.items()}


def load_library(path=None):
    from spllt_amd import _lib
    if path:
        _lib.LIB_PATH = os.path.abspath(path)
    return _lib.load()


if __name__ == "__main__":
    import argparse
    import time
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", action="store_true")
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--lib", default=None, help="the library to record from (of the commit before the change)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    os.environ.setdefault("SPLLT_CHAIN_GRAPH_SERIAL", "0")   # (as tests/conftest.py sets it)
    t0 = time.time()
    table = run_table(load_library(a.lib), a.gpu)
    print(f"{len(table)} rows in {time.time() - t0:.1f} s")
    if a.record:
        with open(a.out or GOLDEN[a.gpu], "w") as fh:
            fh.write(pack(table))
