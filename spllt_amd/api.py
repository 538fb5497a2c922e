"""Host-side mirror of SpLLT's user API over the C-ABI of libspllt_hip.so.

Function names, argument meaning and error behaviour follow the reference
(``spllt_analyse`` src/spllt_analyse_mod.F90:23, ``spllt_factor``
src/spllt_mod.F90:141, ``spllt_wait`` :172, ``spllt_solve``
src/spllt_solve_mod.F90:8-12; C forms include/spllt_iface.h:59-148):
1-based CSC of the lower triangle, status in ``info.flag``, factor is
asynchronous until ``wait``.  All numerical work happens behind the C-ABI in
hand-written HIP; this file only marshals arrays.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import spllt_hip_sym_info_t, spllt_inform_t, spllt_options_t

_I32 = ("order", "sptr", "sparent", "rlist", "small", "level", "bcol_node", "bcol_width",
        "bcol_r0", "bcol_nrow", "node_bcol0")
_I64 = ("rptr", "bcol_off", "map_dst", "map_src", "lmap_ptr", "weight")

UPD_UNIT_DTYPE = np.dtype([
    ("d_off", "<i8"), ("relrow_off", "<i8"), ("gcol_off", "<i8"), ("dinv_off", "<i8"),
    ("src_bcol0", "<i4"), ("nseg", "<i4"), ("seg_r0", "<i4"), ("seg_stride", "<i4"),
    ("src_r0", "<i4"), ("src_c0", "<i4"), ("M", "<i4"), ("N", "<i4"), ("k0", "<i4"),
    ("klen", "<i4"), ("d_ld", "<i4"), ("d_row0", "<i4"), ("d_col0", "<i4"), ("mode", "<i4"),
    ("dinv_ld", "<i4"), ("lower", "<i4"), ("b_bcol0", "<i4"), ("b_seg_r0", "<i4"),
    ("atomic", "<i4"), ("a_w", "<i4"), ("a_off", "<i8")])
UPD_TILE_DTYPE = np.dtype([("unit", "<i4"), ("ti", "<i2"), ("tj", "<i2")])
CHAIN_UNIT_DTYPE = np.dtype([("off", "<i8"), ("winv_off", "<i8"), ("ld", "<i4"), ("c0", "<i4"),
                             ("pn", "<i4"), ("cs", "<i4"), ("ce", "<i4"), ("gcol", "<i4")])
PANEL_UNIT_DTYPE = np.dtype([("off", "<i8"), ("dinv_off", "<i8"),
                             ("ld", "<i4"), ("c0", "<i4"), ("pn", "<i4"), ("next_pn", "<i4"),
                             ("nrow", "<i4"), ("gcol", "<i4"), ("ntile", "<i4"), ("pad_", "<i4")])
SUB_TASK_DTYPE = np.dtype([("g_off", "<i8"), ("node_first", "<i4"), ("node_count", "<i4"), ("g_n", "<i4"),
                           ("pad_", "<i4")])
SUB_NODE_DTYPE = np.dtype([("off", "<i8"), ("dinv_off", "<i8"), ("w", "<i4"), ("nrow", "<i4"), ("gcol", "<i4"),
                           ("unit_first", "<i4"), ("unit_count", "<i4"), ("root", "<i4")])
GATHER_ITEM_DTYPE = np.dtype([("buf_off", "<i8"), ("relrow_off", "<i8"), ("gcol_off", "<i8"), ("ld", "<i4"),
                              ("i0", "<i4"), ("i1", "<i4"), ("j0", "<i4"), ("j1", "<i4"),
                              ("diag_shift", "<i4"), ("lower", "<i4"), ("pad_", "<i4")])
GATHER_TILE_DTYPE = np.dtype([("d_off", "<i8"), ("d_ld", "<i4"), ("row0", "<i4"), ("col0", "<i4"),
                              ("rows", "<i4"), ("cols", "<i4"), ("drow_base", "<i4"),
                              ("dcol_base", "<i4"), ("first", "<i4"), ("count", "<i4"), ("pad_", "<i4")])
# "launches": int64 x 12 per launch
LAUNCH_COLS = ("kind", "level", "first", "count", "tile", "flops", "stream", "record",
               "wait0", "wait1", "wait2", "wait3")
SOLVE_UNIT_DTYPE = np.dtype([("off", "<i8"), ("dinv_off", "<i8"), ("idx_off", "<i8"), ("w", "<i4"),
                             ("nrow", "<i4"), ("pw", "<i4"), ("cb", "<i4"), ("gcol0", "<i4"), ("pad_", "<i4")])
# selected inversion (schedule.hpp SelinvUnit / SelinvRow); "selinv_launches": int64 x 5 per launch
SELINV_UNIT_DTYPE = np.dtype([("off", "<i8"), ("dinv_off", "<i8"), ("row_off", "<i8"), ("y_off", "<i8"),
                              ("p_off", "<i8"), ("ld", "<i4"), ("c0", "<i4"), ("pn", "<i4"), ("dinv_ld", "<i4"),
                              ("nR", "<i4"), ("rbase", "<i4"), ("ntile", "<i4"), ("nsplit", "<i4"),
                              ("kslice", "<i4"), ("gcol", "<i4"), ("ncol", "<i4"), ("nb", "<i4")])
SELINV_ROW_DTYPE = np.dtype([("cbase", "<i8"), ("ld", "<i4"), ("map", "<i4")])
SELINV_LAUNCH_COLS = ("kind", "level", "first", "count", "flops")
POTRF_UNIT_DTYPE = np.dtype([("off", "<i8"), ("dinv_off", "<i8"), ("ld", "<i4"), ("n", "<i4"),
                             ("gcol", "<i4"), ("flags", "<i4")])


class SplltError(RuntimeError):
    def __init__(self, where, flag, msg=""):
        super().__init__(f"{where}: info.flag = {flag} {msg}".strip())
        self.flag = flag


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def csc_lower_1based(A):
    """scipy sparse (symmetric, any format) -> (n, ptr, row, val) of the lower
    triangle, 1-based int32, as the C-ABI expects (example/C/simple.c:37-44)."""
    import scipy.sparse as sp
    L = sp.tril(sp.csc_matrix(A), format="csc")
    L.sort_indices()
    return (L.shape[0], (L.indptr + 1).astype(np.int32), (L.indices + 1).astype(np.int32),
            np.ascontiguousarray(L.data, dtype=np.float64))


class Factorization:
    """One analysed pattern: owns the akeep/fkeep handle pair."""

    def __init__(self, n, ptr, row, nb=256, nemin=32, prune_tree=True, ncpu=1, order=None,
                 panel_width=None, tile=None, engine_flags=0, chain_block=None, symbolic=None):
        """symbolic: optional dict with the SSIDS-style quintuple (0-based numpy arrays
        "sptr", "sparent", "rptr", "rlist", "order"): the analyse then takes exactly this
        supernode partition and tree (spllt_hip_analyse_symbolic)."""
        self.lib = _lib.load()
        self.n = int(n)
        self.ptr = np.ascontiguousarray(ptr, dtype=np.int32)
        self.row = np.ascontiguousarray(row, dtype=np.int32)
        self.nnz = int(self.ptr[n] - 1) if n > 0 else 0
        self.options = spllt_options_t.default()
        self.options.nb = nb
        self.options.nemin = nemin
        self.options.prune_tree = 1 if prune_tree else 0
        self.options.ncpu = ncpu
        self.akeep = C.c_void_p(None)
        self.fkeep = C.c_void_p(None)
        self.info = spllt_inform_t()
        self.order = np.zeros(max(n, 1), dtype=np.int32)
        if symbolic is not None:
            sy = symbolic
            sp = np.ascontiguousarray(np.asarray(sy["sptr"]) + 1, dtype=np.int32)
            spar = np.ascontiguousarray(np.asarray(sy["sparent"]) + 1, dtype=np.int32)
            rp = np.ascontiguousarray(np.asarray(sy["rptr"]) + 1, dtype=np.int64)
            rl = np.ascontiguousarray(np.asarray(sy["rlist"]) + 1, dtype=np.int32)
            oin = np.ascontiguousarray(np.asarray(sy["order"]) + 1, dtype=np.int32)
            self.lib.spllt_hip_analyse_symbolic(C.byref(self.akeep), C.byref(self.fkeep),
                                                C.byref(self.options), n, _ip(self.ptr), _ip(self.row),
                                                C.byref(self.info), len(spar), _ip(sp), _ip(spar),
                                                rp.ctypes.data_as(C.POINTER(C.c_int64)), _ip(rl), _ip(oin))
            self.order[:n] = oin[:n]
        elif order is None:
            self.lib.spllt_analyse(C.byref(self.akeep), C.byref(self.fkeep), C.byref(self.options),
                                   n, _ip(self.ptr), _ip(self.row), C.byref(self.info),
                                   _ip(self.order))
        else:
            oin = np.ascontiguousarray(order, dtype=np.int32)
            self.lib.spllt_hip_analyse_ordered(C.byref(self.akeep), C.byref(self.fkeep),
                                               C.byref(self.options), n, _ip(self.ptr),
                                               _ip(self.row), C.byref(self.info), _ip(self.order),
                                               _ip(oin))
        if self.info.flag < 0:
            raise SplltError("spllt_analyse", self.info.flag)
        if panel_width or tile or engine_flags:
            self.lib.spllt_hip_set_engine(self.fkeep, panel_width or 0, tile or 0, engine_flags)
        if chain_block:
            self.lib.spllt_hip_set_chain_block(self.fkeep, int(chain_block))
        self._val_keepalive = None

    # ---- symbolic introspection ------------------------------------------
    def sym_info(self):
        si = spllt_hip_sym_info_t()
        rc = self.lib.spllt_hip_sym_info(self.akeep, C.byref(si))
        if rc:
            raise SplltError("spllt_hip_sym_info", rc)
        d = {k: getattr(si, k) for k, _ in si._fields_}
        d["ordering"] = si.ordering.decode()
        return d

    def sym(self, name):
        dt = np.int32 if name in _I32 else np.int64
        if name not in _I32 and name not in _I64:
            raise KeyError(name)
        cnt = self.lib.spllt_hip_sym_get(self.akeep, name.encode(), None, 0)
        if cnt < 0:
            raise KeyError(name)
        out = np.zeros(max(cnt, 1), dtype=dt)
        self.lib.spllt_hip_sym_get(self.akeep, name.encode(), out.ctypes.data, cnt)
        return out[:cnt]

    def program(self, name):
        nbytes = self.lib.spllt_hip_program_get(self.fkeep, name.encode(), None, 0)
        if nbytes < 0:
            raise KeyError(name)
        raw = np.zeros(max(nbytes, 1), dtype=np.uint8)
        self.lib.spllt_hip_program_get(self.fkeep, name.encode(), raw.ctypes.data, nbytes)
        raw = raw[:nbytes]
        if name in ("solve_sparse_host_us", "solve_sparse_batch_host_us"):
            return int(raw.view(np.int64)[0])
        if name == "owned":              # entries of the engine's ledger of device buffers, their bytes
            return raw.view(np.int64)
        if name == "matvec_rowptr":      # the operator of the refined solves
            return raw.view(np.int64)
        if name in ("matvec_col", "matvec_src"):
            return raw.view(np.int32)
        if name.startswith("bsolve_"):   # the batch's substitution program: the layouts of "solve_*"
            name = name[1:]
        if name.startswith("batch_"):    # the batch program: the layouts of the unprefixed names
            name = name[len("batch_"):]
            if name.startswith("det_"):  # ... and those of its deterministic form
                name = name[len("det_"):]
        if name == "launches":
            return raw.view(np.int64).reshape(-1, len(LAUNCH_COLS))
        if name == "units":
            return raw.view(UPD_UNIT_DTYPE)
        if name == "tiles":
            return raw.view(UPD_TILE_DTYPE)
        if name == "potrf":
            return raw.view(POTRF_UNIT_DTYPE)
        if name == "chains":
            return raw.view(CHAIN_UNIT_DTYPE)
        if name == "panels":
            return raw.view(PANEL_UNIT_DTYPE)
        if name == "sub_tasks":
            return raw.view(SUB_TASK_DTYPE)
        if name == "sub_nodes":
            return raw.view(SUB_NODE_DTYPE)
        if name == "exchanges":
            return raw.view(np.int64).reshape(-1, 5)
        if name == "xitems":
            return raw.view(np.int64).reshape(-1, 6)
        if name == "xbuf_elems":
            return int(raw.view(np.int64)[0])
        if name in ("chain_block", "scratch_size", "panel_width", "gen_size"):
            return int(raw.view(np.int64)[0])
        if name == "gather_tiles":
            return raw.view(GATHER_TILE_DTYPE)
        if name == "gather_items":
            return raw.view(GATHER_ITEM_DTYPE)
        if name == "relpos":
            return raw.view(np.int32)
        if name == "dinv_size":
            return int(raw.view(np.int64)[0])
        if name == "solve_units":
            return raw.view(SOLVE_UNIT_DTYPE)
        if name == "solve_list":
            return raw.view(np.int32)
        if name == "solve_tiles":
            return raw.view(UPD_TILE_DTYPE)
        if name in ("solve_fwd", "solve_bwd"):
            return raw.view(np.int64).reshape(-1, 4)
        if name == "solve_split":
            return raw.view(np.int64)
        if name in ("rsolve_fslot", "rsolve_bfirst", "rsolve_gptr", "rsolve_gsrc", "rsolve_bslot"):
            return raw.view(np.int64)
        if name in ("rsolve_frows", "rsolve_bsize"):
            return int(raw.view(np.int64)[0])
        if name == "selinv_units":
            return raw.view(SELINV_UNIT_DTYPE)
        if name == "selinv_tiles":
            return raw.view(UPD_TILE_DTYPE)
        if name == "selinv_rows":
            return raw.view(SELINV_ROW_DTYPE)
        if name == "selinv_relpos":
            return raw.view(np.int32)
        if name == "selinv_diag":
            return raw.view(np.int64)
        if name == "selinv_launches":
            return raw.view(np.int64).reshape(-1, len(SELINV_LAUNCH_COLS))
        if name == "selinv_scratch":
            return int(raw.view(np.int64)[0])
        if name == "selinv_flops":
            return float(raw.view(np.float64)[0])
        return raw

    # ---- numerical phases --------------------------------------------------
    def factor(self, val):
        """spllt_factor: asynchronous; call wait() before using L."""
        val = np.ascontiguousarray(val, dtype=np.float64)
        self._val_keepalive = val  # `val` must outlive the submission
        self.lib.spllt_factor(self.akeep, self.fkeep, C.byref(self.options), self.nnz, _dp(val),
                              C.byref(self.info))
        if self.info.flag < 0:
            raise SplltError("spllt_factor", self.info.flag, self.last_error())
        return self

    def factor_dev(self, val_dev_ptr):
        """spllt_factor with `val` already in HBM (integer device pointer)."""
        self.lib.spllt_hip_factor_dev(self.akeep, self.fkeep, C.byref(self.options), self.nnz,
                                      C.c_void_p(val_dev_ptr), C.byref(self.info))
        if self.info.flag < 0:
            raise SplltError("spllt_factor", self.info.flag, self.last_error())
        return self

    def wait(self):
        rc = self.lib.spllt_hip_wait(self.fkeep)
        self._val_keepalive = None
        if rc < 0:
            raise SplltError("spllt_wait", rc, self.last_error())
        return self

    def times(self):
        s, d, h = C.c_double(), C.c_double(), C.c_double()
        nl = C.c_int()
        self.lib.spllt_hip_factor_times(self.fkeep, C.byref(s), C.byref(d), C.byref(h), C.byref(nl))
        return {"submit_ms": s.value, "device_ms": d.value, "h2d_ms": h.value,
                "launches": nl.value}

    def get_factor(self, out=None):
        """the factor's arena on the host; out: an existing float64 array of that length to fill
        (a fresh one pays its page faults during the copy)"""
        arena = self.sym_info()["arena"]
        if out is None:
            out = np.zeros(max(arena, 1), dtype=np.float64)
        assert out.dtype == np.float64 and out.size >= arena and out.flags["C_CONTIGUOUS"]
        self._call("spllt_hip_get_factor", self.fkeep, _dp(out), arena)
        return out[:arena]

    def device_factor_ptr(self):
        return self.lib.spllt_hip_device_factor(self.fkeep)

    # ---- selected inversion ---------------------------------------------------
    def selected_inverse(self):
        """spllt_hip_selected_inverse: Z = (P A P^T)^-1 on the pattern of L, on the device"""
        self._call("spllt_hip_selected_inverse", self.fkeep)
        return self

    def get_inverse(self, out=None):
        """the Z arena on the host (L's layout, see get_factor)"""
        arena = self.sym_info()["arena"]
        if out is None:
            out = np.zeros(max(arena, 1), dtype=np.float64)
        assert out.dtype == np.float64 and out.size >= arena and out.flags["C_CONTIGUOUS"]
        self._call("spllt_hip_get_inverse", self.fkeep, _dp(out), arena)
        return out[:arena]

    def device_inverse_ptr(self):
        return self.lib.spllt_hip_device_inverse(self.fkeep)

    def inverse_diag(self):
        """(A^-1)_ii in the user's variable order"""
        out = np.zeros(max(self.n, 1), dtype=np.float64)
        self._call("spllt_hip_inverse_diag", self.fkeep, _dp(out), self.n)
        return out[:self.n]

    def log_det(self):
        """log det A of the last factorization (2 sum log L_jj)"""
        v = C.c_double()
        self._call("spllt_hip_log_det", self.fkeep, C.byref(v))
        return v.value

    def inverse_on_pattern(self):
        """(A^-1) at the entries of the analysed CSC-lower pattern, nnz values in the order of val"""
        out = np.zeros(max(self.nnz, 1), dtype=np.float64)
        self._call("spllt_hip_inverse_on_pattern", self.fkeep, _dp(out))
        return out[:self.nnz]

    def inverse_on_pattern_dev(self, out_dev_ptr):
        """spllt_hip_inverse_on_pattern_dev: the same nnz values into device memory (integer device pointer)"""
        self._call("spllt_hip_inverse_on_pattern_dev", self.fkeep, C.c_void_p(out_dev_ptr))
        return self

    def factor_serial(self, which=0):
        """spllt_hip_factor_serial: how often the single factor (which=0) or the batch (which=1) has been
        changed successfully on this handle; needs no device"""
        return int(self.lib.spllt_hip_factor_serial(self.fkeep, int(which)))

    # ---- sampled outer product on the pattern ---------------------------------
    def pattern_tables(self):
        """(row, col) int32 per entry of val, 0-based user variables ("pattern_row" / "pattern_col" of
        spllt_hip_program_get); needs no device"""
        return self.program("pattern_row").view(np.int32), self.program("pattern_col").view(np.int32)

    def pattern_outer(self, u, v, alpha=1.0):
        """spllt_hip_pattern_outer on host arrays u, v of shape (n,) or (n, nvec): out[k] = alpha sum_q
        (u_q[i] v_q[j] + [i != j] u_q[j] v_q[i]) at the k-th entry (i, j) of the analysed pattern"""
        u = np.asfortranarray(np.asarray(u, dtype=np.float64).reshape(self.n, -1))
        v = np.asfortranarray(np.asarray(v, dtype=np.float64).reshape(self.n, -1))
        if u.shape != v.shape:
            raise ValueError("pattern_outer: u and v must have the same shape")
        out = np.zeros(max(self.nnz, 1), dtype=np.float64)
        self._call("spllt_hip_pattern_outer", self.fkeep, u.shape[1], _dp(u), max(self.n, 1), _dp(v), max(self.n, 1),
                   float(alpha), _dp(out))
        return out[:self.nnz]

    def pattern_outer_dev(self, u_dev_ptr, v_dev_ptr, nvec, out_dev_ptr, ldu=None, ldv=None, alpha=1.0):
        """spllt_hip_pattern_outer_dev: device vectors (vector q at u[q*ldu .. + n), ld defaults to n), nnz
        doubles written at out_dev_ptr"""
        self._call("spllt_hip_pattern_outer_dev", self.fkeep, int(nvec), C.c_void_p(u_dev_ptr),
                   int(self.n if ldu is None else ldu), C.c_void_p(v_dev_ptr),
                   int(self.n if ldv is None else ldv), float(alpha),
                   C.c_void_p(out_dev_ptr))
        return self

    def pattern_outer_batch_dev(self, u_dev_ptr, v_dev_ptr, nbatch, nvec, out_dev_ptr, ldu=None, ldv=None, ldout=None,
                                alpha=1.0):
        """spllt_hip_pattern_outer_batch_dev: vector q of member b at u[(b*nvec + q)*ldu ..], out[b*ldout + k]"""
        self._call("spllt_hip_pattern_outer_batch_dev", self.fkeep, int(nbatch), int(nvec), C.c_void_p(u_dev_ptr),
                   int(self.n if ldu is None else ldu), C.c_void_p(v_dev_ptr),
                   int(self.n if ldv is None else ldv), float(alpha),
                   C.c_void_p(out_dev_ptr), int(self.nnz if ldout is None else ldout))
        return self

    def release_inverse(self):
        self._call("spllt_hip_release_inverse", self.fkeep)

    def inverse_entries(self, i, j, Z=None):
        """(A^-1)_{ij} for 0-based user indices i, j (scalars or arrays) whose pivot pair lies in the
        pattern of L; ValueError for a pair outside it (inverse_block(i, j) is the route for those: sparse
        solves with unit columns).  Z: the host Z arena (get_inverse()) to read, fetched when not given."""
        i, j = np.broadcast_arrays(np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64))
        if ((i < 0) | (i >= self.n) | (j < 0) | (j >= self.n)).any():
            raise ValueError("inverse_entries: index out of range")
        if Z is None:
            Z = self.get_inverse()
        pos = self._inverse_positions(i.ravel(), j.ravel())
        return Z[pos].reshape(i.shape)

    def _inverse_positions(self, i, j):
        """arena positions of the pivot pairs of user indices (i, j): one global search over the row
        lists, keyed by (node, row) -- the lists are sorted inside a node and the nodes follow in order"""
        if getattr(self, "_pattern", None) is None:
            t = {k: self.sym(k) for k in ("order", "sptr", "rptr", "rlist", "node_bcol0", "bcol_off",
                                          "bcol_width", "bcol_r0")}
            nn = len(t["sptr"]) - 1
            node_of = np.repeat(np.arange(nn), np.diff(t["sptr"]))
            keys = np.repeat(np.arange(nn, dtype=np.int64), np.diff(t["rptr"])) * (self.n + 1) + t["rlist"]
            self._pattern = (t, node_of, keys)
        t, node_of, keys = self._pattern
        pi, pj = t["order"][i], t["order"][j]
        r, c = np.maximum(pi, pj).astype(np.int64), np.minimum(pi, pj)   # (symmetric: the lower triangle holds it)
        s = node_of[c]
        q = s.astype(np.int64) * (self.n + 1) + r
        e = np.searchsorted(keys, q)
        ok = e < len(keys)
        ok[ok] = keys[e[ok]] == q[ok]
        if not ok.all():
            bad = int(np.nonzero(~ok)[0][0])
            raise ValueError(f"inverse_entries: ({int(i[bad])}, {int(j[bad])}) is not in the pattern of L")
        lr = e - t["rptr"][s]                                  # node-local row
        k = c - t["sptr"][s]                                   # node-local column
        b = t["node_bcol0"][s] + k // self.options.nb
        r0 = t["bcol_r0"][b].astype(np.int64)
        return t["bcol_off"][b] + (lr - r0) * t["bcol_width"][b] + (k - r0)

    def solve(self, b, job=0):
        """spllt_solve on a copy of b (n or n x nrhs, column-major per rhs)."""
        x = np.array(b, dtype=np.float64, order="F", copy=True)
        nrhs = 1 if x.ndim == 1 else x.shape[1]
        ws = C.c_long()
        self.lib.spllt_prepare_solve(self.akeep, self.fkeep, self.options.nb, nrhs, C.byref(ws),
                                     C.byref(self.info))
        self.lib.spllt_solve(self.fkeep, C.byref(self.options), _ip(self.order), nrhs, _dp(x),
                             C.byref(self.info), job)
        if self.info.flag < 0:
            raise SplltError("spllt_solve", self.info.flag, self.last_error())
        return x

    def solve_dev(self, y_dev_ptr, nrhs=1, job=0, phase=-1):
        """spllt_hip_solve_dev: substitution on device vectors in pivot order
        (y[q*n + p(i)] = b_q[i], p = 0-based pivot position ("order" of spllt_hip_sym_get)), in place; phase 0/1/2 on a partitioned factor."""
        self._call("spllt_hip_solve_dev", self.fkeep, C.c_void_p(y_dev_ptr), nrhs, job, phase)
        return self

    def solve_many(self, b, job=0):
        """spllt_hip_solve_many on a copy of b (n or n x nrhs): the blocked solve, 32 right-hand sides per
        sweep on the fp64 matrix cores.  Returns a new F-ordered array, like solve."""
        x = np.array(b, dtype=np.float64, order="F", copy=True)
        nrhs = 1 if x.ndim == 1 else x.shape[1]
        ldx = x.shape[0]
        self._call("spllt_hip_solve_many", self.fkeep, nrhs, _dp(x), ldx, job)
        return x

    def solve_many_dev(self, x_dev_ptr, nrhs, ldx=None, job=0, pivot_order=False):
        """spllt_hip_solve_many_dev: the blocked solve on device vectors, in place (vector q at
        x[q*ldx .. q*ldx + n), ldx defaults to n); pivot_order=True: the vectors are in pivot order as for
        solve_dev, else in the user's variable order."""
        if ldx is None:
            ldx = self.n
        self._call("spllt_hip_solve_many_dev", self.fkeep, nrhs, C.c_void_p(x_dev_ptr), int(ldx), job,
                   1 if pivot_order else 0)
        return self

    # ---- reproducible solve ----------------------------------------------------
    def solve_reproducible(self, b, job=0):
        """spllt_hip_solve_repro on a copy of b (n or n x nrhs): the substitution without atomic adds -- the same
        factor bits and the same b give the same bits of x, whatever the number of columns.  Returns a new
        F-ordered array, like solve."""
        x = np.array(b, dtype=np.float64, order="F", copy=True)
        nrhs = 1 if x.ndim == 1 else x.shape[1]
        ldx = x.shape[0]
        self._call("spllt_hip_solve_repro", self.fkeep, nrhs, _dp(x), ldx, job)
        return x

    def solve_reproducible_dev(self, x_dev_ptr, nrhs, ldx=None, job=0, pivot_order=False):
        """spllt_hip_solve_repro_dev: the reproducible solve on device vectors, in place (layout and
        pivot_order as solve_many_dev)."""
        if ldx is None:
            ldx = self.n
        self._call("spllt_hip_solve_repro_dev", self.fkeep, nrhs, C.c_void_p(x_dev_ptr), int(ldx), job,
                   1 if pivot_order else 0)
        return self

    def set_reproducible_solve(self, on):
        """Route solve, solve_dev(phase=-1) and the preconditioner of solve_refined through the reproducible
        path (solve_many is not affected).  Returns the previous setting."""
        rc = self._call("spllt_hip_set_reproducible_solve", self.fkeep, 1 if on else 0)
        return bool(rc)

    def release_solve_repro(self):
        """The tables and the scratch of the reproducible solve back to the device pool."""
        self._call("spllt_hip_release_solve_repro", self.fkeep)
        return self

    # ---- hard linear constraints C x = e (include/spllt_hip_constrain.h) -----------
    def set_constraints(self, C_rows):
        """spllt_hip_set_constraints: store the k <= 64 dense rows of C (k x n, or n for one row) and build
        W = A^-1 C^T, S = C W = G G^T and U = W G^-T for the current factor; a later factorization or update is
        picked up by the next call that needs them.  None or zero rows clear the constraints.  Dependent rows
        raise SplltError with flag -20 and leave the handle without constraints."""
        if C_rows is None:
            self._call("spllt_hip_set_constraints", self.fkeep, 0, None, max(self.n, 1))
            return self
        c = np.ascontiguousarray(np.atleast_2d(np.asarray(C_rows, dtype=np.float64)))
        if c.ndim != 2 or c.shape[1] != self.n:
            raise ValueError(f"C must be (k, {self.n}), got {c.shape}")
        self._call("spllt_hip_set_constraints", self.fkeep, c.shape[0], _dp(c) if c.shape[0] else None, max(self.n, 1))
        return self

    def set_constraints_dev(self, c_dev_ptr, k, ldc=None):
        """spllt_hip_set_constraints_dev: row i of C at c[i*ldc .. i*ldc + n) in device memory"""
        self._call("spllt_hip_set_constraints_dev", self.fkeep, int(k), C.c_void_p(c_dev_ptr),
                   int(self.n if ldc is None else ldc))
        return self

    def _constrain_call(self, name, X, e, multipliers):
        x = np.array(X, dtype=np.float64, order="F", copy=True)
        if x.shape[0] != self.n or x.ndim > 2:
            raise ValueError(f"the vectors must be ({self.n},) or ({self.n}, nvec), got {x.shape}")
        nvec = 1 if x.ndim == 1 else x.shape[1]
        k = self.constraints_info()["k"]
        ev, lde = None, 0
        if e is not None:
            ev = np.array(e, dtype=np.float64, order="F", copy=True)
            if ev.shape not in ((k,), (k, nvec)):
                raise ValueError(f"e must be ({k},) or ({k}, {nvec}), got {ev.shape}")
            lde = k if ev.ndim == 2 else 0     # (one column per vector, else one shared column)
        lam = np.zeros((max(k, 1), nvec), dtype=np.float64, order="F") if multipliers else None
        self._call(name, self.fkeep, nvec, _dp(x), max(self.n, 1), None if ev is None else _dp(ev), lde,
                   None if lam is None else _dp(lam), max(k, 1))
        if not multipliers:
            return x
        lam = lam[:k]
        return x, (lam[:, 0] if x.ndim == 1 else lam)

    def constrain(self, X, e=None, multipliers=False):
        """spllt_hip_constrain on a copy of X (n or n x nvec): x* = x - U G^-1 (C x - e), so that C x* = e.  e: None
        (zeros), k targets shared by all vectors, or (k, nvec).  multipliers=True also returns lambda = S^-1 (C x - e)
        (k or k x nvec).  Bit-reproducible: the same vector gives the same bits whatever nvec and its place."""
        return self._constrain_call("spllt_hip_constrain", X, e, multipliers)

    def solve_constrained(self, b, e=None, multipliers=False):
        """spllt_hip_solve_constrained on a copy of b: constrain(solve_many(b), e) in one call; with
        multipliers=True, (x*, lambda) solves the KKT system A x + C^T lambda = b, C x = e."""
        return self._constrain_call("spllt_hip_solve_constrained", b, e, multipliers)

    def sample_constrained(self, nsamp, seed=0, mean=None, e=None, first_sample=0):
        """spllt_hip_sample_constrained: nsamp draws of N(mean, A^-1) | C x = e as an F-ordered (n, nsamp) array:
        the kind "precision" sample of (seed, first_sample + q), corrected (conditioning by kriging).  e: None or
        k shared targets."""
        x = np.zeros((self.n, nsamp), dtype=np.float64, order="F")
        m = None if mean is None else np.ascontiguousarray(mean, dtype=np.float64)
        if m is not None and m.shape != (self.n,):
            raise ValueError(f"mean must be ({self.n},)")
        ev = None if e is None else np.ascontiguousarray(e, dtype=np.float64)
        if ev is not None and ev.shape != (self.constraints_info()["k"],):
            raise ValueError("e must hold one target per constraint")
        self._call("spllt_hip_sample_constrained", self.fkeep, nsamp, _dp(x), max(self.n, 1), int(seed), int(first_sample),
                   None if m is None else _dp(m), None if ev is None else _dp(ev))
        return x

    def constrain_dev(self, x_dev_ptr, nvec, ldx=None, e_dev_ptr=None, lde=0, lambda_dev_ptr=None, ldl=0,
                      entry="constrain"):
        """spllt_hip_constrain_dev / spllt_hip_solve_constrained_dev (entry="solve_constrained") on device vectors,
        in place (layout of solve_many_dev); e and lambda: device pointers or None"""
        self._call(f"spllt_hip_{entry}_dev", self.fkeep, int(nvec), C.c_void_p(x_dev_ptr), int(self.n if ldx is None else ldx),
                   None if e_dev_ptr is None else C.c_void_p(e_dev_ptr), int(lde),
                   None if lambda_dev_ptr is None else C.c_void_p(lambda_dev_ptr), int(ldl))
        return self

    def sample_constrained_dev(self, x_dev_ptr, nsamp, ldx=None, seed=0, mean_dev_ptr=None, e_dev_ptr=None, first_sample=0):
        """spllt_hip_sample_constrained_dev: the constrained samples into device memory (layout of sample_dev)"""
        self._call("spllt_hip_sample_constrained_dev", self.fkeep, int(nsamp), C.c_void_p(x_dev_ptr),
                   int(self.n if ldx is None else ldx), int(seed), int(first_sample),
                   None if mean_dev_ptr is None else C.c_void_p(mean_dev_ptr),
                   None if e_dev_ptr is None else C.c_void_p(e_dev_ptr))
        return self

    def inverse_diag_constrained(self):
        """Var(x_i | C x = e) = (A^-1)_ii - sum_j U[i, j]^2 in the user's variable order; needs selected_inverse()
        of the current factor, like inverse_diag"""
        out = np.zeros(max(self.n, 1), dtype=np.float64)
        self._call("spllt_hip_inverse_diag_constrained", self.fkeep, _dp(out), self.n)
        return out[:self.n]

    def constraints_info(self):
        """k, rebuilds of U so far, device bytes held, kernel launches of the last call, log det S and the smallest
        relative pivot of S = G G^T"""
        out = np.zeros(4, dtype=np.int64)
        stat = np.zeros(2, dtype=np.float64)
        self._call("spllt_hip_constraints_info", self.fkeep, out.ctypes.data_as(C.POINTER(C.c_int64)), _dp(stat))
        return {"k": int(out[0]), "rebuilds": int(out[1]), "device_bytes": int(out[2]), "launches": int(out[3]),
                "log_det_s": float(stat[0]), "min_relative_pivot": float(stat[1])}

    def release_constraints(self):
        """C, U and the work arrays of the constraints back to the device pool; C is forgotten."""
        self._call("spllt_hip_release_constraints", self.fkeep)
        return self

    # ---- products with the factor, Gaussian sampling ------------------------------
    def factor_mult(self, x, job=0):
        """spllt_hip_factor_mult on a copy of x (n or n x nvec): job 0 P^T L L^T P x, 1 P^T L x, 2 L^T P x -- the
        inverse of solve_many(job), bit-reproducible.  Returns a new F-ordered array, like solve."""
        y = np.array(x, dtype=np.float64, order="F", copy=True)
        nvec = 1 if y.ndim == 1 else y.shape[1]
        self._call("spllt_hip_factor_mult", self.fkeep, nvec, _dp(y), y.shape[0], job)
        return y

    def factor_mult_dev(self, x_dev_ptr, nvec, ldx=None, job=0, pivot_order=False):
        """spllt_hip_factor_mult_dev: the product on device vectors, in place (layout and pivot_order as
        solve_many_dev)."""
        if ldx is None:
            ldx = self.n
        self._call("spllt_hip_factor_mult_dev", self.fkeep, nvec, C.c_void_p(x_dev_ptr), int(ldx), job,
                   1 if pivot_order else 0)
        return self

    def release_factor_mult(self):
        """The second workspace, the scratch and the tables of the factor products back to the device pool."""
        self._call("spllt_hip_release_factor_mult", self.fkeep)
        return self

    # ---- reverse-mode derivative of the factor ------------------------------------
    @staticmethod
    def _order_flags(a_pivot_order, b_pivot_order):
        return (1 if a_pivot_order else 0) | (2 if b_pivot_order else 0)

    def factor_adjoint_seed(self, a, b, alpha=1.0, accumulate=False, a_pivot_order=False, b_pivot_order=False):
        """spllt_hip_factor_adjoint_seed on host arrays a, b of shape (n,) or (n, nvec): Lbar (+)= alpha sum_q
        a_q b_q^T on the lower positions of L; a vector is in the user's variable order unless its flag says
        pivot order"""
        a = np.asfortranarray(np.asarray(a, dtype=np.float64).reshape(self.n, -1))
        b = np.asfortranarray(np.asarray(b, dtype=np.float64).reshape(self.n, -1))
        if a.shape != b.shape:
            raise ValueError("factor_adjoint_seed: a and b must have the same shape")
        self._call("spllt_hip_factor_adjoint_seed", self.fkeep, a.shape[1], _dp(a), _dp(b), max(self.n, 1), float(alpha),
                   1 if accumulate else 0,
                   self._order_flags(a_pivot_order, b_pivot_order))
        return self

    def factor_adjoint_seed_dev(self, a_dev_ptr, b_dev_ptr, nvec, ld=None, alpha=1.0, accumulate=False,
                                a_pivot_order=False, b_pivot_order=False):
        """spllt_hip_factor_adjoint_seed_dev: the seed from device vectors (vector q at a[q*ld .. q*ld + n))"""
        if ld is None:
            ld = self.n
        self._call("spllt_hip_factor_adjoint_seed_dev", self.fkeep, int(nvec), C.c_void_p(a_dev_ptr), C.c_void_p(b_dev_ptr),
                   int(ld), float(alpha), 1 if accumulate else 0,
                   self._order_flags(a_pivot_order, b_pivot_order))
        return self

    def set_factor_adjoint(self, arena):
        """spllt_hip_set_factor_adjoint: an arbitrary Lbar, the layout of get_factor (its strict upper triangles of
        diagonal tiles are never read)"""
        arena = np.ascontiguousarray(arena, dtype=np.float64)
        self._call("spllt_hip_set_factor_adjoint", self.fkeep, _dp(arena), arena.size)
        return self

    def get_factor_adjoint(self, out=None):
        """the adjoint arena on the host: Lbar as seeded, or after factor_adjoint() d loss / d (P A P^T) on the
        stored lower positions"""
        arena = self.sym_info()["arena"]
        if out is None:
            out = np.zeros(max(arena, 1), dtype=np.float64)
        assert out.dtype == np.float64 and out.size >= arena and out.flags["C_CONTIGUOUS"]
        self._call("spllt_hip_get_factor_adjoint", self.fkeep, _dp(out), arena)
        return out[:arena]

    def device_factor_adjoint_ptr(self):
        return self.lib.spllt_hip_device_factor_adjoint(self.fkeep)

    def factor_adjoint(self):
        """spllt_hip_factor_adjoint: the sweep over the seeded arena; returns d loss / d val, nnz values"""
        out = np.zeros(max(self.nnz, 1), dtype=np.float64)
        self._call("spllt_hip_factor_adjoint", self.fkeep, _dp(out))
        return out[:self.nnz]

    def factor_adjoint_dev(self, gval_dev_ptr):
        """spllt_hip_factor_adjoint_dev: the same sweep, the nnz values into device memory"""
        self._call("spllt_hip_factor_adjoint_dev", self.fkeep, C.c_void_p(gval_dev_ptr))
        return self

    def release_factor_adjoint(self):
        self._call("spllt_hip_release_factor_adjoint", self.fkeep)
        return self

    _SAMPLE_KINDS = {"precision": 0, "covariance": 1}

    def _sample_kind(self, kind):
        """0 / 1 of the C interface; an unknown name goes on as -1 and is rejected by the library"""
        return self._SAMPLE_KINDS.get(kind, -1) if isinstance(kind, str) else int(kind)

    def sample(self, nsamp, seed=0, kind="precision", mean=None, first_sample=0):
        """spllt_hip_sample: nsamp draws of N(mean, A^-1) (kind "precision") or N(mean, A) ("covariance") from
        the current factor, as an F-ordered (n, nsamp) array in user order.  Sample q is a function of (seed,
        first_sample + q) alone."""
        k = self._sample_kind(kind)
        x = np.zeros((self.n, nsamp), dtype=np.float64, order="F")
        m = None if mean is None else np.ascontiguousarray(mean, dtype=np.float64)
        assert m is None or m.shape == (self.n,)
        self._call("spllt_hip_sample", self.fkeep, nsamp, _dp(x), max(self.n, 1), k, int(seed), int(first_sample),
                   None if m is None else _dp(m))
        return x

    def sample_dev(self, x_dev_ptr, nsamp, ldx=None, seed=0, kind="precision", mean_dev_ptr=None, first_sample=0):
        """spllt_hip_sample_dev: the samples into device memory (sample q at x[q*ldx .. q*ldx + n), user order);
        mean_dev_ptr: n doubles on the device or None."""
        if ldx is None:
            ldx = self.n
        k = self._sample_kind(kind)
        self._call("spllt_hip_sample_dev", self.fkeep, nsamp, C.c_void_p(x_dev_ptr), int(ldx),
                   k, int(seed), int(first_sample),
                   None if mean_dev_ptr is None else C.c_void_p(mean_dev_ptr))
        return self

    def white_noise_dev(self, z_dev_ptr, nsamp, ldz=None, seed=0, first_sample=0):
        """spllt_hip_white_noise_dev: the standard normals the samplers use into device memory, sample q at
        z[q*ldz .. q*ldz + n) in PIVOT order"""
        if ldz is None:
            ldz = max(self.n, 1)
        self._call("spllt_hip_white_noise_dev", self.fkeep, int(nsamp), C.c_void_p(z_dev_ptr), int(ldz), int(seed),
                   int(first_sample))
        return self

    def white_noise(self, nsamp, seed, first_sample=0):
        """spllt_hip_white_noise_dev, copied to the host: the (n, nsamp) standard normals the samplers use, in
        PIVOT order (row p = pivot position p)."""
        import torch
        z = torch.empty((nsamp, max(self.n, 1)), dtype=torch.float64, device="cuda")
        self._call("spllt_hip_white_noise_dev", self.fkeep, nsamp, C.c_void_p(z.data_ptr()), max(self.n, 1), int(seed),
                   int(first_sample))
        return np.asfortranarray(z.cpu().numpy()[:, :self.n].T)

    # ---- sparse right-hand sides and selected outputs -----------------------------
    def _sparse_columns(self, B, where):
        """B (scipy sparse n x k, or dense) as the 1-based CSC arrays of the C interface; explicit zeros stay"""
        import scipy.sparse as sp
        if not sp.issparse(B):
            B = np.asarray(B, dtype=np.float64)
            if B.ndim == 1:
                B = B.reshape(-1, 1)
        if B.ndim != 2 or B.shape[0] != self.n:
            raise SplltError(where, -10, f"B must have n = {self.n} rows")
        B = sp.csc_matrix(B, dtype=np.float64)
        B.sum_duplicates()
        B.sort_indices()
        return (B.shape[1], np.ascontiguousarray(B.indptr + 1, dtype=np.int32),
                np.ascontiguousarray(np.append(B.indices + 1, 0), dtype=np.int32),
                np.ascontiguousarray(np.append(B.data, 0.0), dtype=np.float64))

    @staticmethod
    def _wanted(rows):
        """rows (0-based variables, None: all) as (nsel, 1-based int32 array or None)"""
        if rows is None:
            return -1, None
        sel = np.ascontiguousarray(np.append(np.asarray(rows, dtype=np.int64).ravel() + 1, 0), dtype=np.int32)
        return len(sel) - 1, sel

    def solve_sparse(self, B, rows=None, job=0):
        """spllt_hip_solve_sparse: A^-1 B (job 1: L^-1 P B, job 2: L^-T of the scattered B) for the sparse columns
        of B (scipy sparse, n x k) at the 0-based variables `rows` (any order, duplicates allowed; None: all n).
        Only the block columns on the elimination-tree paths of B's nonzeros and of the wanted rows are visited.
        Returns an F-ordered (len(rows) or n) x k array."""
        where = "spllt_hip_solve_sparse"
        k, ptr, row, val = self._sparse_columns(B, where)
        nsel, sel = self._wanted(rows)
        m = self.n if sel is None else nsel
        x = np.zeros((max(m, 1), max(k, 1)), dtype=np.float64, order="F")   # (never a null pointer)
        self._call(where, self.fkeep, k, _ip(ptr), _ip(row), _dp(val), nsel,
                   None if sel is None else _ip(sel), _dp(x), max(m, 1), job)
        return np.asfortranarray(x[:m, :k])

    def solve_sparse_dev(self, B, x_dev_ptr, ldx, rows=None, job=0):
        """spllt_hip_solve_sparse_dev: as solve_sparse with the result written to device memory, column q at
        x[q*ldx .. q*ldx + (len(rows) or n)); nothing else is written."""
        where = "spllt_hip_solve_sparse_dev"
        k, ptr, row, val = self._sparse_columns(B, where)
        nsel, sel = self._wanted(rows)
        self._call(where, self.fkeep, k, _ip(ptr), _ip(row), _dp(val), nsel,
                   None if sel is None else _ip(sel), C.c_void_p(x_dev_ptr), int(ldx), job)
        return self

    def gram(self, B):
        """spllt_hip_gram_sparse: B^T A^-1 B for the sparse columns of B (n x k), by forward sweeps on the paths
        of B's nonzeros only; k x k, exactly symmetric."""
        where = "spllt_hip_gram_sparse"
        k, ptr, row, val = self._sparse_columns(B, where)
        G = np.zeros((max(k, 1), max(k, 1)), dtype=np.float64, order="F")
        self._call(where, self.fkeep, k, _ip(ptr), _ip(row), _dp(val), _dp(G), max(k, 1))
        return G[:k, :k]

    def inverse_block(self, i, j):
        """A^-1[i][:, j] for any 0-based index sets i, j, inside the pattern of L or not: sparse solves with the
        unit columns e_j and the wanted rows i."""
        import scipy.sparse as sp
        i = np.asarray(i, dtype=np.int64).ravel()
        j = np.asarray(j, dtype=np.int64).ravel()
        if ((i < 0) | (i >= self.n)).any() or ((j < 0) | (j >= self.n)).any():
            raise ValueError("inverse_block: index out of range")
        E = sp.csc_matrix((np.ones(len(j)), (j, np.arange(len(j)))), shape=(self.n, len(j)))
        return self.solve_sparse(E, rows=i)

    def solve_sparse_plan(self, B, rows=None, job=0):
        """spllt_hip_solve_sparse_plan: (fwd, bwd), the block columns the two sweeps of solve_sparse(B, rows, job)
        would visit with B's columns taken as one group, ascending (needs no device and no factor)"""
        where = "spllt_hip_solve_sparse_plan"
        k, ptr, row, _ = self._sparse_columns(B, where)
        nsel, sel = self._wanted(rows)
        selp = None if sel is None else _ip(sel)
        cnt = np.zeros(2, dtype=np.int64)
        cp = cnt.ctypes.data_as(C.POINTER(C.c_int64))
        self._call(where, self.fkeep, k, _ip(ptr), _ip(row), nsel, selp, job, None, 0, None, 0, cp)
        fwd = np.zeros(max(int(cnt[0]), 1), dtype=np.int32)
        bwd = np.zeros(max(int(cnt[1]), 1), dtype=np.int32)
        i32 = C.POINTER(C.c_int32)
        self._call(where, self.fkeep, k, _ip(ptr), _ip(row), nsel, selp, job,
                   fwd.ctypes.data_as(i32), len(fwd), bwd.ctypes.data_as(i32), len(bwd), cp)
        return fwd[:int(cnt[0])], bwd[:int(cnt[1])]

    def solve_sparse_info(self):
        """of the last solve_sparse / gram, summed over its groups of columns: block columns and doubles of L the
        forward / backward sweeps visited, kernel launches, workgroups of the sweeps"""
        out = np.zeros(6, dtype=np.int64)
        self._call("spllt_hip_solve_sparse_info", self.fkeep, out.ctypes.data_as(C.POINTER(C.c_int64)))
        return dict(zip(("fwd_bcols", "bwd_bcols", "fwd_entries", "bwd_entries", "launches", "workgroups"),
                        (int(v) for v in out)))

    def release_solve_sparse(self):
        """The staged lists, the gathered block and the gram workspaces back to the device pool."""
        self._call("spllt_hip_release_solve_sparse", self.fkeep)
        return self

    # ---- refined solves --------------------------------------------------------
    _METHODS = {"ir": 0, "pcg": 1, 0: 0, 1: 1}
    refine_status = None     # return value of the last solve_refined() on this handle

    def _values(self, val, where):
        val = np.ascontiguousarray(val, dtype=np.float64)
        if val.ndim != 1:
            raise SplltError(where, -10, "val must be one array of nnz values")
        return val

    def matvec(self, val, x):
        """spllt_hip_matvec: A x on the device with A = (the analysed pattern, val); x is n or n x nvec.
        Two calls with the same inputs return bit-identical results.  Needs no factor."""
        val = self._values(val, "spllt_hip_matvec")
        x = np.asarray(x, dtype=np.float64)
        xs = np.asfortranarray(x.reshape(x.shape[0], -1))
        y = np.empty_like(xs, order="F")
        ld = max(1, xs.shape[0])
        self._call("spllt_hip_matvec", self.fkeep, int(val.size), _dp(val), xs.shape[1], _dp(xs), ld, _dp(y), ld)
        return y.reshape(x.shape, order="F")

    def matvec_dev(self, val_dev_ptr, nnz, x_dev_ptr, y_dev_ptr, nvec, ldx=None, ldy=None, pivot_order=False):
        """spllt_hip_matvec_dev: the product on device arrays (vector q at x[q*ldx .. q*ldx + n), y alike;
        pivot_order as for solve_many_dev; x and y must not overlap)."""
        self._call("spllt_hip_matvec_dev", self.fkeep, int(nnz), C.c_void_p(val_dev_ptr), nvec, C.c_void_p(x_dev_ptr),
                   int(self.n if ldx is None else ldx), C.c_void_p(y_dev_ptr),
                   int(self.n if ldy is None else ldy), 1 if pivot_order else 0)
        return self

    def solve_refined(self, val, b, method="pcg", tol=1e-14, max_iter=50):
        """spllt_hip_solve_refined on a copy of b (n or n x nrhs): solve A x = b for A = (pattern, val) with the
        current factor as preconditioner, to the backward error tol.  method "ir" (refinement) or "pcg".
        Returns (x, iterations, error): per vector the applications of the factor after the first and the
        backward error of a true residual; `not error[q] <= tol` marks a vector that did not converge (x then
        holds its best iterate).  self.refine_status keeps the call's return value (0: every vector reached tol,
        1: at least one did not, negative: the flag of the error raised; None before the first call)."""
        if method not in self._METHODS:
            raise SplltError("spllt_hip_solve_refined", -10, "method is not 'ir' or 'pcg'")
        val = self._values(val, "spllt_hip_solve_refined")
        x = np.array(b, dtype=np.float64, order="F", copy=True)
        nrhs = 1 if x.ndim == 1 else x.shape[1]
        it = np.zeros(max(1, nrhs), dtype=np.int32)
        err = np.zeros(max(1, nrhs), dtype=np.float64)
        rc = self.lib.spllt_hip_solve_refined(self.fkeep, int(val.size), _dp(val), nrhs, _dp(x), max(1, x.shape[0]),
                                              self._METHODS[method], float(tol), int(max_iter), _ip(it), _dp(err))
        self.refine_status = rc
        if rc < 0:
            raise SplltError("spllt_hip_solve_refined", rc, self.last_error())
        return x, it[:nrhs], err[:nrhs]

    def solve_refined_dev(self, val_dev_ptr, nnz, x_dev_ptr, nrhs, ldx=None, method="pcg", tol=1e-14, max_iter=50):
        """spllt_hip_solve_refined_dev: values and vectors on the device (user order, in place).  Returns
        (status, iterations, error); status 0: every vector reached tol, 1: at least one did not."""
        if method not in self._METHODS:
            raise SplltError("spllt_hip_solve_refined_dev", -10, "method is not 'ir' or 'pcg'")
        it = np.zeros(max(1, nrhs), dtype=np.int32)
        err = np.zeros(max(1, nrhs), dtype=np.float64)
        rc = self._call("spllt_hip_solve_refined_dev", self.fkeep, int(nnz), C.c_void_p(val_dev_ptr), nrhs,
                        C.c_void_p(x_dev_ptr), int(self.n if ldx is None else ldx),
                        self._METHODS[method], float(tol), int(max_iter), _ip(it), _dp(err))
        return rc, it[:nrhs], err[:nrhs]

    def release_refine(self):
        """spllt_hip_release_refine: the operator tables and work vectors go back to the pool"""
        self._call("spllt_hip_release_refine", self.fkeep)
        return self

    # ---- low-rank update / downdate ----------------------------------------------
    def _updown_columns(self, W, where):
        """W (scipy sparse n x k, a dense vector of length n or a dense n x k array; zeros dropped) as the
        1-based CSC arrays of the C interface"""
        import scipy.sparse as sp
        if not sp.issparse(W):
            W = np.asarray(W, dtype=np.float64)
            if W.ndim == 1:
                W = W.reshape(-1, 1)
            if W.ndim != 2:
                raise SplltError(where, -10, "W must be a vector or an n x k matrix")
        if W.shape[0] != self.n:
            raise SplltError(where, -10, f"W has {W.shape[0]} rows, n = {self.n}")
        W = sp.csc_matrix(W, dtype=np.float64)
        W.sum_duplicates()
        W.eliminate_zeros()
        W.sort_indices()
        return (W.shape[1], np.ascontiguousarray(W.indptr + 1, dtype=np.int32),
                np.ascontiguousarray(np.append(W.indices + 1, 0), dtype=np.int32),
                np.ascontiguousarray(np.append(W.data, 0.0), dtype=np.float64))

    def update(self, W, downdate=False):
        """spllt_hip_updown: the factor of A + W W^T (downdate: A - W W^T) in place of the current one; the
        pattern of every column of W must be a clique of the analysed matrix (include/spllt_hip.h).  A downdate
        that is not positive definite raises with flag -20 and leaves the handle without a factor until the
        next factor()."""
        k, ptr, row, val = self._updown_columns(W, "spllt_hip_updown")
        self._call("spllt_hip_updown", self.fkeep, k, _ip(ptr), _ip(row), _dp(val), -1 if downdate else 1)
        return self

    def updown_plan(self, W):
        """spllt_hip_updown_plan: the block columns update(W) would visit, ascending (needs no device)"""
        k, ptr, row, _ = self._updown_columns(W, "spllt_hip_updown_plan")
        cnt = self.lib.spllt_hip_updown_plan(self.fkeep, k, _ip(ptr), _ip(row), None, 0)
        if cnt < 0:
            raise SplltError("spllt_hip_updown_plan", int(cnt), self.last_error())
        out = np.zeros(max(cnt, 1), dtype=np.int32)
        self.lib.spllt_hip_updown_plan(self.fkeep, k, _ip(ptr), _ip(row), out.ctypes.data_as(C.POINTER(C.c_int32)), cnt)
        return out[:cnt]

    def updown_info(self):
        """of the last update(): block columns visited, entries of L in them, kernel launches, passes"""
        out = np.zeros(4, dtype=np.int64)
        self._call("spllt_hip_updown_info", self.fkeep, out.ctypes.data_as(C.POINTER(C.c_int64)))
        return dict(zip(("bcols", "entries", "launches", "passes"), (int(v) for v in out)))

    def updown_device_ms(self):
        """spllt_hip_updown_time: device time of the last update(), first scatter to last kernel"""
        v = C.c_double()
        self._call("spllt_hip_updown_time", self.fkeep, C.byref(v))
        return v.value

    def matvec_tables(self):
        """the operator of the refined solves: (rowptr int64, col int32, src int32) of the full CSR of
        P A P^T in pivot order ("matvec_*" of spllt_hip_program_get); needs no device"""
        return self.program("matvec_rowptr"), self.program("matvec_col"), self.program("matvec_src")

    # ---- batched factorization ------------------------------------------------
    # every error of a batch call raises, except -20: a batch with a member that is not positive definite returns
    # normally (batch_status() tells which), so that a sweep with one bad sample keeps the rest
    _BATCH_OK = (-20,)

    def factor_batch(self, vals, ldval=None):
        """spllt_hip_factor_batch: vals of shape (B, nnz), one row of values per member; finished on
        return.  Returns 0, or -20 when at least one member is not positive definite."""
        vals = np.ascontiguousarray(vals, dtype=np.float64)
        if vals.ndim != 2:
            raise ValueError("factor_batch: vals must have shape (B, nnz)")
        if ldval is None:
            ldval = vals.shape[1]
        return self._call("spllt_hip_factor_batch", self.akeep, self.fkeep, vals.shape[0], self.nnz,
                          C.c_void_p(vals.ctypes.data), int(ldval), ok=self._BATCH_OK)

    def factor_batch_dev(self, val_dev_ptr, nbatch, ldval=None):
        """the same with the values in HBM (integer device pointer; member b at ptr + b * ldval doubles)"""
        if ldval is None:
            ldval = self.nnz
        return self._call("spllt_hip_factor_batch_dev", self.akeep, self.fkeep, int(nbatch), self.nnz,
                          C.c_void_p(val_dev_ptr), int(ldval), ok=self._BATCH_OK)

    def batch_status(self):
        """(flags, columns) of the last batch: 0 / -20 per member, 1-based pivot position of the first
        non-positive pivot (0: none)"""
        nb = self.lib.spllt_hip_batch_status(self.fkeep, None, None, 0)
        if nb < 0:
            raise SplltError("spllt_hip_batch_status", nb, self.last_error())
        flags = np.zeros(max(nb, 1), dtype=np.int32)
        cols = np.zeros(max(nb, 1), dtype=np.int32)
        self.lib.spllt_hip_batch_status(self.fkeep, _ip(flags), _ip(cols), nb)
        return flags[:nb], cols[:nb]

    def solve_batch(self, b, job=0):
        """spllt_hip_solve_batch on a copy of b: shape (B, n), one vector per member, or (B, nrhs, n).
        The vectors of a member that is not positive definite come back unchanged."""
        x = np.array(b, dtype=np.float64, order="C", copy=True)
        if x.ndim not in (2, 3):
            raise ValueError("solve_batch: b must have shape (B, n) or (B, nrhs, n)")
        nrhs = 1 if x.ndim == 2 else x.shape[1]
        # the C entry point takes no nbatch: it reads and writes the vectors of EVERY member of the last batch
        nb = self.lib.spllt_hip_batch_status(self.fkeep, None, None, 0)
        if nb > 0 and x.shape[0] != nb:
            raise ValueError(f"solve_batch: b holds vectors for {x.shape[0]} members, the last batch has {nb}")
        if x.shape[-1] != self.n:
            raise ValueError(f"solve_batch: the vectors have length {x.shape[-1]}, n = {self.n}")
        self._call("spllt_hip_solve_batch", self.fkeep, nrhs, C.c_void_p(x.ctypes.data), x.shape[-1], job, ok=self._BATCH_OK)
        return x

    def solve_batch_dev(self, x_dev_ptr, nrhs, ldx=None, job=0, pivot_order=False):
        """spllt_hip_solve_batch_dev: device vectors in place, vector q of member b at
        x[(b*nrhs + q)*ldx .. + n); pivot_order as solve_many_dev.  Returns 0 or -20.
        The library touches nbatch * nrhs vectors, nbatch being the size of the LAST batch
        (batch_status()[0].size): the array behind the pointer must hold that many."""
        if ldx is None:
            ldx = self.n
        return self._call("spllt_hip_solve_batch_dev", self.fkeep, int(nrhs), C.c_void_p(x_dev_ptr), int(ldx), job,
                          1 if pivot_order else 0, ok=self._BATCH_OK)

    def get_factor_batch(self, member, out=None):
        """one member's arena on the host (the layout of get_factor)"""
        arena = self.sym_info()["arena"]
        if out is None:
            out = np.zeros(max(arena, 1), dtype=np.float64)
        assert out.dtype == np.float64 and out.size >= arena and out.flags["C_CONTIGUOUS"]
        self._call("spllt_hip_get_factor_batch", self.fkeep, int(member), _dp(out), arena)
        return out[:arena]

    def device_factor_batch_ptr(self):
        """(device pointer of member 0's arena, member stride in doubles)"""
        stride = C.c_int64()
        p = self.lib.spllt_hip_device_factor_batch(self.fkeep, C.byref(stride))
        return p, stride.value

    def log_det_batch(self):
        """log det A_b of every member of the last batch (NaN for a failed member)"""
        nb = self.lib.spllt_hip_batch_status(self.fkeep, None, None, 0)
        out = np.zeros(max(nb, 1), dtype=np.float64)
        self._call("spllt_hip_log_det_batch", self.fkeep, _dp(out))
        return out[:nb]

    def batch_launches(self):
        """kernel launches of the last batched factorization"""
        return int(self.lib.spllt_hip_batch_launches(self.fkeep))

    def release_batch(self):
        self._call("spllt_hip_release_batch", self.fkeep)

    # ---- batched factor products and sampling (include/spllt_hip_batch_mult.h) -----
    def _batch_count(self):
        return int(self.lib.spllt_hip_batch_status(self.fkeep, None, None, 0))

    def factor_mult_batch(self, X, job=0):
        """spllt_hip_factor_mult_batch on a copy of X: shape (B, n), one vector per member, or (B, nvec, n), like
        solve_batch.  job 0 P^T L_b L_b^T P x, 1 P^T L_b x, 2 L_b^T P x: the inverse of solve_batch(job),
        bit-reproducible.  The vectors of a member that is not positive definite come back unchanged."""
        x = np.array(X, dtype=np.float64, order="C", copy=True)
        if x.ndim not in (2, 3):
            raise ValueError("factor_mult_batch: X must have shape (B, n) or (B, nvec, n)")
        nvec = 1 if x.ndim == 2 else x.shape[1]
        if x.shape[-1] != self.n:
            raise ValueError(f"factor_mult_batch: the vectors have length {x.shape[-1]}, n = {self.n}")
        nb = self._batch_count()
        if nb > 0 and x.shape[0] != nb:
            raise ValueError(f"factor_mult_batch: X holds vectors for {x.shape[0]} members, the last batch has {nb}")
        self._call("spllt_hip_factor_mult_batch", self.fkeep, nvec, C.c_void_p(x.ctypes.data), x.shape[-1], job,
                   ok=self._BATCH_OK)
        return x

    def factor_mult_batch_dev(self, x_dev_ptr, nvec, ldx=None, job=0, pivot_order=False):
        """spllt_hip_factor_mult_batch_dev: device vectors in place, the layout of solve_batch_dev.  Returns 0 or
        -20."""
        if ldx is None:
            ldx = self.n
        return self._call("spllt_hip_factor_mult_batch_dev", self.fkeep, int(nvec), C.c_void_p(x_dev_ptr), int(ldx), job,
                          1 if pivot_order else 0, ok=self._BATCH_OK)

    def _batch_mean(self, mean, where):
        """(array or None, ldmean) of a mean of shape (n,) -- shared by all members -- or (B, n)"""
        if mean is None:
            return None, 0
        m = np.ascontiguousarray(mean, dtype=np.float64)
        if m.shape == (self.n,):
            return m, 0
        if m.ndim != 2 or m.shape[1] != self.n:
            raise ValueError(f"{where}: mean must have shape (n,) or (B, n), n = {self.n}, not {m.shape}")
        nb = self._batch_count()
        if m.ndim == 2 and m.shape[1] == self.n and (nb <= 0 or m.shape[0] == nb):
            return m, max(self.n, 1)
        raise ValueError(f"{where}: mean must have shape (n,) or (B, n) = ({nb}, {self.n}), not {m.shape}")

    def sample_batch(self, nsamp, seed=0, kind="precision", mean=None, first_sample=0, stream0=0, common_noise=False):
        """spllt_hip_sample_batch: nsamp draws per member of the last batch of N(mean_b, A_b^-1) (kind
        "precision") or N(mean_b, A_b) ("covariance"), as a (B, nsamp, n) array in user order.  mean: (n,) for all
        members or (B, n).  Member b draws from noise stream stream0 + b; common_noise gives every member the
        noise of stream0.  The samples of a member that is not positive definite are NaN."""
        if int(nsamp) < 0:
            raise ValueError("sample_batch: nsamp < 0")
        k = self._sample_kind(kind)
        m, ldm = self._batch_mean(mean, "sample_batch")
        x = np.zeros((max(self._batch_count(), 0), int(nsamp), self.n), dtype=np.float64)
        self._call("spllt_hip_sample_batch", self.fkeep, int(nsamp), C.c_void_p(x.ctypes.data), max(self.n, 1), k,
                   int(seed), int(first_sample), int(stream0), 0 if common_noise else 1,
                   None if m is None else C.c_void_p(m.ctypes.data), ldm, ok=self._BATCH_OK)
        return x

    def sample_batch_dev(self, x_dev_ptr, nsamp, ldx=None, seed=0, kind="precision", mean_dev_ptr=None, ldmean=0,
                         first_sample=0, stream0=0, common_noise=False):
        """spllt_hip_sample_batch_dev: the samples into device memory, sample q of member b at
        x[(b*nsamp + q)*ldx .. + n); mean_dev_ptr: device doubles (ldmean 0: one mean, >= n: per member) or None.
        Returns 0 or -20."""
        if ldx is None:
            ldx = max(self.n, 1)
        return self._call("spllt_hip_sample_batch_dev", self.fkeep, int(nsamp), C.c_void_p(x_dev_ptr), int(ldx),
                          self._sample_kind(kind), int(seed), int(first_sample), int(stream0), 0 if common_noise else 1,
                          None if mean_dev_ptr is None else C.c_void_p(mean_dev_ptr), int(ldmean), ok=self._BATCH_OK)

    def white_noise_batch_dev(self, z_dev_ptr, nsamp, ldz=None, seed=0, first_sample=0, stream0=0, common_noise=False):
        """spllt_hip_white_noise_batch_dev: the standard normals the batched samplers use into device memory,
        sample q of member b at z[(b*nsamp + q)*ldz .. + n) in PIVOT order.  Returns 0 or -20."""
        if ldz is None:
            ldz = max(self.n, 1)
        return self._call("spllt_hip_white_noise_batch_dev", self.fkeep, int(nsamp), C.c_void_p(z_dev_ptr), int(ldz),
                          int(seed), int(first_sample), int(stream0), 0 if common_noise else 1, ok=self._BATCH_OK)

    def white_noise_batch(self, nsamp, seed, first_sample=0, stream0=0, common_noise=False):
        """white_noise_batch_dev, copied to the host: (B, n, nsamp), row p = pivot position p (member b's slice is
        what white_noise returns, for its stream)."""
        import torch
        if int(nsamp) < 0:
            raise ValueError("white_noise_batch: nsamp < 0")
        nb, n1 = max(self._batch_count(), 0), max(self.n, 1)
        z = torch.empty((max(nb, 1), int(nsamp), n1), dtype=torch.float64, device="cuda")
        self.white_noise_batch_dev(z.data_ptr(), nsamp, n1, seed, first_sample, stream0, common_noise)
        return np.ascontiguousarray(z.cpu().numpy()[:nb, :, :self.n].transpose(0, 2, 1))

    def release_factor_mult_batch(self):
        """The workspaces and the scratch of the batched products back to the device pool."""
        self._call("spllt_hip_release_factor_mult_batch", self.fkeep)
        return self

    # ---- blocked solve for the members of a batch (include/spllt_hip_batch_solve_many.h) -----
    def solve_many_batch(self, X, job=0):
        """spllt_hip_solve_many_batch on a copy of X: shape (B, n), one vector per member, or (B, nrhs, n), like
        solve_batch, whose numbers it gives to rounding.  A member's vectors go through the fp64 matrix cores in
        blocks of 32 (a tail of at most 16: a block of 16), its factor is read once per block: the call for many
        right-hand sides per member.  Measured: with 8 or more right-hand sides per member
        and 4 or more members it is 1.3 to 12 times faster than solve_batch; with ONE right-hand side per member and
        the backward sweep alone (job 2) solve_batch is faster (this path at 0.73-0.98 of it: a block of 16 is the
        least it runs), and so it is for a batch of one small matrix with well over 32 right-hand sides of job 2
        (0.57 on poisson2d_128 with 128).  job 0 / 1 / 2 as solve_batch.
        The vectors of a member that is not positive definite come back unchanged."""
        x = np.array(X, dtype=np.float64, order="C", copy=True)
        if x.ndim not in (2, 3):
            raise ValueError("solve_many_batch: X must have shape (B, n) or (B, nrhs, n)")
        nrhs = 1 if x.ndim == 2 else x.shape[1]
        if x.shape[-1] != self.n:
            raise ValueError(f"solve_many_batch: the vectors have length {x.shape[-1]}, n = {self.n}")
        nb = self._batch_count()
        if nb > 0 and x.shape[0] != nb:
            raise ValueError(f"solve_many_batch: X holds vectors for {x.shape[0]} members, the last batch has {nb}")
        self._call("spllt_hip_solve_many_batch", self.fkeep, nrhs, C.c_void_p(x.ctypes.data), x.shape[-1], job,
                   ok=self._BATCH_OK)
        return x

    def solve_many_batch_dev(self, x_dev_ptr, nrhs, ldx=None, job=0, pivot_order=False):
        """spllt_hip_solve_many_batch_dev: device vectors in place, the layout of solve_batch_dev.  Returns 0 or
        -20."""
        if int(nrhs) < 0:
            raise ValueError("solve_many_batch_dev: nrhs < 0")
        if ldx is None:
            ldx = self.n
        return self._call("spllt_hip_solve_many_batch_dev", self.fkeep, int(nrhs), C.c_void_p(x_dev_ptr), int(ldx), job,
                          1 if pivot_order else 0, ok=self._BATCH_OK)

    def set_batch_blocked_solve(self, on):
        """Route the backward sweep of sample_batch(kind="precision") through the blocked path (off by default;
        the samples agree to rounding).  Returns the previous setting."""
        return bool(self._call("spllt_hip_set_batch_blocked_solve", self.fkeep, 1 if on else 0))

    def solve_many_batch_info(self):
        """of the blocked batch solve: block width in use (0: no storage held), blocks per member and kernel
        launches of the last call, bytes of the workspace"""
        out = np.zeros(4, dtype=np.int64)
        self._call("spllt_hip_solve_many_batch_info", self.fkeep, out.ctypes.data_as(C.POINTER(C.c_int64)))
        return dict(zip(("rb", "blocks", "launches", "workspace_bytes"), (int(v) for v in out)))

    def release_solve_many_batch(self):
        """The workspace of the blocked batch solve back to the device pool."""
        self._call("spllt_hip_release_solve_many_batch", self.fkeep)
        return self

    # ---- the bit-reproducible batch (include/spllt_hip_batch_repro.h) -----
    def set_batch_reproducible(self, on):
        """on: factor_batch runs the deterministic batch program and EVERY sweep over the members of a batch
        (solve_batch, solve_many_batch, the constrained family, sample_batch(kind="precision"), the preconditioner of
        solve_refined_batch) runs the reproducible blocked kernels: a member's bits depend on its values and vectors
        alone, not on the run, on B, on its place in the batch or on the other vectors.  Off
        by default; flipping it keeps an existing batch.  Returns the previous setting."""
        return bool(self._call("spllt_hip_set_batch_reproducible", self.fkeep, 1 if on else 0))

    def solve_reproducible_batch(self, X, job=0):
        """spllt_hip_solve_repro_batch on a copy of X, shapes and jobs as solve_many_batch: the reproducible sweep
        whatever set_batch_reproducible says.  The vectors of a member that is not positive definite come back
        unchanged."""
        x = np.array(X, dtype=np.float64, order="C", copy=True)
        if x.ndim not in (2, 3):
            raise ValueError("solve_reproducible_batch: X must have shape (B, n) or (B, nrhs, n)")
        nrhs = 1 if x.ndim == 2 else x.shape[1]
        if x.shape[-1] != self.n:
            raise ValueError(f"solve_reproducible_batch: the vectors have length {x.shape[-1]}, n = {self.n}")
        nb = self._batch_count()
        if nb > 0 and x.shape[0] != nb:
            raise ValueError(f"solve_reproducible_batch: X holds vectors for {x.shape[0]} members, the last batch has {nb}")
        self._call("spllt_hip_solve_repro_batch", self.fkeep, nrhs, C.c_void_p(x.ctypes.data), x.shape[-1], job,
                   ok=self._BATCH_OK)
        return x

    def solve_reproducible_batch_dev(self, x_dev_ptr, nrhs, ldx=None, job=0, pivot_order=False):
        """spllt_hip_solve_repro_batch_dev: device vectors in place, the layout of solve_batch_dev.  Returns 0 or
        -20."""
        if int(nrhs) < 0:
            raise ValueError("solve_reproducible_batch_dev: nrhs < 0")
        if ldx is None:
            ldx = self.n
        return self._call("spllt_hip_solve_repro_batch_dev", self.fkeep, int(nrhs), C.c_void_p(x_dev_ptr), int(ldx), job,
                          1 if pivot_order else 0, ok=self._BATCH_OK)

    def batch_repro_info(self):
        """the switch, whether the last batch was factorized by the deterministic program, the kernel launches of that
        factorization, the width of the last block of the last reproducible sweep, bytes of the factor scratch and of
        the sweep scratch"""
        out = np.zeros(6, dtype=np.int64)
        self._call("spllt_hip_batch_repro_info", self.fkeep, out.ctypes.data_as(C.POINTER(C.c_int64)))
        return dict(zip(("on", "deterministic_factor", "factor_launches", "sweep_rb", "factor_scratch_bytes",
                         "sweep_scratch_bytes"), (int(v) for v in out)))

    def release_batch_repro(self):
        """The scratch and the tables of the reproducible sweep back to the device pool."""
        self._call("spllt_hip_release_batch_repro", self.fkeep)
        return self

    # ---- update / downdate of the factors of a batch (include/spllt_hip_updown_batch.h) -----
    def _updown_batch_pattern(self, W, where):
        """W (scipy sparse n x k) as the 1-based CSC arrays of the C interface and its values, in canonical CSC order
        (rows ascending within a column, duplicates summed); stored zeros stay: W gives the PATTERN"""
        import scipy.sparse as sp
        if not sp.issparse(W):
            raise ValueError(f"{where}: W must be a scipy sparse n x k matrix (it gives the pattern)")
        if W.shape[0] != self.n:
            raise ValueError(f"{where}: W has {W.shape[0]} rows, n = {self.n}")
        W = sp.csc_matrix(W, dtype=np.float64, copy=True)
        W.sum_duplicates()
        W.sort_indices()
        return (W.shape[1], np.ascontiguousarray(W.indptr + 1, dtype=np.int32),
                np.ascontiguousarray(np.append(W.indices + 1, 0), dtype=np.int32),
                np.ascontiguousarray(W.data, dtype=np.float64))

    def update_batch(self, W, vals=None, downdate=False):
        """spllt_hip_updown_batch: the factors of A_b + W_b W_b^T (downdate: A_b - W_b W_b^T) in place of those of the
        last batch.  W (scipy sparse, n x k) gives the ONE pattern; vals of shape (B, nnz(W)) holds member b's values
        in W's CSC order (rows ascending within a column); vals=None: W's own values for every member.  The pattern
        of every column must be a clique of the analysed matrix (include/spllt_hip.h, spllt_hip_updown).  Returns 0,
        or -20 when a member is not positive definite (batch_status() tells which; the others are served)."""
        where = "update_batch"
        k, ptr, row, wdata = self._updown_batch_pattern(W, where)
        nent = int(wdata.size)
        nb = self._batch_count()
        if vals is None:
            vals = np.tile(wdata, (max(nb, 1), 1))
        vals = np.ascontiguousarray(vals, dtype=np.float64)
        if vals.ndim != 2 or vals.shape[1] != nent:
            raise ValueError(f"{where}: vals must have shape (B, nnz(W)) = (B, {nent}), not {vals.shape}")
        if nb > 0 and vals.shape[0] != nb:
            raise ValueError(f"{where}: vals holds values for {vals.shape[0]} members, the last batch has {nb}")
        if nent == 0:
            vals = np.zeros((vals.shape[0], 1))
        return self._call("spllt_hip_updown_batch", self.fkeep, k, _ip(ptr), _ip(row), C.c_void_p(vals.ctypes.data),
                          int(vals.shape[1]), -1 if downdate else 1, ok=self._BATCH_OK)

    def update_batch_dev(self, W, vals_ptr, ldw, downdate=False):
        """spllt_hip_updown_batch_dev: the same with the values in HBM (integer device pointer; member b's value of
        CSC position e at ptr + (b * ldw + e) doubles, ldw >= nnz(W)).  The library reads the values of EVERY member of
        the last batch.  Returns 0 or -20."""
        k, ptr, row, wdata = self._updown_batch_pattern(W, "update_batch_dev")
        if int(ldw) < int(wdata.size):
            raise ValueError(f"update_batch_dev: ldw = {ldw} < nnz(W) = {wdata.size}")
        return self._call("spllt_hip_updown_batch_dev", self.fkeep, k, _ip(ptr), _ip(row), C.c_void_p(vals_ptr), int(ldw),
                          -1 if downdate else 1, ok=self._BATCH_OK)

    def updown_batch_info(self):
        """of the last update_batch(): block columns visited, entries of L in them per member, kernel launches, passes,
        members served, members that failed in that call"""
        out = np.zeros(6, dtype=np.int64)
        self._call("spllt_hip_updown_batch_info", self.fkeep, out.ctypes.data_as(C.POINTER(C.c_int64)))
        return dict(zip(("bcols", "entries", "launches", "passes", "served", "failed"), (int(v) for v in out)))

    def updown_batch_device_ms(self):
        """spllt_hip_updown_batch_time: device time of the last update_batch(), first scatter to last kernel"""
        v = C.c_double()
        self._call("spllt_hip_updown_batch_time", self.fkeep, C.byref(v))
        return v.value

    def release_updown_batch(self):
        """The work arrays of update_batch back to the device pool."""
        self._call("spllt_hip_release_updown_batch", self.fkeep)
        return self

    # ---- sparse right-hand sides for the members of a batch (include/spllt_hip_solve_sparse_batch.h) -----
    solve_sparse_batch_status = None     # return value (0 or -20) of the last host call of this family

    def _sparse_batch_columns(self, B, vals, where):
        """B (scipy sparse n x k) as the 1-based CSC arrays of the C interface, in canonical CSC order (rows ascending
        within a column, duplicates summed; stored zeros stay: B gives the PATTERN), and (values, ldb): B's own for
        every member (ldb 0) or vals of shape (nbatch, nnz(B)) in that order.  Refuses before any library call."""
        import scipy.sparse as sp
        if not sp.issparse(B):
            raise ValueError(f"{where}: B must be a scipy sparse n x k matrix (it gives the pattern)")
        if B.shape[0] != self.n:
            raise ValueError(f"{where}: B has {B.shape[0]} rows, n = {self.n}")
        B = sp.csc_matrix(B, dtype=np.float64, copy=True)
        B.sum_duplicates()
        B.sort_indices()
        nent = int(B.data.size)
        ptr = np.ascontiguousarray(B.indptr + 1, dtype=np.int32)
        row = np.ascontiguousarray(np.append(B.indices + 1, 0), dtype=np.int32)
        if vals is None:
            return B.shape[1], ptr, row, np.ascontiguousarray(np.append(B.data, 0.0), dtype=np.float64), 0
        vals = np.ascontiguousarray(vals, dtype=np.float64)
        if vals.ndim != 2 or vals.shape[1] != nent:
            raise ValueError(f"{where}: vals must have shape (B, nnz(B)) = (B, {nent}), not {vals.shape}")
        nb = self._batch_count()
        if nb > 0 and vals.shape[0] != nb:
            raise ValueError(f"{where}: vals holds values for {vals.shape[0]} members, the last batch has {nb}")
        if nent == 0:
            vals = np.zeros((vals.shape[0], 1))
        return B.shape[1], ptr, row, vals, int(vals.shape[1])

    def _wanted_checked(self, rows, where):
        if rows is not None:
            r = np.asarray(rows)
            if r.ndim > 1 or (r.size and not np.issubdtype(r.dtype, np.integer)):
                raise ValueError(f"{where}: rows must be a one-dimensional list of 0-based variables")
            if r.size and (int(r.min()) < 0 or int(r.max()) >= self.n):
                raise ValueError(f"{where}: a wanted row is outside [0, n)")
        return self._wanted(rows)

    def solve_sparse_batch(self, B, rows=None, job=0, vals=None):
        """spllt_hip_solve_sparse_batch: A_b^-1 B_b (job 1: L_b^-1 P B_b, job 2: the backward sweep) for every member of
        the last batch, at the 0-based variables `rows` (None: all n).  B (scipy sparse, n x k) gives the ONE pattern;
        vals of shape (nbatch, nnz(B)) holds member b's values in B's CSC order, None: B's own for every member.
        Returns (nbatch, len(rows) or n, k), a view whose columns are contiguous; a member that is not positive
        definite is NaN (solve_sparse_batch_status is then -20)."""
        where = "solve_sparse_batch"
        if job not in (0, 1, 2):
            raise ValueError(f"{where}: job must be 0, 1 or 2")
        k, ptr, row, v, ldb = self._sparse_batch_columns(B, vals, where)
        nsel, sel = self._wanted_checked(rows, where)
        m = self.n if sel is None else nsel
        nb = self._batch_count()
        x = np.zeros((max(nb, 1), max(k, 1), max(m, 1)), dtype=np.float64)
        self.solve_sparse_batch_status = self._call(
            "spllt_hip_solve_sparse_batch", self.fkeep, k, _ip(ptr), _ip(row), _dp(v), ldb, nsel,
            None if sel is None else _ip(sel), _dp(x), x.shape[2], job, ok=self._BATCH_OK)
        # (a view: member b's column q is the contiguous x[b, q]; no second pass over nbatch * k * nout doubles)
        return x[:nb, :k, :m].transpose(0, 2, 1)

    def solve_sparse_batch_dev(self, B, x_dev_ptr, ldx, rows=None, job=0, vals=None):
        """spllt_hip_solve_sparse_batch_dev: the same into device memory, column q of member b at
        x[(b*k + q)*ldx .. + (len(rows) or n)); nothing else is written.  Returns 0 or -20."""
        where = "solve_sparse_batch_dev"
        k, ptr, row, v, ldb = self._sparse_batch_columns(B, vals, where)
        nsel, sel = self._wanted_checked(rows, where)
        if int(ldx) < (self.n if sel is None else nsel):
            raise ValueError(f"{where}: ldx = {ldx} is smaller than the number of wanted entries")
        return self._call("spllt_hip_solve_sparse_batch_dev", self.fkeep, k, _ip(ptr), _ip(row), _dp(v), ldb, nsel,
                          None if sel is None else _ip(sel), C.c_void_p(x_dev_ptr), int(ldx), job, ok=self._BATCH_OK)

    def gram_batch(self, B, vals=None):
        """spllt_hip_gram_sparse_batch: B_b^T A_b^-1 B_b for every member, (nbatch, k, k), each exactly symmetric;
        B and vals as in solve_sparse_batch."""
        where = "gram_batch"
        k, ptr, row, v, ldb = self._sparse_batch_columns(B, vals, where)
        nb = self._batch_count()
        G = np.zeros((max(nb, 1), max(k, 1), max(k, 1)), dtype=np.float64)
        self.solve_sparse_batch_status = self._call("spllt_hip_gram_sparse_batch", self.fkeep, k, _ip(ptr), _ip(row), _dp(v),
                                                    ldb, _dp(G), G.shape[2], ok=self._BATCH_OK)
        # (member b's column j is row j of G[b]; the matrices are symmetric)
        return np.ascontiguousarray(G[:nb, :k, :k].transpose(0, 2, 1))

    def gram_batch_dev(self, B, g_dev_ptr, ldg, vals=None):
        """spllt_hip_gram_sparse_batch_dev: G_b column-major at g + b*k*ldg doubles.  Returns 0 or -20."""
        where = "gram_batch_dev"
        k, ptr, row, v, ldb = self._sparse_batch_columns(B, vals, where)
        if int(ldg) < k:
            raise ValueError(f"{where}: ldg = {ldg} < k = {k}")
        return self._call("spllt_hip_gram_sparse_batch_dev", self.fkeep, k, _ip(ptr), _ip(row), _dp(v), ldb,
                          C.c_void_p(g_dev_ptr), int(ldg), ok=self._BATCH_OK)

    def inverse_block_batch(self, i, j):
        """A_b^-1[i][:, j] for every member and any 0-based index sets i, j, inside the pattern of L or not: sparse
        solves with the unit columns e_j and the wanted rows i; (nbatch, len(i), len(j))."""
        import scipy.sparse as sp
        i = np.asarray(i, dtype=np.int64).ravel()
        j = np.asarray(j, dtype=np.int64).ravel()
        if ((i < 0) | (i >= self.n)).any() or ((j < 0) | (j >= self.n)).any():
            raise ValueError("inverse_block_batch: index out of range")
        E = sp.csc_matrix((np.ones(len(j)), (j, np.arange(len(j)))), shape=(self.n, len(j)))
        return self.solve_sparse_batch(E, rows=i)

    def solve_sparse_batch_info(self):
        """of the last solve_sparse_batch / gram_batch: the fields of solve_sparse_info (block columns and doubles of
        L per member, kernel launches, workgroups of the sweeps summed over the members), members served and flagged"""
        out = np.zeros(8, dtype=np.int64)
        self._call("spllt_hip_solve_sparse_batch_info", self.fkeep, out.ctypes.data_as(C.POINTER(C.c_int64)))
        return dict(zip(("fwd_bcols", "bwd_bcols", "fwd_entries", "bwd_entries", "launches", "workgroups", "served",
                         "flagged"), (int(v) for v in out)))

    def release_solve_sparse_batch(self):
        """The staged tables, the output buffer and the gram workspaces of the batch back to the device pool."""
        self._call("spllt_hip_release_solve_sparse_batch", self.fkeep)
        return self

    # ---- the product and the refined solves for the members of a batch (include/spllt_hip_batch_refine.h) -----
    def _batch_values(self, vals, where):
        vals = np.ascontiguousarray(vals, dtype=np.float64)
        if vals.ndim != 2 or vals.shape[1] != self.nnz:
            raise ValueError(f"{where}: vals must have shape (B, nnz) = (B, {self.nnz}), not {vals.shape}")
        return vals

    def _batch_vectors(self, X, nb, where):
        """a C-ordered copy of X, shape (B, n) or (B, nvec, n) with B = nb, and nvec"""
        x = np.array(X, dtype=np.float64, order="C", copy=True)
        if x.ndim not in (2, 3):
            raise ValueError(f"{where}: the vectors must have shape (B, n) or (B, nvec, n)")
        if x.shape[-1] != self.n:
            raise ValueError(f"{where}: the vectors have length {x.shape[-1]}, n = {self.n}")
        if x.shape[0] != nb:
            raise ValueError(f"{where}: vectors for {x.shape[0]} members, values for {nb}")
        return x, (1 if x.ndim == 2 else x.shape[1])

    def matvec_batch(self, vals, X):
        """spllt_hip_matvec_batch: y_b = A_b x_b on the device with A_b = (the analysed pattern, vals[b]); vals of
        shape (B, nnz), X of shape (B, n) or (B, nvec, n), like solve_batch.  Member b's product is bit-identical
        to matvec(vals[b], ...), and two calls return bit-identical results.  Needs neither a factor nor a batch."""
        vals = self._batch_values(vals, "matvec_batch")
        x, nvec = self._batch_vectors(X, vals.shape[0], "matvec_batch")
        y = np.empty_like(x)
        ld = max(1, self.n)
        self._call("spllt_hip_matvec_batch", self.fkeep, vals.shape[0], self.nnz, _dp(vals), max(1, self.nnz), nvec,
                   _dp(x), ld, _dp(y), ld)
        return y

    def matvec_batch_dev(self, val_dev_ptr, nbatch, x_dev_ptr, y_dev_ptr, nvec, ldval=None, ldx=None, ldy=None,
                         pivot_order=False):
        """spllt_hip_matvec_batch_dev: the product on device arrays (member b's values at val + b*ldval, vector q
        of member b at x[(b*nvec + q)*ldx .. + n), y alike; pivot_order as solve_many_dev; x and y must not
        overlap)."""
        self._call("spllt_hip_matvec_batch_dev", self.fkeep, int(nbatch), self.nnz, C.c_void_p(val_dev_ptr),
                   int(self.nnz if ldval is None else ldval), int(nvec), C.c_void_p(x_dev_ptr),
                   int(self.n if ldx is None else ldx), C.c_void_p(y_dev_ptr), int(self.n if ldy is None else ldy),
                   1 if pivot_order else 0)
        return self

    def solve_refined_batch(self, vals, B, method="pcg", tol=1e-14, max_iter=50):
        """spllt_hip_solve_refined_batch on a copy of B (shape (B, n) or (B, nrhs, n), like solve_batch): solve
        A_b x = b for A_b = (pattern, vals[b]) with the factor of member b of the last factor_batch as
        preconditioner, to the backward error tol, all members in one set of launches.  method "ir" or "pcg".
        Returns (x, iterations, error) of shapes (B, nrhs, n), (B, nrhs) and (B, nrhs): as solve_refined per pair.
        A member that is not positive definite keeps its vectors, with iterations 0 and error NaN.
        self.refine_status keeps the call's return value (0: every pair reached tol, 1: at least one did not,
        -20: a member is not positive definite -- the others were served; other negative flags raise)."""
        if method not in self._METHODS:
            raise SplltError("spllt_hip_solve_refined_batch", -10, "method is not 'ir' or 'pcg'")
        vals = self._batch_values(vals, "solve_refined_batch")
        nb = self._batch_count()
        if nb > 0 and vals.shape[0] != nb:
            raise ValueError(f"solve_refined_batch: values for {vals.shape[0]} members, the last batch has {nb}")
        x, nrhs = self._batch_vectors(B, vals.shape[0], "solve_refined_batch")
        x = x.reshape(vals.shape[0], nrhs, self.n)
        it = np.zeros(max(1, x.shape[0] * nrhs), dtype=np.int32)
        err = np.zeros(max(1, x.shape[0] * nrhs), dtype=np.float64)
        rc = self.lib.spllt_hip_solve_refined_batch(self.fkeep, self.nnz, _dp(vals), max(1, self.nnz), nrhs, _dp(x),
                                                    max(1, self.n), self._METHODS[method], float(tol), int(max_iter),
                                                    _ip(it), _dp(err))
        self.refine_status = rc
        if rc < 0 and rc not in self._BATCH_OK:
            raise SplltError("spllt_hip_solve_refined_batch", rc, self.last_error())
        shape = (x.shape[0], nrhs)
        return x, it[:x.shape[0] * nrhs].reshape(shape), err[:x.shape[0] * nrhs].reshape(shape)

    def solve_refined_batch_dev(self, val_dev_ptr, x_dev_ptr, nrhs, ldval=None, ldx=None, method="pcg", tol=1e-14,
                                max_iter=50):
        """spllt_hip_solve_refined_batch_dev: values and vectors on the device (user order, in place), the layout
        of solve_batch_dev.  Returns (status, iterations, error) with arrays of shape (B, nrhs); status 0: every
        pair reached tol, 1: at least one did not, -20: a member is not positive definite."""
        if method not in self._METHODS:
            raise SplltError("spllt_hip_solve_refined_batch_dev", -10, "method is not 'ir' or 'pcg'")
        if int(nrhs) < 0:
            raise ValueError("solve_refined_batch_dev: nrhs < 0")
        nb = max(self._batch_count(), 0)
        it = np.zeros(max(1, nb * nrhs), dtype=np.int32)
        err = np.zeros(max(1, nb * nrhs), dtype=np.float64)
        rc = self._call("spllt_hip_solve_refined_batch_dev", self.fkeep, self.nnz, C.c_void_p(val_dev_ptr),
                        int(self.nnz if ldval is None else ldval), int(nrhs), C.c_void_p(x_dev_ptr),
                        int(self.n if ldx is None else ldx), self._METHODS[method], float(tol), int(max_iter),
                        _ip(it), _dp(err), ok=self._BATCH_OK)
        self.refine_status = rc
        return rc, it[:nb * nrhs].reshape(nb, nrhs), err[:nb * nrhs].reshape(nb, nrhs)

    def solve_refined_batch_info(self):
        """of the refined batch solve: pass width the storage holds (0: none held), passes and kernel launches of
        the last call (this family's and the sweeps'), bytes of the storage"""
        out = np.zeros(4, dtype=np.int64)
        self._call("spllt_hip_solve_refined_batch_info", self.fkeep, out.ctypes.data_as(C.POINTER(C.c_int64)))
        return dict(zip(("width", "passes", "launches", "workspace_bytes"), (int(v) for v in out)))

    def release_refine_batch(self):
        """The work arrays of the refined batch solve back to the device pool."""
        self._call("spllt_hip_release_refine_batch", self.fkeep)
        return self

    # ---- batched selected inversion -------------------------------------------
    def selected_inverse_batch(self):
        """spllt_hip_selected_inverse_batch: Z_b on the pattern of L for every member of the last batch.
        Returns 0, or -20 when a member is not positive definite (the others are inverted)."""
        return self._call("spllt_hip_selected_inverse_batch", self.fkeep, ok=self._BATCH_OK)

    def get_inverse_batch(self, member, out=None):
        """one member's Z arena on the host (the layout of get_inverse); a failed member raises (-20)"""
        arena = self.sym_info()["arena"]
        if out is None:
            out = np.zeros(max(arena, 1), dtype=np.float64)
        assert out.dtype == np.float64 and out.size >= arena and out.flags["C_CONTIGUOUS"]
        self._call("spllt_hip_get_inverse_batch", self.fkeep, int(member), _dp(out), arena)
        return out[:arena]

    def device_inverse_batch_ptr(self):
        """(device pointer of member 0's Z arena, member stride in doubles)"""
        stride = C.c_int64()
        p = self.lib.spllt_hip_device_inverse_batch(self.fkeep, C.byref(stride))
        return p, stride.value

    def _batch_rows(self, name, width):
        nb = self.lib.spllt_hip_batch_status(self.fkeep, None, None, 0)
        out = np.zeros((max(nb, 1), max(width, 1)), dtype=np.float64)
        self._call(name, self.fkeep, _dp(out), out.shape[1])
        return out[:nb, :width]

    def inverse_diag_batch(self):
        """(A_b^-1)_ii in the user's variable order, shape (nbatch, n); NaN rows for failed members"""
        return self._batch_rows("spllt_hip_inverse_diag_batch", self.n)

    def inverse_on_pattern_batch(self):
        """(A_b^-1) at the entries of the analysed pattern in the order of val, shape (nbatch, nnz); NaN
        rows for failed members"""
        return self._batch_rows("spllt_hip_inverse_on_pattern_batch", self.nnz)

    def inverse_on_pattern_batch_dev(self, out_dev_ptr, ldout=None):
        """spllt_hip_inverse_on_pattern_batch_dev: the same rows into device memory, out[b*ldout + k]"""
        self._call("spllt_hip_inverse_on_pattern_batch_dev", self.fkeep, C.c_void_p(out_dev_ptr),
                   int(self.nnz if ldout is None else ldout))
        return self

    def batch_selinv_launches(self):
        """kernel launches of the last batched inversion"""
        return int(self.lib.spllt_hip_batch_selinv_launches(self.fkeep))

    def release_inverse_batch(self):
        self._call("spllt_hip_release_inverse_batch", self.fkeep)

    # ---- hard linear constraints for the members of a batch (include/spllt_hip_constrain_batch.h) -----
    def set_constraints_batch(self, C_rows):
        """spllt_hip_set_constraints_batch: store the k <= 64 dense rows of ONE C (k x n, or n for one row) for all
        members of the last batch and build U_b, G_b per member.  They stay with the handle across batches: a later
        factor_batch is picked up by the next call that needs them.  None or zero rows clear the constraints.
        Dependent rows in any factorized member raise SplltError with flag -20 (the message names the member and the
        row) and leave the batch without constraints.  A member that is not positive definite holds none; the
        others do (self.constrain_batch_status keeps the call's 0 or -20)."""
        if C_rows is None:
            self._call("spllt_hip_set_constraints_batch", self.fkeep, 0, None, max(self.n, 1))
            return self
        c = np.ascontiguousarray(np.atleast_2d(np.asarray(C_rows, dtype=np.float64)))
        if c.ndim != 2 or (c.shape[0] and c.shape[1] != self.n):
            raise ValueError(f"set_constraints_batch: C must be (k, {self.n}), got {c.shape}")
        rc = self._call("spllt_hip_set_constraints_batch", self.fkeep, c.shape[0], _dp(c) if c.shape[0] else None,
                        max(self.n, 1), ok=self._BATCH_OK)
        if rc == -20 and c.shape[0] and self.constraints_batch_info()["k"] == 0:
            raise SplltError("spllt_hip_set_constraints_batch", rc, self.last_error())
        self.constrain_batch_status = rc
        return self

    def set_constraints_batch_dev(self, c_dev_ptr, k, ldc=None):
        """spllt_hip_set_constraints_batch_dev: row i of C at c[i*ldc .. i*ldc + n) in device memory.  Returns 0 or
        -20 (see constraints_batch_info()["k"]: 0 after dependent rows)."""
        return self._call("spllt_hip_set_constraints_batch_dev", self.fkeep, int(k), C.c_void_p(c_dev_ptr),
                          int(self.n if ldc is None else ldc), ok=self._BATCH_OK)

    def _constrain_batch_call(self, name, X, e, multipliers):
        where = name[len("spllt_hip_"):]
        nb = self._batch_count()
        x = np.array(X, dtype=np.float64, order="C", copy=True)
        if x.ndim not in (2, 3):
            raise ValueError(f"{where}: the vectors must have shape (B, n) or (B, nvec, n)")
        if x.shape[-1] != self.n:
            raise ValueError(f"{where}: the vectors have length {x.shape[-1]}, n = {self.n}")
        if nb > 0 and x.shape[0] != nb:
            raise ValueError(f"{where}: vectors for {x.shape[0]} members, the last batch has {nb}")
        nvec = 1 if x.ndim == 2 else x.shape[1]
        k = self.constraints_batch_info()["k"]
        ev, lde = None, 0
        if e is not None:
            ev = np.ascontiguousarray(e, dtype=np.float64)
            if ev.shape not in ((k,), (x.shape[0], nvec, k)):
                raise ValueError(f"{where}: e must be ({k},) or ({x.shape[0]}, {nvec}, {k}), got {ev.shape}")
            lde = k if ev.ndim == 3 else 0     # (one column per vector, else one shared column)
        lam = np.zeros((x.shape[0], nvec, max(k, 1)), dtype=np.float64) if multipliers else None
        self.constrain_batch_status = self._call(
            name, self.fkeep, nvec, C.c_void_p(x.ctypes.data), max(self.n, 1),
            None if ev is None else C.c_void_p(ev.ctypes.data), lde,
            None if lam is None else C.c_void_p(lam.ctypes.data), max(k, 1), ok=self._BATCH_OK)
        if not multipliers:
            return x
        lam = lam[..., :k]
        return x, (lam[:, 0] if x.ndim == 2 else lam)

    def constrain_batch(self, X, e=None, multipliers=False):
        """spllt_hip_constrain_batch on a copy of X ((B, n) or (B, nvec, n), like solve_many_batch): per member
        x* = x - U_b G_b^-1 (C x - e), so that C x* = e.  e: None (zeros), (k,) shared by every vector of every member,
        or (B, nvec, k).  multipliers=True also returns lambda = S_b^-1 (C x - e), shape (B, k) or (B, nvec, k).  The
        vectors of a member that is not positive definite come back unchanged, its multipliers NaN."""
        return self._constrain_batch_call("spllt_hip_constrain_batch", X, e, multipliers)

    def solve_constrained_batch(self, B, e=None, multipliers=False):
        """spllt_hip_solve_constrained_batch on a copy of B: constrain_batch(solve_many_batch(B), e) in one call; with
        multipliers=True (x, lambda) solves A_b x + C^T lambda = b, C x = e for every member."""
        return self._constrain_batch_call("spllt_hip_solve_constrained_batch", B, e, multipliers)

    def _constrain_batch_targets(self, e, where):
        if e is None:
            return None
        ev = np.ascontiguousarray(e, dtype=np.float64)
        if ev.shape != (self.constraints_batch_info()["k"],):
            raise ValueError(f"{where}: e must hold one target per constraint")
        return ev

    def sample_constrained_batch(self, nsamp, seed=0, mean=None, e=None, first_sample=0, stream0=0, common_noise=False):
        """spllt_hip_sample_constrained_batch: nsamp draws per member of N(mean_b, A_b^-1) | C x = e as a (B, nsamp, n)
        array: the samples of sample_batch(kind="precision") with the same arguments, corrected.  e: None or (k,).
        The samples of a member that is not positive definite are NaN."""
        if int(nsamp) < 0:
            raise ValueError("sample_constrained_batch: nsamp < 0")
        m, ldm = self._batch_mean(mean, "sample_constrained_batch")
        ev = self._constrain_batch_targets(e, "sample_constrained_batch")
        x = np.zeros((max(self._batch_count(), 0), int(nsamp), self.n), dtype=np.float64)
        self.constrain_batch_status = self._call(
            "spllt_hip_sample_constrained_batch", self.fkeep, int(nsamp), C.c_void_p(x.ctypes.data), max(self.n, 1),
            int(seed), int(first_sample), int(stream0), 0 if common_noise else 1,
            None if m is None else C.c_void_p(m.ctypes.data), ldm, None if ev is None else C.c_void_p(ev.ctypes.data),
            ok=self._BATCH_OK)
        return x

    def constrain_batch_dev(self, x_dev_ptr, nvec, ldx=None, e_dev_ptr=None, lde=0, lambda_dev_ptr=None, ldl=0,
                            entry="constrain"):
        """spllt_hip_constrain_batch_dev / spllt_hip_solve_constrained_batch_dev (entry="solve_constrained") on device
        vectors, in place: vector q of member b at x[(b*nvec + q)*ldx .. + n), e and lambda alike.  Returns 0 or
        -20."""
        return self._call(f"spllt_hip_{entry}_batch_dev", self.fkeep, int(nvec), C.c_void_p(x_dev_ptr),
                          int(self.n if ldx is None else ldx), None if e_dev_ptr is None else C.c_void_p(e_dev_ptr),
                          int(lde), None if lambda_dev_ptr is None else C.c_void_p(lambda_dev_ptr), int(ldl),
                          ok=self._BATCH_OK)

    def sample_constrained_batch_dev(self, x_dev_ptr, nsamp, ldx=None, seed=0, mean_dev_ptr=None, ldmean=0, e_dev_ptr=None,
                                     first_sample=0, stream0=0, common_noise=False):
        """spllt_hip_sample_constrained_batch_dev: the constrained samples into device memory (layout of
        sample_batch_dev).  Returns 0 or -20."""
        return self._call("spllt_hip_sample_constrained_batch_dev", self.fkeep, int(nsamp), C.c_void_p(x_dev_ptr),
                          int(max(self.n, 1) if ldx is None else ldx), int(seed), int(first_sample), int(stream0),
                          0 if common_noise else 1, None if mean_dev_ptr is None else C.c_void_p(mean_dev_ptr),
                          int(ldmean), None if e_dev_ptr is None else C.c_void_p(e_dev_ptr), ok=self._BATCH_OK)

    def inverse_diag_constrained_batch(self):
        """Var(x_i | C x = e) = (A_b^-1)_ii - sum_j U_b[i, j]^2 per member, shape (nbatch, n), user order; needs
        selected_inverse_batch() of the current batch.  NaN rows for members that are not positive definite."""
        nb = self._batch_count()
        out = np.zeros((max(nb, 1), max(self.n, 1)), dtype=np.float64)
        self.constrain_batch_status = self._call("spllt_hip_inverse_diag_constrained_batch", self.fkeep, _dp(out),
                                                 out.shape[1], ok=self._BATCH_OK)
        return out[:nb, :self.n]

    def constraints_batch_info(self):
        """k (0: none set), rebuilds of the U_b, device bytes, kernel launches of the family in the last call, and per
        member of the last batch log det S_b and the smallest relative pivot of S_b (NaN for a member that is not
        positive definite, or until the first call after a new batch has rebuilt them; empty without constraints)."""
        out = np.zeros(4, dtype=np.int64)
        nb = max(self._batch_count(), 0)
        stat = np.zeros((max(nb, 1), 2), dtype=np.float64)
        self._call("spllt_hip_constraints_batch_info", self.fkeep, out.ctypes.data_as(C.POINTER(C.c_int64)), _dp(stat), 2)
        have = nb if out[0] > 0 else 0
        return {"k": int(out[0]), "rebuilds": int(out[1]), "device_bytes": int(out[2]), "launches": int(out[3]),
                "log_det_s": stat[:have, 0].copy(), "min_relative_pivot": stat[:have, 1].copy()}

    def release_constraints_batch(self):
        """C, the U_b and the work arrays of the batch's constraints back to the device pool; C is forgotten."""
        self._call("spllt_hip_release_constraints_batch", self.fkeep)
        return self

    # ---- factor adjoint of the members of a batch (include/spllt_hip_batch_adjoint.h) ----
    def factor_adjoint_seed_batch(self, a, b, alpha=1.0, accumulate=False, a_pivot_order=False, b_pivot_order=False):
        """spllt_hip_factor_adjoint_seed_batch on host arrays a, b of shape (B, n), one vector per member, or
        (B, nvec, n), like solve_batch: Lbar_b (+)= alpha sum_q a_bq b_bq^T on the lower positions of L_b; a
        vector is in the user's variable order unless its flag says pivot order"""
        a = np.ascontiguousarray(a, dtype=np.float64)
        b = np.ascontiguousarray(b, dtype=np.float64)
        if a.shape != b.shape or a.ndim not in (2, 3) or a.shape[-1] != self.n:
            raise ValueError("factor_adjoint_seed_batch: a and b must both have shape (B, n) or (B, nvec, n)")
        nb = self._batch_count()
        if nb > 0 and a.shape[0] != nb:
            raise ValueError(f"factor_adjoint_seed_batch: vectors for {a.shape[0]} members, the last batch has {nb}")
        nvec = 1 if a.ndim == 2 else a.shape[1]
        self._call("spllt_hip_factor_adjoint_seed_batch", self.fkeep, nvec, _dp(a), _dp(b), max(self.n, 1), float(alpha),
                   1 if accumulate else 0, self._order_flags(a_pivot_order, b_pivot_order))
        return self

    def factor_adjoint_seed_batch_dev(self, a_dev_ptr, b_dev_ptr, nvec, ld=None, alpha=1.0, accumulate=False,
                                      a_pivot_order=False, b_pivot_order=False):
        """spllt_hip_factor_adjoint_seed_batch_dev: the seed from device vectors, vector q of member b at
        a[(b*nvec + q)*ld .. + n)"""
        if ld is None:
            ld = self.n
        self._call("spllt_hip_factor_adjoint_seed_batch_dev", self.fkeep, int(nvec), C.c_void_p(a_dev_ptr),
                   C.c_void_p(b_dev_ptr), int(ld), float(alpha), 1 if accumulate else 0,
                   self._order_flags(a_pivot_order, b_pivot_order))
        return self

    def set_factor_adjoint_batch(self, arenas):
        """spllt_hip_set_factor_adjoint_batch: an arbitrary Lbar_b for every member, shape (B, >= arena), each row
        in the layout of get_factor_batch"""
        arenas = np.ascontiguousarray(arenas, dtype=np.float64)
        if arenas.ndim != 2:
            raise ValueError("set_factor_adjoint_batch: arenas must have shape (B, arena)")
        nb = self._batch_count()
        if nb > 0 and arenas.shape[0] != nb:
            raise ValueError(f"set_factor_adjoint_batch: arenas for {arenas.shape[0]} members, the last batch has {nb}")
        self._call("spllt_hip_set_factor_adjoint_batch", self.fkeep, _dp(arenas), arenas.shape[1])
        return self

    def get_factor_adjoint_batch(self, member, out=None):
        """one member's adjoint arena on the host: Lbar_b as seeded, or after factor_adjoint_batch() d loss /
        d (P A_b P^T) on the stored lower positions"""
        arena = self.sym_info()["arena"]
        if out is None:
            out = np.zeros(max(arena, 1), dtype=np.float64)
        assert out.dtype == np.float64 and out.size >= arena and out.flags["C_CONTIGUOUS"]
        self._call("spllt_hip_get_factor_adjoint_batch", self.fkeep, int(member), _dp(out), arena)
        return out[:arena]

    def device_factor_adjoint_batch_ptr(self):
        """(device pointer of member 0's adjoint arena, member stride in doubles); (None, 0) while unseeded"""
        stride = C.c_int64()
        p = self.lib.spllt_hip_device_factor_adjoint_batch(self.fkeep, C.byref(stride))
        return p, stride.value

    def factor_adjoint_batch(self):
        """spllt_hip_factor_adjoint_batch: the sweep over the seeded arenas; returns d loss / d val_b, shape
        (nbatch, nnz); the row of a member that is not positive definite is NaN"""
        nb = self._batch_count()
        out = np.zeros((max(nb, 1), max(self.nnz, 1)), dtype=np.float64)
        self._call("spllt_hip_factor_adjoint_batch", self.fkeep, _dp(out), out.shape[1], ok=self._BATCH_OK)
        return out[:nb, :self.nnz]

    def factor_adjoint_batch_dev(self, gval_dev_ptr, ldout=None):
        """spllt_hip_factor_adjoint_batch_dev: the same sweep, gval[b*ldout + k] into device memory.  Returns 0
        or -20."""
        return self._call("spllt_hip_factor_adjoint_batch_dev", self.fkeep, C.c_void_p(gval_dev_ptr),
                          int(self.nnz if ldout is None else ldout), ok=self._BATCH_OK)

    def batch_adjoint_launches(self):
        """kernel launches of the last sweep of the batch's factor adjoint, the reader included"""
        return int(self.lib.spllt_hip_batch_adjoint_launches(self.fkeep))

    def release_factor_adjoint_batch(self):
        self._call("spllt_hip_release_factor_adjoint_batch", self.fkeep)
        return self

    # ---- multi-GPU subtree partition ------------------------------------------
    def set_partition(self, rank, nranks):
        """Declare this process as `rank` of `nranks`; returns the number of
        doubles of the top-tree exchange buffer (0 for nranks == 1)."""
        n = C.c_int64()
        rc = self.lib.spllt_hip_set_partition(self.fkeep, rank, nranks, C.byref(n))
        if rc < 0:
            raise SplltError("spllt_hip_set_partition", rc)
        self.rank, self.nranks = rank, nranks
        return n.value

    def set_communicator(self, nccl_comm):
        """hand the caller's RCCL communicator (ncclComm_t as an integer) to the library: the
        exchanges of the partition then run inside spllt_factor / spllt_wait / spllt_solve"""
        self._call("spllt_hip_set_communicator", self.fkeep, C.c_void_p(nccl_comm))

    def set_exchange_buffer(self, dev_ptr):
        rc = self.lib.spllt_hip_set_exchange_buffer(self.fkeep, C.c_void_p(dev_ptr))
        if rc < 0:
            raise SplltError("spllt_hip_set_exchange_buffer", rc)

    def engine_stream(self):
        """hipStream_t (integer) on which the exchange buffer is packed / unpacked"""
        p = self.lib.spllt_hip_engine_stream(self.fkeep)
        if not p:
            raise SplltError("spllt_hip_engine_stream", -30, self.last_error())
        return int(p)

    def exchange_stream(self):
        """hipStream_t (integer) of the pending exchange: its collective belongs on this stream"""
        return int(self.lib.spllt_hip_exchange_stream(self.fkeep) or 0)

    def continue_after_exchange(self):
        self._call("spllt_hip_continue", self.fkeep)
        return self

    def pending_exchange(self):
        """index of the exchange (program("exchanges")) the engine is waiting for, -1: none"""
        return int(self.lib.spllt_hip_pending_exchange(self.fkeep))

    def partition(self, name):
        nbytes = self.lib.spllt_hip_partition_get(self.fkeep, name.encode(), None, 0)
        if nbytes < 0:
            raise KeyError(name)
        raw = np.zeros(max(nbytes, 1), dtype=np.uint8)
        self.lib.spllt_hip_partition_get(self.fkeep, name.encode(), raw.ctypes.data, nbytes)
        raw = raw[:nbytes]
        if name == "arena_elems":
            return raw.view(np.int64)
        return raw if name == "map_keep" else raw.view(np.int32)

    def profile(self, val, in_program=False):
        """per-launch device time (ms) of one factorization: launches serialized on one
        stream (kernels alone on the chip), or in_program=True: inside the real
        multi-stream program (durations under contention)"""
        val = np.ascontiguousarray(val, dtype=np.float64)
        nl = len(self.program("launches"))
        ms = np.zeros(max(nl, 1), dtype=np.float32)
        rc = self._call("spllt_hip_profile_in_program" if in_program else "spllt_hip_profile", self.fkeep, _dp(val),
                        self.nnz, ms.ctypes.data_as(C.POINTER(C.c_float)), nl, where="spllt_hip_profile")
        return ms[:rc]

    def timeline(self, val):
        """spllt_hip_timeline: ms after the value scatter at which the event of every recording
        launch of the real multi-stream program completed (-1: none); last entry = the end"""
        val = np.ascontiguousarray(val, dtype=np.float64)
        nl = len(self.program("launches")) + 1
        t = np.zeros(nl, dtype=np.float32)
        rc = self._call("spllt_hip_timeline", self.fkeep, _dp(val), self.nnz, t.ctypes.data_as(C.POINTER(C.c_float)), nl)
        return t[:rc]

    def _call(self, name, *args, ok=(), where=None):
        """lib.<name>(*args); a negative return value that is not in `ok` raises with the handle's message"""
        rc = getattr(self.lib, name)(*args)
        if rc < 0 and rc not in ok:
            raise SplltError(where or name, rc, self.last_error())
        return rc

    def last_error(self):
        return (self.lib.spllt_hip_last_error(self.fkeep) or b"").decode()

    def close(self):
        if getattr(self, "lib", None) is None:
            return
        st = C.c_int()
        if self.fkeep:
            self.lib.spllt_deallocate_fkeep(C.byref(self.fkeep), C.byref(st))
        if self.akeep:
            self.lib.spllt_deallocate_akeep(C.byref(self.akeep), C.byref(st))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def residual(n, ptr, row, val, x, b):
    """||A x - b||_2 / ||b||_2 for the symmetric matrix given by its 1-based
    CSC lower triangle (the metric of reference drivers/spllt_omp.F90:248-262)."""
    import scipy.sparse as sp
    L = sp.csc_matrix((val, np.asarray(row) - 1, np.asarray(ptr) - 1), shape=(n, n))
    A = L + sp.tril(L, -1).T
    r = A @ x - b
    return float(np.linalg.norm(r) / np.linalg.norm(b))
