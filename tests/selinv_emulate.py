"""Numpy interpreter of the selected-inversion program exported by
spllt_hip_program_get ("selinv_*").  TEST-ONLY, like tests/emulate.py: it runs the
same work tables the HIP kernels consume (units, tiles, launches, row descriptors,
row maps, scratch offsets) with dense numpy arithmetic, so that the program can be
validated on a machine without a GPU."""
import numpy as np

SI_SYMM, SI_SCALE, SI_DIAG = 0, 1, 2
TILE = 64


def selinv_tables(f):
    return {k: f.program("selinv_" + k) for k in ("units", "tiles", "launches", "rows", "relpos", "diag",
                                                   "scratch")}


def z_index(t, u, ri, rk):
    """arena offsets of Z(ri, rk) for node-local rows ri, rk (broadcast arrays) of unit u's node:
    the lower half through row k's descriptor, the upper half transposed"""
    rows, relpos = t["rows"], t["relpos"]
    ri, rk = np.broadcast_arrays(np.asarray(ri), np.asarray(rk))
    lo = ri >= rk
    i = np.where(lo, ri, rk)
    k = np.where(lo, rk, ri)
    d = rows[int(u["row_off"]) + k]
    own = d["map"] < 0
    q = i.astype(np.int64).copy()
    if (~own).any():
        q[~own] = relpos[d["map"][~own].astype(np.int64) + i[~own] - k[~own]]
    return d["cbase"] + q * d["ld"]


def dinv_block(dinv, u):
    pn, ld, o = int(u["pn"]), int(u["dinv_ld"]), int(u["dinv_off"])
    D = dinv[o + np.arange(pn)[:, None] * ld + np.arange(pn)[None, :]]
    return np.tril(D)                      # (what lies above the diagonal is never read)


def l_rows(L, u, r0, r1):
    """rows [r0, r1) of R (0 = first row below the panel) x the panel's columns"""
    ld, c0, pn = int(u["ld"]), int(u["c0"]), int(u["pn"])
    rr = c0 + pn + np.arange(r0, r1)
    return L[int(u["off"]) + rr[:, None] * ld + c0 + np.arange(pn)[None, :]]


def z_rows_index(u, r0, r1):
    ld, c0, pn = int(u["ld"]), int(u["c0"]), int(u["pn"])
    rr = c0 + pn + np.arange(r0, r1)
    return int(u["off"]) + rr[:, None] * ld + c0 + np.arange(pn)[None, :]


def z_diag_index(u):
    ld, c0, pn = int(u["ld"]), int(u["c0"]), int(u["pn"])
    a, b = np.tril_indices(pn)
    return int(u["off"]) + (c0 + a) * ld + c0 + b, a, b


def emulate_selinv(f, L, dinv, t=None):
    """Z arena from the factor arena L and the dinv scratch.  Entries the program never writes stay
    NaN (the strict upper triangle of diagonal tiles), and so does anything computed from them."""
    t = t or selinv_tables(f)
    units, tiles = t["units"], t["tiles"]
    Z = np.full(L.shape, np.nan)
    scratch = np.full(max(1, t["scratch"]), np.nan)
    for kind, level, first, count, _ in t["launches"]:
        if kind == SI_SYMM:
            for ui, ti, ks in tiles[first:first + count]:
                u, ti, ks = units[ui], int(ti), int(ks)          # (int16 fields: no overflow below)
                nR, rb, kl, pn = int(u["nR"]), int(u["rbase"]), int(u["kslice"]), int(u["pn"])
                i0, i1 = ti * TILE, min(nR, ti * TILE + TILE)
                k0, k1 = ks * kl, min(nR, ks * kl + kl)
                assert 0 <= i0 < i1 and 0 <= k0 < k1 and ks < u["nsplit"]
                idx = z_index(t, u, rb + np.arange(i0, i1)[:, None], rb + np.arange(k0, k1)[None, :])
                Y = Z[idx] @ l_rows(L, u, k0, k1)
                so = int(u["y_off"]) + (ks * nR + np.arange(i0, i1))[:, None] * pn + np.arange(pn)[None, :]
                assert so.min() >= int(u["y_off"]) and so.max() < int(u["p_off"])
                scratch[so] = Y
        elif kind == SI_SCALE:
            for ui, ti, _ in tiles[first:first + count]:
                u, ti = units[ui], int(ti)
                nR, pn = int(u["nR"]), int(u["pn"])
                i0, i1 = ti * TILE, min(nR, ti * TILE + TILE)
                Y = np.zeros((i1 - i0, pn))
                for ks in range(int(u["nsplit"])):      # the slices in order
                    Y += scratch[int(u["y_off"]) + (ks * nR + np.arange(i0, i1))[:, None] * pn + np.arange(pn)[None, :]]
                Zrj = -Y @ dinv_block(dinv, u)
                Z[z_rows_index(u, i0, i1)] = Zrj
                po = int(u["p_off"]) + ti * pn * pn
                scratch[po:po + pn * pn] = (l_rows(L, u, i0, i1).T @ Zrj).ravel()
        elif kind == SI_DIAG:
            for u in units[first:first + count]:
                pn = int(u["pn"])
                D = dinv_block(dinv, u)
                T = D.copy()
                for ti in range(int(u["ntile"])):        # the tiles in order
                    po = int(u["p_off"]) + ti * pn * pn
                    T -= scratch[po:po + pn * pn].reshape(pn, pn)
                idx, a, b = z_diag_index(u)
                Z[idx] = (D.T @ T)[a, b]
        else:
            raise AssertionError(f"unknown selinv launch kind {kind}")
    return Z


def panel_inverses(f, L, t=None):
    """a dinv scratch with inv(L_JJ) of every panel at its unit's slot (numpy inverses)"""
    t = t or selinv_tables(f)
    units = t["units"]
    size = int(max((u["dinv_off"] + u["pn"] * u["dinv_ld"] for u in units), default=1))
    dinv = np.zeros(size)
    for u in units:
        pn, ld, c0 = int(u["pn"]), int(u["ld"]), int(u["c0"])
        blk = np.tril(L[int(u["off"]) + (c0 + np.arange(pn))[:, None] * ld + c0 + np.arange(pn)[None, :]])
        o, dl = int(u["dinv_off"]), int(u["dinv_ld"])
        dinv[o + np.arange(pn)[:, None] * dl + np.arange(pn)[None, :]] = np.linalg.inv(blk)
    return dinv


def launch_access(f, t=None):
    """per launch: (Z arena offsets it writes, Z arena offsets it gathers)"""
    t = t or selinv_tables(f)
    units, tiles = t["units"], t["tiles"]
    out = []
    for kind, level, first, count, _ in t["launches"]:
        w, r = [], []
        if kind == SI_SYMM:
            for ui in np.unique(tiles[first:first + count]["unit"]):
                u = units[ui]
                rr = int(u["rbase"]) + np.arange(int(u["nR"]))
                r.append(z_index(t, u, rr[:, None], rr[None, :]).ravel())
        elif kind == SI_SCALE:
            for ui in np.unique(tiles[first:first + count]["unit"]):
                w.append(z_rows_index(units[ui], 0, int(units[ui]["nR"])).ravel())
        else:
            for u in units[first:first + count]:
                w.append(z_diag_index(u)[0])
        cat = lambda v: np.concatenate(v) if v else np.zeros(0, dtype=np.int64)  # noqa: E731
        out.append((cat(w), cat(r)))
    return out


def check_order(access, arena):
    """every entry a launch gathers was written by an EARLIER launch; returns the violations"""
    writer = np.full(arena, -1, dtype=np.int64)
    bad = []
    for k, (w, r) in enumerate(access):
        if r.size and (writer[r] < 0).any():
            bad.append(k)
        writer[w] = k
    return bad


def expected_z(f, A):
    """inv(P A P^T) on L's arena positions (dense reference)"""
    import scipy.sparse as sp
    from helpers import sym_tables
    tb = sym_tables(f)
    n = f.n
    P = np.empty(n, dtype=np.int64)
    P[tb["order"]] = np.arange(n)
    Zd = np.linalg.inv(sp.csc_matrix(A).toarray()[np.ix_(P, P)])
    out = np.zeros(f.sym_info()["arena"])
    for b in range(len(tb["bcol_off"])):
        s = int(tb["bcol_node"][b])
        rows = tb["rlist"][tb["rptr"][s]:tb["rptr"][s + 1]]
        w, nr, off, r0 = (int(tb["bcol_width"][b]), int(tb["bcol_nrow"][b]), int(tb["bcol_off"][b]),
                          int(tb["bcol_r0"][b]))
        c0 = int(tb["sptr"][s]) + r0
        out[off:off + nr * w] = Zd[np.ix_(rows[r0:r0 + nr], np.arange(c0, c0 + w))].ravel()
    return out
