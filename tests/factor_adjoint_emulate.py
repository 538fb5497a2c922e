"""Numpy interpreter of the factor-adjoint sweep (spllt_hip_factor_adjoint) and its dense references.
TEST-ONLY, like tests/selinv_emulate.py: the sweep runs the selected-inversion program exported by
spllt_hip_program_get ("selinv_*": units, tiles, launches, row descriptors, row maps, scratch offsets) with
the arithmetic of factor_adjoint.hip in dense numpy, so that it can be validated without a GPU.

G: an arena with L's layout.  On entry Lbar = d loss / d L on the lower positions; on exit
d loss / d (P A P^T)_ij on every stored lower position, a stored lower entry standing for a_ij and a_ji."""
import numpy as np
import scipy.linalg as sl
import scipy.sparse as sp

from helpers import lower_mask, sym_tables
from selinv_emulate import (SI_DIAG, SI_SCALE, SI_SYMM, TILE, dinv_block, l_rows, selinv_tables, z_diag_index,
                            z_index, z_rows_index)


def phi(X):
    """lower triangle with the diagonal halved"""
    return np.tril(X, -1) + 0.5 * np.diag(np.diag(X))


def emulate_factor_adjoint(f, L, dinv, Lbar, t=None, trace=None):
    """The swept arena.  What is not a lower position of L starts as NaN (it must never be read).
    trace: a list that receives per launch (offsets written, offsets gathered from G_RR, own offsets read)."""
    t = t or selinv_tables(f)
    units, tiles = t["units"], t["tiles"]
    G = np.where(lower_mask(f), Lbar, np.nan)
    scratch = np.full(max(1, t["scratch"]), np.nan)
    for kind, level, first, count, _ in t["launches"]:
        w, r, own = [], [], []
        if kind == SI_SYMM:
            for ui, ti, ks in tiles[first:first + count]:
                u, ti, ks = units[ui], int(ti), int(ks)
                nR, rb, kl, pn = int(u["nR"]), int(u["rbase"]), int(u["kslice"]), int(u["pn"])
                i0, i1 = ti * TILE, min(nR, ti * TILE + TILE)
                k0, k1 = ks * kl, min(nR, ks * kl + kl)
                ri, rk = rb + np.arange(i0, i1)[:, None], rb + np.arange(k0, k1)[None, :]
                idx = z_index(t, u, ri, rk)
                S = G[idx] * np.where(ri == rk, 2.0, 1.0)           # tril + tril^T: the diagonal counts twice
                so = int(u["y_off"]) + (ks * nR + np.arange(i0, i1))[:, None] * pn + np.arange(pn)[None, :]
                scratch[so] = S @ l_rows(L, u, k0, k1)
                r.append(idx.ravel())
        elif kind == SI_SCALE:
            for ui, ti, _ in tiles[first:first + count]:
                u, ti = units[ui], int(ti)
                nR, pn = int(u["nR"]), int(u["pn"])
                i0, i1 = ti * TILE, min(nR, ti * TILE + TILE)
                Y = np.zeros((i1 - i0, pn))
                for ks in range(int(u["nsplit"])):                  # the slices in order
                    Y += scratch[int(u["y_off"]) + (ks * nR + np.arange(i0, i1))[:, None] * pn + np.arange(pn)[None, :]]
                idx = z_rows_index(u, i0, i1)
                own.append(idx.ravel())
                W = (G[idx] - Y) @ dinv_block(dinv, u)
                G[idx] = W
                w.append(idx.ravel())
                po = int(u["p_off"]) + ti * pn * pn
                scratch[po:po + pn * pn] = (W.T @ l_rows(L, u, i0, i1)).ravel()
        elif kind == SI_DIAG:
            for u in units[first:first + count]:
                pn = int(u["pn"])
                D = dinv_block(dinv, u)
                Q = np.zeros((pn, pn))
                for ti in range(int(u["ntile"])):                   # the tiles in order
                    po = int(u["p_off"]) + ti * pn * pn
                    Q += scratch[po:po + pn * pn].reshape(pn, pn)
                idx, a, b = z_diag_index(u)
                own.append(idx)
                M = np.zeros((pn, pn))
                M[a, b] = G[idx] - Q[a, b]
                Ljj = np.zeros((pn, pn))
                Ljj[a, b] = L[idx]
                P = phi(Ljj.T @ M)
                N = D.T @ (P + P.T) @ D
                G[idx] = phi(N)[a, b]
                w.append(idx)
        else:
            raise AssertionError(f"unknown selinv launch kind {kind}")
        if trace is not None:
            cat = lambda v: np.concatenate(v) if v else np.zeros(0, dtype=np.int64)  # noqa: E731
            trace.append((cat(w), cat(r), cat(own)))
    return G


# ---- between dense pivot-order matrices and the arena ------------------------------------------------
def _blocks(f):
    tb = sym_tables(f)
    for b in range(len(tb["bcol_off"])):
        s = int(tb["bcol_node"][b])
        rows = tb["rlist"][tb["rptr"][s]:tb["rptr"][s + 1]]
        w, nr, off, r0 = (int(tb["bcol_width"][b]), int(tb["bcol_nrow"][b]), int(tb["bcol_off"][b]),
                          int(tb["bcol_r0"][b]))
        c0 = int(tb["sptr"][s]) + r0
        yield off, nr, w, rows[r0:r0 + nr], np.arange(c0, c0 + w)


def arena_from_dense(f, M):
    """M (n x n, pivot order) at L's arena positions"""
    out = np.zeros(f.sym_info()["arena"])
    for off, nr, w, rows, cols in _blocks(f):
        out[off:off + nr * w] = M[np.ix_(rows, cols)].ravel()
    return out


def dense_from_arena(f, arena):
    """the lower positions of an arena as a dense lower-triangular matrix in pivot order"""
    M = np.zeros((f.n, f.n))
    for off, nr, w, rows, cols in _blocks(f):
        M[np.ix_(rows, cols)] = arena[off:off + nr * w].reshape(nr, w)
    return np.tril(M)


def pivot_matrix(f, A):
    """P A P^T, dense"""
    P = np.empty(f.n, dtype=np.int64)
    P[f.sym("order")] = np.arange(f.n)
    return sp.csc_matrix(A).toarray()[np.ix_(P, P)]


def dense_factor_adjoint(f, Ld, Lbar):
    """the dense formula Phi(L^-T (P + P^T) L^-1), P = Phi(L^T Lbar), on L's arena positions.  Ld: the dense
    Cholesky factor of P A P^T, Lbar: an arena"""
    P = phi(Ld.T @ dense_from_arena(f, Lbar))
    X = sl.solve_triangular(Ld, P + P.T, lower=True, trans="T")           # L^-T S
    N = sl.solve_triangular(Ld, X.T, lower=True, trans="T").T             # ... L^-1
    return arena_from_dense(f, phi(N))


def outer_seed(f, a, b, alpha=1.0):
    """alpha sum_q a_q b_q^T (pivot-order vectors, n or n x nvec) at L's arena positions"""
    a, b = np.reshape(a, (f.n, -1)), np.reshape(b, (f.n, -1))
    return arena_from_dense(f, alpha * (a @ b.T))


def logdet_seed(f, L):
    """diag(2 / L_jj): the seed of log det A"""
    out = np.zeros(f.sym_info()["arena"])
    d = f.program("selinv_diag")
    out[d] = 2.0 / L[d]
    return out


def on_pattern(f, G):
    """the arena values at the entries of A, in the order of val (host lookup, user indices)"""
    prow, pcol = f.pattern_tables()
    return f.inverse_entries(prow, pcol, Z=G)


def rel(a, b, mask):
    return float(np.abs(a[mask] - b[mask]).max() / np.abs(b[mask]).max())


def _cases():
    from spllt_amd import matgen
    return [
        ("p2d12-nb4", lambda: matgen.poisson2d(12), 4, 4, None),
        ("p2d16-nb8-pw32", lambda: matgen.poisson2d(16), 8, 4, 32),
        ("p2d32-nb16", lambda: matgen.poisson2d(32), 16, 32, None),
        ("p2d64-nb100-pw32", lambda: matgen.poisson2d(64), 100, 32, 32),
        ("p3d10-nb48", lambda: matgen.poisson3d(10), 48, 16, None),
        ("box8-nb96", lambda: matgen.nd_like((8, 8, 8), 2), 96, 16, None),
        ("box12-nb256", lambda: matgen.nd_like((12, 12, 11), 3), 256, 32, None),     # units with several K slices
        ("fe27-nb64", lambda: matgen.fe27((5, 5, 4), 3), 64, 16, None),
        ("box11-nb100-pw48", lambda: matgen.nd_like((11, 10, 10), 3), 100, 16, 48),   # ragged panels
    ]


# the cases of tests/test_selinv_gpu.py up to n = 4096: (name, matrix, nb, nemin, panel width)
CASES = _cases()
KSLICE_CASE = "box12-nb256"
