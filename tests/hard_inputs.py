"""Ill-conditioned, graded and scaled SPD inputs, a high-precision reference and backward-error metrics
(TEST-ONLY, CPU only, never timed).

The forward criterion of the suite (max |L - L_oracle| / max |L| <= 1e-12) means nothing once cond(A) u
approaches it: two backward-stable factors already differ by that much.  What is compared here are backward
errors, evaluated in np.longdouble (64-bit significand) so that the evaluation itself is exact to ~1e-19:

  eta(Ap, L)      = ||Ap - L L^T||_F / ||Ap||_F            Ap = P A P^T, pivot order
  omega(A, x, b)  = ||b - A x||_2 / (||b||_2 + max|a_ij| ||x||_2)      (helpers.bwd_err, the reference's formula)
  inv_resid(L, W) = ||W L - I||_F / (||W||_F ||L||_F)

and the bars are ratios to the same metric of a CPU computation of the same algorithm (tests/emulate.py for
the factor, model_solve here for the substitution) and of the oracle, never constants."""
import numpy as np
import pytest
import scipy.linalg as sl
import scipy.sparse as sp

from helpers import make_case, oracle_factor, sym_tables
from spllt_amd import matgen

LD = np.longdouble
if not np.finfo(LD).eps < 1e-18:
    pytest.skip("np.longdouble is no wider than double here: no high-precision reference", allow_module_level=True)

U = 2.0 ** -53            # unit roundoff of fp64


# ---- generators (each returns a scipy CSC matrix) ------------------------------------------------------------
def hilbert_shift(n, s):
    i = np.arange(n)
    return sp.csc_matrix(1.0 / (i[:, None] + i[None, :] + 1.0) + s * np.eye(n))


def randsvd(n, kappa, seed):
    """Q diag(sigma) Q^T, sigma_i geometric from 1 down to 1 / kappa, Q the orthogonal factor of a Gaussian"""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    sig = kappa ** (-np.arange(n) / (n - 1.0))
    A = (Q * sig) @ Q.T
    return sp.csc_matrix(0.5 * (A + A.T))


def biharmonic1d(n):
    T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(n, n)).tocsc()
    return sp.csc_matrix(T @ T)


def biharmonic2d(g):
    P = sp.csc_matrix(matgen.poisson2d(g))
    return sp.csc_matrix(P @ P)


def graded(A, e):
    """D A D with D = diag(2.0 ** e), e an integer array: exact scaling of the stored values"""
    A = sp.csc_matrix(A, copy=True)
    A.sort_indices()
    e = np.asarray(e, dtype=np.int64)
    col = np.repeat(np.arange(A.shape[1]), np.diff(A.indptr))
    A.data = np.ldexp(A.data, (e[A.indices] + e[col]).astype(np.int32))
    return A


def scaled(A, k):
    """A 2**k, exactly"""
    A = sp.csc_matrix(A, copy=True)
    A.sort_indices()
    A.data = np.ldexp(A.data, int(k))
    return A


def grading_exponents(n, seed, lo=-100, hi=100):
    return np.random.default_rng(seed).integers(lo, hi + 1, n)


# ---- the cases of tests/test_conditioning_{cpu,gpu}.py --------------------------------------------------------
# (id, matrix, options, class); "hard": cond(A) ~ 2e10 with kappa(L_pp) ~ 1e5, where the inverse-multiply
# algorithm itself crosses the reference's 1e-14 bar
CASES = [
    ("h192-s2", lambda: hilbert_shift(192, 1e-2), dict(nb=64, nemin=4), "benign"),
    ("h192-s6", lambda: hilbert_shift(192, 1e-6), dict(nb=64, nemin=4), "benign"),
    ("h192-s10", lambda: hilbert_shift(192, 1e-10), dict(nb=64, nemin=4), "hard"),
    ("h200-s10-pw48", lambda: hilbert_shift(200, 1e-10), dict(nb=100, nemin=4, panel_width=48), "hard"),
    ("h260-s10-nb256", lambda: hilbert_shift(260, 1e-10), dict(nb=256, nemin=4), "hard"),
    ("rsvd200-k6", lambda: randsvd(200, 1e6, 6), dict(nb=64, nemin=4), "benign"),
    ("rsvd200-k10", lambda: randsvd(200, 1e10, 10), dict(nb=64, nemin=4), "benign"),
    ("rsvd200-k12", lambda: randsvd(200, 1e12, 12), dict(nb=64, nemin=4), "benign"),
    ("bih1d-320-nb64", lambda: biharmonic1d(320), dict(nb=64, nemin=16), "benign"),
    ("bih1d-320-nb16-pw8", lambda: biharmonic1d(320), dict(nb=16, nemin=4, panel_width=8), "benign"),
    ("bih2d-20-nb64", lambda: biharmonic2d(20), dict(nb=64, nemin=16), "benign"),
    ("bih2d-20-nb100-pw40", lambda: biharmonic2d(20), dict(nb=100, nemin=8, panel_width=40), "benign"),
]
CASE_IDS = [c[0] for c in CASES]
SPARSE = {c[0] for c in CASES if c[0].startswith("bih")}

EQUI_BASES = [("nd887", lambda: matgen.nd_like((8, 8, 7), 2)), ("fe27-544", lambda: matgen.fe27((5, 4, 4), 3))]
EQUI_OPTS = [dict(nb=48, nemin=8, panel_width=24), dict(nb=160, nemin=8, panel_width=32)]
EQUI_KINDS = ["graded", "scaled+600", "scaled-600"]


def equi_scaling(kind, n, seed):
    """exponents e with D = diag(2**e) such that the scaled matrix is D A D (scaled(A, 2k) = graded(A, k 1))"""
    if kind == "graded":
        return grading_exponents(n, seed)
    return np.full(n, 300 if kind == "scaled+600" else -300, dtype=np.int64)


# ---- pivot order, dense factors ---------------------------------------------------------------------------------
def pivot_perm(f):
    """P with P[position] = variable"""
    P = np.empty(f.n, dtype=np.int64)
    P[f.sym("order")] = np.arange(f.n)
    return P


def permuted(f, A):
    """P A P^T as a dense longdouble matrix"""
    P = pivot_perm(f)
    return sp.csc_matrix(A).toarray()[np.ix_(P, P)].astype(LD)


def dense_L(f, arena):
    """the arena as a dense lower triangle in pivot order (the inverse of helpers.dense_arena)"""
    t = sym_tables(f)
    L = np.zeros((f.n, f.n), dtype=np.asarray(arena).dtype)
    for b in range(len(t["bcol_off"])):
        s = int(t["bcol_node"][b])
        rows = t["rlist"][t["rptr"][s]:t["rptr"][s + 1]]
        w, nr, off, r0 = (int(t["bcol_width"][b]), int(t["bcol_nrow"][b]), int(t["bcol_off"][b]), int(t["bcol_r0"][b]))
        c0 = int(t["sptr"][s]) + r0
        L[np.ix_(rows[r0:r0 + nr], np.arange(c0, c0 + w))] = np.asarray(arena[off:off + nr * w]).reshape(nr, w)
    return np.tril(L)


def chol_ld(Ap):
    """column Cholesky in longdouble; returns None where a pivot is not positive"""
    Ap = np.asarray(Ap, dtype=LD)
    n = Ap.shape[0]
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        c = Ap[j:, j] - L[j:, :j] @ L[j, :j]
        if not c[0] > 0:
            return None
        L[j:, j] = c / np.sqrt(c[0])
    return L


# ---- metrics, all in longdouble ----------------------------------------------------------------------------------
def _fro(M):
    return np.sqrt(np.sum(np.asarray(M, dtype=LD) ** 2))


def eta(Ap, L):
    L = np.asarray(L, dtype=LD)
    Ap = np.asarray(Ap, dtype=LD)
    return float(_fro(Ap - L @ L.T) / _fro(Ap))


def omega(A, x, b):
    """per column for matrices; A dense or sparse"""
    Ad = np.asarray(A.toarray() if sp.issparse(A) else A, dtype=LD)
    x, b = np.asarray(x, dtype=LD), np.asarray(b, dtype=LD)
    r = b - Ad @ x
    amax = np.abs(Ad).max()
    nrm = lambda v: np.sqrt(np.sum(v * v, axis=0))   # noqa: E731
    out = nrm(r) / (nrm(b) + amax * nrm(x))
    return float(out) if out.ndim == 0 else out.astype(np.float64)


def inv_resid(L, W):
    L, W = np.asarray(L, dtype=LD), np.asarray(W, dtype=LD)
    return float(_fro(W @ L - np.eye(L.shape[0], dtype=LD)) / (_fro(W) * _fro(L)))


# ---- the panels the program really uses ---------------------------------------------------------------------------
def panels(f, pw):
    """(first column, width) of every diagonal panel in pivot order: block columns from f.sym, cut every pw"""
    t = sym_tables(f)
    out = []
    for b in range(len(t["bcol_off"])):
        c0 = int(t["sptr"][int(t["bcol_node"][b])]) + int(t["bcol_r0"][b])
        w = int(t["bcol_width"][b])
        out += [(c0 + p0, min(pw, w - p0)) for p0 in range(0, w, pw)]
    return sorted(out)


def panel_kappa(f, L, pw):
    L = np.asarray(L, dtype=np.float64)
    return max(float(np.linalg.cond(L[c:c + w, c:c + w])) for c, w in panels(f, pw))


def model_solve(f, L, B, pw):
    """forward and backward substitution with a dense factor in pivot order, applying inv(L_pp) panel by panel
    as the engine's solve kernels do (B: n or n x nrhs, pivot order); fp64"""
    L = np.asarray(L, dtype=np.float64)
    y = np.array(B, dtype=np.float64, copy=True)
    pl = panels(f, pw)
    inv = [sl.solve_triangular(L[c:c + w, c:c + w], np.eye(w), lower=True) for c, w in pl]
    for (c, w), W in zip(pl, inv):
        y[c:c + w] = W @ y[c:c + w]
        y[c + w:] -= L[c + w:, c:c + w] @ y[c:c + w]
    for (c, w), W in zip(pl[::-1], inv[::-1]):
        y[c:c + w] -= L[c + w:, c:c + w].T @ y[c + w:]
        y[c:c + w] = W.T @ y[c:c + w]
    return y


def panel_chol16(S):
    """the 64-panel POTRF as the kernels block it (kernels.hip potrf64_body; a hook for
    emulate.emulate_program(panel_chol=)): 16 x 16 blocks, left-looking,
      A1  T_IJ -= sum_{K<J} T_IK T_JK^T          I >= J
      A2  D_J = chol(T_JJ), inv(D_J)
      A3  T_IJ = T_IJ inv(D_J)^T                 I > J      (a product, not a substitution)
      B   X_JJ = inv(D_J);  X_IJ = -inv(D_I) sum_{K=J}^{I-1} T_IK X_KJ      (the panel's inverse)
    in LAPACK arithmetic per block.  Returns (L, inv(L))."""
    n = len(S)
    T = np.tril(np.asarray(S, dtype=np.float64))
    X = np.zeros((n, n))
    blocks = [(j0, min(j0 + 16, n)) for j0 in range(0, n, 16)]
    DI = []
    for j0, j1 in blocks:
        T[j0:, j0:j1] -= T[j0:, :j0] @ T[j0:j1, :j0].T
        d = np.tril(T[j0:j1, j0:j1])
        D = sl.cholesky(d + np.tril(d, -1).T, lower=True)
        W = sl.solve_triangular(D, np.eye(j1 - j0), lower=True)
        T[j0:j1, j0:j1] = D
        T[j1:, j0:j1] = T[j1:, j0:j1] @ W.T
        X[j0:j1, j0:j1] = W
        DI.append(W)
    for d in range(1, len(blocks)):
        for J in range(len(blocks) - d):
            i0, i1 = blocks[J + d]
            j0, j1 = blocks[J]
            X[i0:i1, j0:j1] = -DI[J + d] @ (T[i0:i1, j0:i0] @ X[j0:i0, j0:j1])
    return np.tril(T), X


def to_pivot(f, b):
    out = np.empty_like(np.asarray(b, dtype=np.float64))
    out[f.sym("order")] = b
    return out


def from_pivot(f, y):
    return np.asarray(y)[f.sym("order")]


# ---- references of one case, computed once ------------------------------------------------------------------------
_cache = {}


def rhs(A, nrhs=33, seed=7):
    x0 = np.random.default_rng(seed).standard_normal((A.shape[0], nrhs))
    return np.asarray(A @ x0)


def case_inputs(cid):
    """A, b (33 columns) and the dense longdouble references that depend on the matrix alone"""
    key = ("A", cid)
    if key not in _cache:
        gen = next(c[1] for c in CASES if c[0] == cid)
        A = gen()
        _cache[key] = dict(A=A, b=rhs(A))
    return _cache[key]


def oracle_references(f, A, val, b, key=None):
    """what depends on the matrix and the symbolic factorization alone (not on the engine's program): Ap,
    the longdouble factor's and the oracle's eta, the oracle's factor and the omega of its solve"""
    if key is not None and ("oracle", key) in _cache:
        return _cache[("oracle", key)]
    Ap = permuted(f, A)
    r = dict(Ap=Ap)
    Lld = chol_ld(Ap)
    assert Lld is not None, "the longdouble Cholesky met a non-positive pivot"
    r["eta_ld"] = eta(Ap, Lld)
    o, rc = oracle_factor(f, val)
    r["rc_oracle"] = rc
    r["L_oracle"] = dense_L(f, o.arena())
    r["eta_oracle"] = eta(Ap, r["L_oracle"])
    r["omega_oracle"] = np.atleast_1d(omega(A, o.solve(b), b))
    if key is not None:
        _cache[("oracle", key)] = r
    return r


def references(f, A, val, b, pw, key=None, prog=None):
    """the CPU side of one (matrix, program): oracle and emulated program, factor and solve.  Returns a dict
    with Ap, eta_ld, eta_oracle, eta_emul, L_oracle, L_emul, kappa, omega_oracle, omega_model (per column of b).
    key: the matrix and its options (the oracle's part is computed once per key); prog: what the interpreter
    reads the program from, where that is not f itself (batch_emulate.BatchProgramView)"""
    from emulate import emulate_program
    r = dict(oracle_references(f, A, val, b, key))
    Ap = r["Ap"]
    # (chain blocks as the kernels compute them: the interpreter's default, one dpotrf of the block and a true
    # substitution of the rows below, is a different and backward-stable algorithm)
    prog = f if prog is None else prog
    r["L_emul"] = dense_L(f, emulate_program(prog, val, chain_inverse_multiply=True))
    r["eta_emul"] = eta(Ap, r["L_emul"])
    r["eta_emul16"] = eta(Ap, dense_L(f, emulate_program(prog, val, panel_chol=panel_chol16, chain_inverse_multiply=True)))
    r["kappa"] = panel_kappa(f, r["L_emul"], pw)
    xm = from_pivot(f, model_solve(f, r["L_emul"], to_pivot(f, b), pw))
    r["omega_model"] = np.atleast_1d(omega(A, xm, b))
    r["fwd_emul"] = float(np.abs(r["L_emul"] - r["L_oracle"]).max() / np.abs(r["L_oracle"]).max())
    return r


def make(cid, **extra):
    """(A, b, f, val, pw, class) of a case of CASES; extra: engine_flags etc. for helpers.make_case"""
    _, _, opts, cls = next(c for c in CASES if c[0] == cid)
    ci = case_inputs(cid)
    f, val = make_case(ci["A"], **opts, **extra)
    return ci["A"], ci["b"], f, val, int(f.program("panel_width")), cls
