"""Dense numpy statement of the hard linear constraints C x = e (include/spllt_hip_constrain.h), the reference of
tests/test_constrain_cpu.py and tests/test_constrain_gpu.py.  A: dense SPD (n x n), C: k x n of full row rank.

    W = A^-1 C^T,  S = C W = G G^T,  U = W G^-T
    correct(x):  r = C x - e,  t = G^-1 r,  x* = x - U t,  lambda = G^-T t = S^-1 r
    kkt_solve:   [[A, C^T], [C, 0]] [x; lambda] = [b; e]  by numpy.linalg.solve of the bordered matrix
    conditional_cov = A^-1 - W S^-1 W^T
"""
import numpy as np


class Constraints:
    def __init__(self, A, C):
        self.A = np.asarray(A, dtype=np.float64)
        self.C = np.atleast_2d(np.asarray(C, dtype=np.float64))
        self.k, self.n = self.C.shape
        self.W = np.linalg.solve(self.A, self.C.T)
        self.S = self.C @ self.W
        self.S = 0.5 * (self.S + self.S.T)
        self.G = np.linalg.cholesky(self.S)
        self.U = np.linalg.solve(self.G, self.W.T).T            # W G^-T

    def targets(self, e, nvec):
        """e (None, (k,) or (k, nvec)) as a (k, nvec) array"""
        if e is None:
            return np.zeros((self.k, nvec))
        e = np.asarray(e, dtype=np.float64)
        return np.repeat(e[:, None], nvec, axis=1) if e.ndim == 1 else e

    def correct(self, X, e=None):
        """(x*, lambda) for the columns of X ((n,) or (n, nvec))"""
        X = np.asarray(X, dtype=np.float64)
        X2 = X.reshape(self.n, -1)
        r = self.C @ X2 - self.targets(e, X2.shape[1])
        t = np.linalg.solve(self.G, r)
        xs = X2 - self.U @ t
        lam = np.linalg.solve(self.G.T, t)
        return (xs[:, 0], lam[:, 0]) if X.ndim == 1 else (xs, lam)

    def kkt_solve(self, B, e=None):
        """(x, lambda) of the bordered system for the columns of B"""
        B = np.asarray(B, dtype=np.float64)
        B2 = B.reshape(self.n, -1)
        K = np.block([[self.A, self.C.T], [self.C, np.zeros((self.k, self.k))]])
        sol = np.linalg.solve(K, np.vstack([B2, self.targets(e, B2.shape[1])]))
        x, lam = sol[:self.n], sol[self.n:]
        return (x[:, 0], lam[:, 0]) if B.ndim == 1 else (x, lam)

    def solve_constrained(self, B, e=None):
        return self.correct(np.linalg.solve(self.A, np.asarray(B, dtype=np.float64)), e)

    def conditional_cov(self):
        return np.linalg.inv(self.A) - self.W @ np.linalg.solve(self.S, self.W.T)

    def variances(self):
        """diag(A^-1) - sum_j U[:, j]^2: what spllt_hip_inverse_diag_constrained computes"""
        return np.diag(np.linalg.inv(self.A)) - (self.U * self.U).sum(axis=1)

    def log_det_s(self):
        return float(np.linalg.slogdet(self.S)[1])

    def min_relative_pivot(self):
        """min_j pivot_j / S_jj of the Cholesky factorization of S (pivot_j = G_jj^2)"""
        return float((np.diag(self.G) ** 2 / np.diag(self.S)).min())


def residual_bar(C, xs, e):
    """the bound on max |C x* - e| of the tests: 1e-12 (|C|_inf max|x*| + max|e|)"""
    return 1e-12 * (np.abs(C).sum(axis=1).max() * np.abs(xs).max() + (0.0 if e is None else np.abs(e).max()))


def case_matrix(name):
    """the matrices of the GPU tests: (A as scipy CSC, nb, nemin)"""
    from spllt_amd import matgen
    return {"p2d8": (matgen.poisson2d(8), 16, 8), "p2d12": (matgen.poisson2d(12), 16, 8),
            "p3d5": (matgen.poisson3d(5), 16, 8)}[name]


def constraint_rows(k, n, seed=0):
    """C = standard normal (k, n) with row 0 all ones"""
    C = np.random.default_rng(1000 + seed).standard_normal((k, n))
    C[0] = 1.0
    return C
