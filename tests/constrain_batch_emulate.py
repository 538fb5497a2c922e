"""Dense numpy statement of the hard linear constraints of a batch (include/spllt_hip_constrain_batch.h), the
reference of tests/test_constrain_batch_cpu.py and tests/test_constrain_batch_gpu.py: constrain_emulate.Constraints
per member, A_b = batch_emulate.member_matrix(A, b), with ONE C = constrain_emulate.constraint_rows(k, n) for all
members.  Computed once per (matrix, k, nbatch) and shared; nothing here is modified after it is built."""
import functools

import numpy as np

import batch_emulate
import constrain_emulate as emu
from spllt_amd import api

MATS = ("p2d8", "p2d12", "p3d5")
KS = (1, 3, 16, 17, 33, 64)
CASES = [(m, k) for m in MATS for k in KS if not (m == "p2d8" and k == 64)]
NVECS = (1, 5, 32, 33, 40)
NBATCH = 3


class Matrix:
    """the pattern of a case matrix and the members of a batch on it"""

    def __init__(self, name):
        self.name = name
        self.A, self.nb, self.nemin = emu.case_matrix(name)
        self.n, self.ptr, self.row, self.val = api.csc_lower_1based(self.A)

    @functools.lru_cache(maxsize=None)
    def member(self, b):
        """(A_b dense, its values in the order of the analysed pattern)"""
        Ab, v = batch_emulate.member_values(self.A, b, self.ptr, self.row)
        return Ab.toarray(), v

    def values(self, nbatch, scale=1.0):
        return np.ascontiguousarray(np.stack([scale * self.member(b)[1] for b in range(nbatch)]))


@functools.lru_cache(maxsize=None)
def matrix(name):
    return Matrix(name)


@functools.lru_cache(maxsize=None)
def rows(name, k):
    return emu.constraint_rows(k, matrix(name).n)


@functools.lru_cache(maxsize=None)
def member_constraints(name, k, b, scale=1.0):
    """constrain_emulate.Constraints(scale * A_b, C)"""
    return emu.Constraints(scale * matrix(name).member(b)[0], rows(name, k))


class BatchConstraints:
    """the members 0 .. nbatch - 1 of (matrix, k); vectors in the layout of the library: (B, nvec, n)"""

    def __init__(self, name, k, nbatch=NBATCH, scale=1.0):
        self.name, self.k, self.nbatch = name, k, nbatch
        self.n = matrix(name).n
        self.C = rows(name, k)
        self.members = [member_constraints(name, k, b, scale) for b in range(nbatch)]

    def targets(self, e, nvec):
        """e (None, (k,) or (B, nvec, k)) as a list of (k, nvec) arrays, one per member"""
        if e is None or np.ndim(e) == 1:
            return [self.members[0].targets(e, nvec) for _ in range(self.nbatch)]
        return [np.asarray(e[b], dtype=np.float64).T for b in range(self.nbatch)]

    def _per_member(self, fn, X, e):
        X = np.asarray(X, dtype=np.float64)
        E = self.targets(e, X.shape[1])
        out = [getattr(m, fn)(X[b].T, E[b]) for b, m in enumerate(self.members)]
        return np.stack([x.T for x, _ in out]), np.stack([lam.T for _, lam in out])

    def correct(self, X, e=None):
        """(x*, lambda) of shapes (B, nvec, n) and (B, nvec, k) for X of shape (B, nvec, n)"""
        return self._per_member("correct", X, e)

    def solve_constrained(self, Bv, e=None):
        return self._per_member("solve_constrained", Bv, e)

    def kkt_solve(self, Bv, e=None):
        return self._per_member("kkt_solve", Bv, e)

    def variances(self):
        return np.stack([m.variances() for m in self.members])

    def conditional_cov_diag(self):
        return np.stack([np.diag(m.conditional_cov()) for m in self.members])

    def log_det_s(self):
        return np.array([m.log_det_s() for m in self.members])

    def min_relative_pivot(self):
        return np.array([m.min_relative_pivot() for m in self.members])


@functools.lru_cache(maxsize=None)
def batch(name, k, nbatch=NBATCH, scale=1.0):
    return BatchConstraints(name, k, nbatch, scale)
