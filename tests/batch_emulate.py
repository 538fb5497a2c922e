"""Helpers of the batched-factorization tests (TEST-ONLY, never timed): the adapter that feeds the batch
program to the numpy interpreter of tests/emulate.py, and the members of a test batch."""
import numpy as np
import scipy.sparse as sp

from spllt_amd import api

L_GEMM, L_CHAIN = 1, 4
MODE_DIRECT, MODE_SCATTER, MODE_TRSM = 0, 1, 2


class BatchProgramView:
    """answers program(name) with the handle's batch program ("batch_" + name) and passes everything
    else through: emulate.emulate_program(BatchProgramView(f), val) interprets the batch program"""

    def __init__(self, f):
        self._f = f

    def program(self, name):
        return self._f.program("batch_" + name)

    def __getattr__(self, name):
        return getattr(self._f, name)


def member_matrix(A, b):
    """A_b = D_b A D_b, D_b diagonal with entries uniform in [0.5, 2] (default_rng(100 + b)): the pattern
    of A, SPD, its own values and conditioning"""
    d = np.random.default_rng(100 + b).uniform(0.5, 2.0, A.shape[0])
    D = sp.diags(d)
    return sp.csc_matrix(D @ sp.csc_matrix(A) @ D)


def member_values(A, b, ptr, row):
    """(A_b, its values in the CSC-lower order of the analysed pattern)"""
    Ab = member_matrix(A, b)
    n, p, r, v = api.csc_lower_1based(Ab)
    assert np.array_equal(p, ptr) and np.array_equal(r, row), "the scaling changed the pattern"
    return Ab, v


def check_batch_program(f):
    """the batch program holds only what batch.hip implements; returns (launches, units, tiles)"""
    launches, units, tiles = f.program("batch_launches"), f.program("batch_units"), f.program("batch_tiles")
    assert set(launches[:, 0].tolist()) <= {L_CHAIN, L_GEMM}, sorted(set(launches[:, 0].tolist()))
    for kind, _level, first, count, tile in launches[:, :5]:
        if kind != L_GEMM or count == 0:
            continue
        assert tile in (32, 64), tile
        u = units[tiles[first:first + count]["unit"]]
        assert set(u["mode"].tolist()) <= {MODE_DIRECT, MODE_SCATTER, MODE_TRSM}
        assert (u["atomic"][u["mode"] == MODE_DIRECT] == 0).all()
    return launches, units, tiles
