"""Helpers of the tests of the batch's factor adjoint (include/spllt_hip_batch_adjoint.h), TEST-ONLY and shared by
tests/test_batch_adjoint_cpu.py and tests/test_batch_adjoint_gpu.py: the batch's selected-inversion tables as the
numpy interpreter of tests/factor_adjoint_emulate.py takes them, the launch count of a sweep computed from those
tables alone, and the references of one member."""
import functools

import numpy as np

import factor_adjoint_emulate as fe
from batch_emulate import member_matrix
from helpers import dense_arena, lower_mask, make_case
from selinv_emulate import SI_DIAG, panel_inverses
from spllt_amd import api

TABLES = ("units", "tiles", "launches", "rows", "relpos", "diag", "scratch")
IDS = [c[0] for c in fe.CASES]

# The largest relative error, on the lower pattern, of the interpreted sweep on the batch tables against the
# dense formula on a LAPACK factor: test_batch_adjoint_cpu.py measures it over all cases of
# factor_adjoint_emulate.CASES, members 0 - 2 and the three seeds, prints it and checks that this record is not
# below what it measures.  The GPU bar is 100 times this (MFMA summation order, the inverted panels of the batch
# factorization): the convention of tests/test_factor_adjoint_gpu.py.
E_MAX = 5.3e-15   # measured 5.268e-15 (p2d64-nb100-pw32), rounded up
GPU_BAR = 100 * E_MAX


def batch_selinv_tables(f):
    return {k: f.program("batch_selinv_" + k) for k in TABLES}


def handle_panel_width(pw):
    """a panel width for the handle that is not the batch's 64"""
    return 32 if pw is None else pw


def steps(t):
    """[(launch indices of the step, fused-eligible)]: a step ends with its DIAG launch; the fused kernel takes it
    when every unit of that launch has at most 64 rows below its panel and at most one K slice"""
    out, cur = [], []
    for i, row in enumerate(t["launches"]):
        kind, first, count = int(row[0]), int(row[2]), int(row[3])
        cur.append(i)
        if kind == SI_DIAG:
            u = t["units"][first:first + count]
            out.append((cur, count > 0 and bool((u["nR"] <= 64).all() and (u["nsplit"] <= 1).all())))
            cur = []
    assert not cur, "the program ends with a DIAG launch"
    return out


def expected_launches(t, fused, nnz=1):
    """kernel launches of one sweep (member ranges not split): 1 per fused step, else one per non-empty launch
    of the step (3, or 2 where nothing lies below the panels), plus the reader"""
    n = 0
    for idx, ok in steps(t):
        n += 1 if (fused and ok) else sum(1 for i in idx if int(t["launches"][i][3]) > 0)
    return n + (1 if nnz > 0 else 0)


@functools.lru_cache(maxsize=None)
def case(name):
    """the handle of a case (panel width != 64), its matrix and the batch tables: computed once, never modified"""
    _, gen, nb, nemin, pw = fe.CASES[IDS.index(name)]
    A = gen()
    f, val = make_case(A, nb=nb, nemin=nemin, panel_width=handle_panel_width(pw))
    return dict(A=A, f=f, val=val, t=batch_selinv_tables(f), mask=lower_mask(f))


@functools.lru_cache(maxsize=None)
def member(name, b):
    """member b of a case: its matrix, values, LAPACK arena, dense factor"""
    c = case(name)
    Ab = member_matrix(c["A"], b)
    _, _, _, vb = api.csc_lower_1based(Ab)
    L = dense_arena(c["f"], Ab)
    return dict(A=Ab, val=vb, L=L, Ld=fe.dense_from_arena(c["f"], L))


def emulate(name, L, seed):
    """the interpreter on the batch tables with the panel inverses of L"""
    c = case(name)
    return fe.emulate_factor_adjoint(c["f"], L, panel_inverses(c["f"], L, c["t"]), seed, c["t"])


def logdet_weight(f):
    w = np.full(f.sym_info()["arena"], 2.0)
    w[f.program("batch_selinv_diag")] = 1.0
    return w
