"""The 64 x 64 POTRF body at its register budget (k_chain_potrf at <= 128 registers per lane,
DESIGN.md section 5): every fragment boundary of its 16 x 16 blocking, through the operator twins
and through tiny factorizations whose chain launches hold several units.

Tolerance: TOL_L of tests/test_gpu_parity.py (imported), max |got - ref| / max |ref| <= 1e-12 over the
meaningful entries.  The blocks are B B^T + n I with Gaussian B (2-norm condition below ~10 for n <= 64,
below ~6 for the widest here, 128), so a backward-stable factor, or the inverse of one, of order n <= 128
carries an error of a few n * 2^-53 ~ 1e-14 relative to its largest entry: two orders below the bar.
"""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg as sl
import scipy.sparse as sp

from helpers import bwd_err, lower_mask, make_case, oracle_factor, rel_err
from spllt_amd import api
from test_gpu_parity import TOL_L

pytestmark = pytest.mark.gpu

# every fragment boundary of the 16 x 16 blocking; identity padding is on where n % 16 != 0
ORDERS = [1, 2, 15, 16, 17, 31, 33, 48, 63, 64]
SENTINEL = 7.25          # what the strict upper triangle holds before the call
DPP = C.POINTER(C.c_double)


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _dev(torch, a, dtype=None):
    return torch.tensor(np.ascontiguousarray(a), device="cuda", dtype=dtype)


def _spd(rng, n):
    B = rng.standard_normal((n, n))
    return B @ B.T + n * np.eye(n)


def _tile(rng, m, n, below):
    """m x n diagonal tile: lower triangle of an SPD block, SENTINEL above it, `below` in the rows under it"""
    S = _spd(rng, n)
    tile = np.full((m, n), SENTINEL)
    tile[:n] = np.tril(S) + np.triu(np.full((n, n), SENTINEL), 1)
    tile[n:] = below
    return S, tile


def _oracle_tile(tile, m, n):
    from oracle import pyoracle
    exp = tile.copy()
    exp[:n] = np.tril(exp[:n])           # the oracle's dpotrf owns the whole n x n head
    assert pyoracle.load("plain").spo_factor_diag_block(m, n, exp.ctypes.data_as(DPP)) == 0
    return exp


def _masks(m, n):
    low = np.ones((m, n), dtype=bool)
    low[:n] = np.tril(np.ones((n, n), dtype=bool))
    return low


@pytest.mark.parametrize("n", ORDERS)
def test_twin_factor_and_inverse_every_fragment_boundary(n):
    """m = 2 n with the identity in the rows below: the tile comes back as [L; inv(L)^T] -- the factor
    and the inverse the kernel stored (the rows below are solved as a product with it)."""
    torch = _torch()
    rng = np.random.default_rng(100 + n)
    m = 2 * n
    S, tile = _tile(rng, m, n, np.eye(n))
    exp = _oracle_tile(tile, m, n)
    d = _dev(torch, tile)
    assert api._lib.load().spllt_factor_diag_block_hip(None, m, n, d.data_ptr(), None) == 0
    got = d.cpu().numpy()
    low = _masks(m, n)
    eL = rel_err(got[:n], exp[:n], low[:n])
    Lref = np.linalg.cholesky(S)
    Wref = sl.solve_triangular(Lref, np.eye(n), lower=True)      # inv(L), numpy / LAPACK
    eLn = rel_err(got[:n], Lref, low[:n])
    eW = rel_err(got[n:].T, Wref)
    eWo = rel_err(got[n:], exp[n:])
    print(f"n={n}: L vs oracle {eL:.2e}, L vs numpy {eLn:.2e}, inv(L) vs numpy {eW:.2e}, vs oracle {eWo:.2e}")
    assert eL <= TOL_L and eLn <= TOL_L and eW <= TOL_L and eWo <= TOL_L
    assert np.all(got[~low] == SENTINEL)                           # nothing outside the lower triangle is written


@pytest.mark.parametrize("n", ORDERS)
def test_twin_second_panel_row_stride_larger_than_n_rows_below(n):
    """block column of width 64 + n: its second panel has order n at row stride 64 + n > n, behind a
    full first panel; 37 rows below (m > n)."""
    torch = _torch()
    w = 64 + n
    m = w + 37
    rng = np.random.default_rng(200 + n)
    S, tile = _tile(rng, m, w, rng.standard_normal((m - w, w)))
    exp = _oracle_tile(tile, m, w)
    d = _dev(torch, tile)
    assert api._lib.load().spllt_factor_diag_block_hip(None, m, w, d.data_ptr(), None) == 0
    got = d.cpu().numpy()
    low = _masks(m, w)
    e = rel_err(got, exp, low)
    e2 = rel_err(got[64:w, 64:], exp[64:w, 64:], low[64:w, 64:])   # the second panel's own block
    print(f"n={n}: tile vs oracle {e:.2e}, second diagonal panel {e2:.2e}")
    assert e <= TOL_L and e2 <= TOL_L
    assert np.all(got[~low] == SENTINEL)


@pytest.mark.parametrize("n", ORDERS + [100])
def test_twin_inverse_only_of_a_given_factor(n):
    """flags bit 0 ("already factored, inverse only"): spllt_solve_block_hip inverts the diagonal panels of
    a GIVEN factor; with the identity as right-hand side the result is inv(L)^T.  (100: two panels.)"""
    torch = _torch()
    from oracle import pyoracle
    rng = np.random.default_rng(300 + n)
    Lkk = np.linalg.cholesky(_spd(rng, n))
    given = Lkk.copy()
    X = np.eye(n)
    exp = X.copy()
    pyoracle.load("plain").spo_solve_block(n, n, exp.ctypes.data_as(DPP), np.ascontiguousarray(Lkk).ctypes.data_as(DPP))
    dk, dx = _dev(torch, given), _dev(torch, X)
    assert api._lib.load().spllt_solve_block_hip(None, n, n, dk.data_ptr(), dx.data_ptr()) == 0
    got = dx.cpu().numpy()
    Wref = sl.solve_triangular(Lkk, np.eye(n), lower=True)
    eo, en = rel_err(got, exp), rel_err(got.T, Wref)
    print(f"n={n}: inv(L)^T vs oracle {eo:.2e}, vs numpy {en:.2e}")
    assert eo <= TOL_L and en <= TOL_L
    assert np.array_equal(dk.cpu().numpy(), given)                 # the factor itself is left as it was


@pytest.mark.parametrize("n,col", [(1, 0), (17, 0), (17, 16), (33, 15), (48, 32), (64, 47), (64, 63), (80, 70)])
def test_twin_not_positive_definite_is_an_error_return(n, col):
    """a_cc made negative: the leading minors up to c - 1 stay positive, pivot c fails.  The device flag
    receives the column the CPU oracle's dpotrf reports (1-based); nothing faults."""
    torch = _torch()
    from oracle import pyoracle
    rng = np.random.default_rng(400 + n + col)
    S = _spd(rng, n)
    S[col, col] = -3.0
    tile = np.tril(S)
    exp = tile.copy()
    info = pyoracle.load("plain").spo_factor_diag_block(n, n, exp.ctypes.data_as(DPP))
    assert info == col + 1
    d = _dev(torch, tile)
    flag = torch.full((1,), np.iinfo(np.int32).max, device="cuda", dtype=torch.int32)
    assert api._lib.load().spllt_factor_diag_block_hip(None, n, n, d.data_ptr(), flag.data_ptr()) == 0
    assert int(flag.item()) == info


def _arrow(sizes, seed, r=20):
    """dense SPD blocks of the given orders, all coupled to r last variables: each block is a leaf
    supernode with r rows below it"""
    rng = np.random.default_rng(seed)
    D = sp.block_diag([_spd(rng, s) for s in sizes]).tocsc()
    Cpl = sp.csc_matrix(rng.standard_normal((D.shape[0], r)) * 0.1)
    return sp.bmat([[D, Cpl], [Cpl.T, sp.identity(r) * 50.0]]).tocsc()


def _chain_launches(f):
    la, ch = f.program("launches"), f.program("chains")
    return [ch[int(l[2]):int(l[2] + l[3])] for l in la if int(l[0]) == 4]


# engine flag 512: no fused panel launches, so every panel step starts with a k_chain_potrf launch
@pytest.mark.parametrize("sizes,want", [
    # leaves of every order in ONE launch (unit 0 in the kernel arguments, the others from the table)
    ([1, 2, 15, 16, 17, 31, 33, 48, 63, 64], {1, 15, 16, 17, 31, 33, 48, 63}),
    # leaves of width 64 + n: second panels of every order at row stride 64 + n
    # (the 128-wide leaf is ordered next to the root: its second panel, order 64, is a launch of its own)
    ([65, 66, 79, 80, 81, 95, 97, 112, 127, 128], {1, 2, 15, 16, 17, 31, 33, 48, 63}),
])
def test_chain_launch_with_several_units_of_different_order(sizes, want):
    _torch()
    A = _arrow(sizes, seed=len(sizes) + sizes[0])
    f, val = make_case(A, nb=128, nemin=1, engine_flags=512)
    launches = _chain_launches(f)
    multi = [u for u in launches if len(u) >= 3 and len(set(int(p) for p in u["pn"])) >= 3]
    assert multi, [list(u["pn"]) for u in launches]
    big = max(multi, key=len)
    assert want <= set(int(p) for p in big["pn"]), list(big["pn"])
    if sizes[0] > 64:
        assert all(int(x["ld"]) > int(x["pn"]) and int(x["c0"]) == 64 for x in big)   # row stride > n
    assert int((f.sym("bcol_nrow") - f.sym("bcol_width")).min()) == 0 < int((f.sym("bcol_nrow") - f.sym("bcol_width")).max())
    got = f.factor(val).wait().get_factor()
    o, rc = oracle_factor(f, val)
    assert rc == 0
    mask = lower_mask(f)
    e = rel_err(got, o.arena(), mask)
    b = A @ np.ones(f.n)
    be = bwd_err(A, f.solve(b), b)          # the solve applies the stored inv(L_pp) of every panel
    print(f"units {[int(p) for p in big['pn']]}: L vs oracle {e:.2e}, bwd_err {be:.2e}")
    assert e <= TOL_L
    assert np.all(got[~mask] == 0.0)        # the arena's upper triangles stay as they were initialised
    assert be <= 1e-14
    f.close()


def test_chain_launch_reports_the_first_failed_pivot_of_a_table_unit():
    """the failing block is not unit 0 of its launch.  The engine reports -20 and the pivot position; the
    CPU side: the oracle fails too, and LAPACK's dpotrf of the permuted dense matrix names the column."""
    _torch()
    A0 = _arrow([16, 33, 17, 48], seed=9)
    f, val = make_case(A0, nb=128, nemin=1, engine_flags=512)
    multi = [u for u in _chain_launches(f) if len(u) >= 3]
    assert multi
    u = multi[0][2]                           # a unit that travels in the table
    pos = int(u["gcol"]) + int(u["pn"]) // 2  # a pivot position inside it
    v = int(np.where(f.sym("order") == pos)[0][0])    # the variable eliminated there
    f.close()
    A = A0.tolil()
    A[v, v] = -3.0                            # (the pattern, and with it the ordering, stays)
    A = A.tocsc()
    f, val = make_case(A, nb=128, nemin=1, engine_flags=512)
    assert int(f.sym("order")[v]) == pos
    P = np.empty(f.n, dtype=np.int64)
    P[f.sym("order")] = np.arange(f.n)
    _, info = sl.lapack.dpotrf(A.toarray()[np.ix_(P, P)], lower=1)
    assert info == pos + 1
    o, rc = oracle_factor(f, val)
    assert rc != 0
    f.factor(val)
    with pytest.raises(api.SplltError) as ei:
        f.wait()
    assert ei.value.flag == -20
    assert "pivot column %d " % info in f.last_error(), f.last_error()
    f.close()
