"""GPU tests of the selected inversion (spllt_hip_selected_inverse and friends): Z = (P A P^T)^-1
on the pattern of L, against the dense inverse and against the numpy interpretation of the same
program (tests/selinv_emulate.py) on the GPU's own L."""
import numpy as np
import pytest
import scipy.sparse as sp

from helpers import bwd_err, lower_mask, make_case
from selinv_emulate import emulate_selinv, expected_z, panel_inverses
from spllt_amd import api, matgen

pytestmark = pytest.mark.gpu

CASES = [
    ("kat3", lambda: sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(3, 3)).tocsc(), 4, 32, None),
    ("p2d12-nb4", lambda: matgen.poisson2d(12), 4, 4, None),
    ("p2d16-nb8-pw32", lambda: matgen.poisson2d(16), 8, 4, 32),
    ("p2d32-nb16", lambda: matgen.poisson2d(32), 16, 32, None),
    ("p2d64-nb100-pw32", lambda: matgen.poisson2d(64), 100, 32, 32),
    ("p3d10-nb48", lambda: matgen.poisson3d(10), 48, 16, None),
    ("box8-nb96", lambda: matgen.nd_like((8, 8, 8), 2), 96, 16, None),
    ("box12-nb256", lambda: matgen.nd_like((12, 12, 11), 3), 256, 32, None),
    ("fe27-nb64", lambda: matgen.fe27((5, 5, 4), 3), 64, 16, None),
    ("box11-nb100-pw48", lambda: matgen.nd_like((11, 10, 10), 3), 100, 16, 48),   # ragged panels
    ("diag", lambda: sp.diags(np.arange(1.0, 41.0)).tocsc(), 8, 4, None),
]


def _rel(a, b, mask):
    return float(np.abs(a[mask] - b[mask]).max() / np.abs(b[mask]).max())


def _inverted(A, nb, nemin, pw, flags=0):
    f, val = make_case(A, nb=nb, nemin=nemin, panel_width=pw, engine_flags=flags)
    f.factor(val).wait()
    f.selected_inverse()
    return f, val


@pytest.mark.parametrize("name,gen,nb,nemin,pw", CASES, ids=[c[0] for c in CASES])
def test_selected_inverse_matches_dense_inverse(name, gen, nb, nemin, pw):
    A = gen()
    f, _ = _inverted(A, nb, nemin, pw)
    Z = f.get_inverse()
    mask = lower_mask(f)
    assert _rel(Z, expected_z(f, A), mask) <= 1e-11
    # the same program interpreted in numpy on the GPU's own L (panel inverses from numpy)
    L = f.get_factor()
    Ze = emulate_selinv(f, L, panel_inverses(f, L))
    assert _rel(Z, Ze, mask) <= 1e-13
    Ainv = np.linalg.inv(A.toarray())
    assert np.abs(f.inverse_diag() - np.diag(Ainv)).max() <= 1e-11 * np.abs(np.diag(Ainv)).max()
    sign, ld = np.linalg.slogdet(A.toarray())
    assert sign > 0 and abs(f.log_det() - ld) <= 1e-12 * max(1.0, abs(ld))
    f.close()


def test_two_runs_are_bit_identical():
    A = matgen.nd_like((12, 12, 11), 3)
    f, _ = _inverted(A, 96, 16, None)
    Z1 = f.get_inverse().copy()
    f.selected_inverse()
    Z2 = f.get_inverse()
    mask = lower_mask(f)
    assert np.array_equal(Z1[mask], Z2[mask])
    f.close()


@pytest.mark.parametrize("variant", ["deterministic", "subtrees", "single_stream", "chain4", "chain_graph"])
def test_same_inverse_under_engine_variants(variant, monkeypatch):
    """Z reads only L and the dinv slots: every engine variant that produces the factor gives the same Z"""
    A = matgen.nd_like((12, 12, 11), 3)
    nb, nemin = 256, 16
    base, _ = _inverted(A, nb, nemin, 64)
    Z0 = base.get_inverse().copy()
    mask = lower_mask(base)
    base.close()
    flags = {"deterministic": 4096, "subtrees": 1 << 18, "single_stream": 2}.get(variant, 0)
    if variant == "chain4":
        monkeypatch.setenv("SPLLT_CHAIN4", "1")
    if variant == "chain_graph":
        monkeypatch.delenv("SPLLT_CHAIN_GRAPH_SERIAL", raising=False)   # the default factor path
    f, _ = _inverted(A, nb, nemin, 64, flags)
    assert _rel(f.get_inverse(), Z0, mask) <= 1e-13
    f.close()


def test_inverse_entries_on_and_off_pattern():
    A = matgen.poisson2d(24)
    f, _ = _inverted(A, 16, 8, None)
    Ainv = np.linalg.inv(A.toarray())
    Lp = sp.tril(sp.csc_matrix(A)).tocoo()
    got = f.inverse_entries(Lp.row, Lp.col)
    assert np.abs(got - Ainv[Lp.row, Lp.col]).max() <= 1e-11 * np.abs(Ainv).max()
    assert np.array_equal(f.inverse_entries(Lp.col, Lp.row), got)
    with pytest.raises(ValueError):
        f.inverse_entries(0, f.n - 1)
    f.close()


def test_refactor_makes_inverse_stale():
    A = matgen.poisson2d(20)
    f, val = _inverted(A, 16, 8, None)
    f.get_inverse()
    A2 = A + sp.identity(A.shape[0]) * 0.5
    n, ptr, row, val2 = api.csc_lower_1based(A2)
    f.factor(val2).wait()
    for read in (f.get_inverse, f.inverse_diag):
        with pytest.raises(api.SplltError) as ei:
            read()
        assert ei.value.flag == -10 and "selected_inverse" in f.last_error()
    f.selected_inverse()
    assert _rel(f.get_inverse(), expected_z(f, A2), lower_mask(f)) <= 1e-11
    sign, ld = np.linalg.slogdet(A2.toarray())
    assert abs(f.log_det() - ld) <= 1e-12 * abs(ld)
    f.release_inverse()
    with pytest.raises(api.SplltError):
        f.get_inverse()
    f.close()


def test_solve_after_inversion():
    A = matgen.nd_like((10, 10, 9), 2)
    f, _ = _inverted(A, 96, 16, None)
    b = A @ np.random.default_rng(3).standard_normal(A.shape[0])
    x = f.solve(b)
    assert bwd_err(A, x, b) <= 1e-14
    f.close()


def test_partitioned_factor_returns_unimplemented_after_factor():
    """a rank of a partition that has factored its part: the inversion is not available"""
    import torch
    from helpers import drive_exchanges
    A = matgen.poisson2d(32)
    fs, bufs = [], []
    for r in range(2):
        f, val = make_case(A, nb=16, nemin=8, prune=True, ncpu=2)
        xb = torch.zeros(max(1, f.set_partition(r, 2)), dtype=torch.float64, device="cuda")
        f.set_exchange_buffer(xb.data_ptr())
        fs.append(f)
        bufs.append(xb)
    dval = torch.tensor(val, device="cuda")
    torch.cuda.synchronize()
    for f in fs:
        f.factor_dev(dval.data_ptr())
    drive_exchanges(fs, bufs)
    for f in fs:
        f.wait()
        with pytest.raises(api.SplltError) as ei:
            f.selected_inverse()
        assert ei.value.flag == -98 and "partitioned" in f.last_error()
    for f in fs:
        f.close()


def test_full_size_columns_agree_with_solves():
    """nd24k_like at full size: for 8 seeded columns j, x = A^-1 e_j from a solve agrees with Z on
    the pattern of L's column j (pivot order) and its diagonal"""
    A, order, cfg = matgen.build_config("nd24k_like", 1.0)
    n, ptr, row, val = api.csc_lower_1based(A)
    f = api.Factorization(n, ptr, row, nb=cfg["nb"], nemin=32, prune_tree=False, order=order)
    f.factor(val).wait()
    f.selected_inverse()
    Z = f.get_inverse()
    t = {k: f.sym(k) for k in ("order", "sptr", "rptr", "rlist", "node_bcol0", "bcol_off", "bcol_width", "bcol_r0")}
    porder = np.empty(n, dtype=np.int64)
    porder[t["order"]] = np.arange(n)
    rng = np.random.default_rng(24)
    cols = rng.choice(n, size=8, replace=False)
    node_of = np.repeat(np.arange(len(t["sptr"]) - 1), np.diff(t["sptr"]))
    for c in cols:                                  # c: pivot position
        s = node_of[c]
        k = c - t["sptr"][s]
        b = t["node_bcol0"][s] + k // cfg["nb"]
        r0, w, off = int(t["bcol_r0"][b]), int(t["bcol_width"][b]), int(t["bcol_off"][b])
        rows = t["rlist"][t["rptr"][s] + k:t["rptr"][s + 1]]          # pivot positions of column c's pattern
        pos = off + (np.arange(k, k + len(rows)) - r0) * w + (k - r0)
        e = np.zeros(n)
        e[porder[c]] = 1.0
        x = f.solve(e)
        want = x[porder[rows]]
        assert np.abs(Z[pos] - want).max() <= 1e-10 * np.abs(want).max(), int(c)
    f.close()
