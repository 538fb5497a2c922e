"""CPU tests of the selected-inversion program (schedule.hpp build_selinv_program): its tables
are interpreted in numpy (tests/selinv_emulate.py) on an L from an independent LAPACK Cholesky
and compared with the dense inverse of P A P^T on the pattern of L."""
import numpy as np
import pytest
import scipy.sparse as sp

from helpers import dense_arena, lower_mask, make_case, quintuple_hand_amalgamated, quintuple_single_columns, sym_tables
from selinv_emulate import (SI_DIAG, check_order, emulate_selinv, expected_z, launch_access, panel_inverses,
                            selinv_tables)
from spllt_amd import api, matgen


def _forest():
    """three disconnected components of different shapes"""
    blocks = [matgen.poisson2d(6), matgen.poisson3d(3), sp.identity(5) * 3.0]
    return sp.block_diag(blocks, format="csc")


CASES = [
    ("p2d12-nb4-pw32", lambda: matgen.poisson2d(12), 4, 4, 32),
    ("p2d16-nb8", lambda: matgen.poisson2d(16), 8, 4, 64),
    ("p3d6-nb16", lambda: matgen.poisson3d(6), 16, 8, 64),
    ("box6-nb100-pw32", lambda: matgen.nd_like((6, 6, 6), 2), 100, 8, 32),     # nodes of several block columns
    ("box7-nb256", lambda: matgen.nd_like((7, 7, 6), 2), 256, 16, 64),
    ("box7-nb256-pw32", lambda: matgen.nd_like((7, 7, 6), 2), 256, 16, 32),
    ("p2d10-single-col", lambda: matgen.poisson2d(10), 8, 1, 64),               # nemin 1: single-column nodes
    ("diag", lambda: sp.diags(np.arange(1.0, 31.0)).tocsc(), 8, 4, 64),
    ("n1", lambda: sp.csc_matrix(np.array([[4.0]])), 8, 4, 64),
    ("forest", _forest, 8, 4, 32),
]


def _check(f, A):
    t = selinv_tables(f)
    L = dense_arena(f, A)
    Z = emulate_selinv(f, L, panel_inverses(f, L, t), t)
    ref = expected_z(f, A)
    mask = lower_mask(f)
    assert np.isfinite(Z[mask]).all(), "an entry of the pattern was read before it was written, or never written"
    err = float(np.abs(Z[mask] - ref[mask]).max() / np.abs(ref[mask]).max())
    assert err <= 1e-12, err
    return t


@pytest.mark.parametrize("name,gen,nb,nemin,pw", CASES, ids=[c[0] for c in CASES])
def test_selinv_program_reproduces_inverse(name, gen, nb, nemin, pw):
    A = gen()
    f, val = make_case(A, nb=nb, nemin=nemin, panel_width=pw)
    t = _check(f, A)
    if name == "box6-nb100-pw32":
        tb = sym_tables(f)
        assert (np.diff(tb["node_bcol0"]) > 1).any(), "expected nodes wider than one block column"
    if name == "p2d10-single-col":
        assert (np.diff(sym_tables(f)["sptr"]) == 1).any()
    assert t["scratch"] >= 0


@pytest.mark.parametrize("kind", ["single", "amalgamated"])
def test_selinv_program_on_foreign_symbolic(kind):
    A = matgen.poisson2d(11)
    f0, _ = make_case(A, nb=8, nemin=4)
    quint = quintuple_single_columns(f0) if kind == "single" else quintuple_hand_amalgamated(f0)
    n, ptr, row, val = api.csc_lower_1based(A)
    f = api.Factorization(n, ptr, row, nb=8, nemin=4, symbolic=quint, panel_width=32)
    assert f.sym_info()["ordering"] == "symbolic"
    _check(f, A)


@pytest.mark.parametrize("name,gen,nb,nemin,pw", CASES[:6], ids=[c[0] for c in CASES[:6]])
def test_every_panel_has_one_unit(name, gen, nb, nemin, pw):
    f, _ = make_case(gen(), nb=nb, nemin=nemin, panel_width=pw)
    tb = sym_tables(f)
    units = f.program("selinv_units")
    want = set()
    for b in range(len(tb["bcol_off"])):
        for c0 in range(0, int(tb["bcol_width"][b]), pw):
            want.add((int(tb["bcol_off"][b]), c0))
    got = [(int(u["off"]), int(u["c0"])) for u in units]
    assert len(got) == len(set(got)) == len(want) and set(got) == want
    # every unit is in exactly one DIAG launch, and the DIAG launches cover the units in order
    launches = f.program("selinv_launches")
    d = launches[launches[:, 0] == SI_DIAG]
    assert (d[1:, 2] == d[:-1, 2] + d[:-1, 3]).all() and d[0, 2] == 0 and d[-1, 2] + d[-1, 3] == len(units)
    assert (np.diff(launches[:, 1]) <= 0).all(), "levels from the root down"


@pytest.mark.parametrize("name,gen,nb,nemin,pw", [CASES[1], CASES[3], CASES[9]], ids=[CASES[i][0] for i in (1, 3, 9)])
def test_selinv_launches_order_every_gather(name, gen, nb, nemin, pw):
    """every Z entry a launch gathers was written by an earlier launch; the check catches a program
    whose lowest level runs one step too early"""
    f, _ = make_case(gen(), nb=nb, nemin=nemin, panel_width=pw)
    access = launch_access(f)
    arena = f.sym_info()["arena"]
    assert check_order(access, arena) == []
    assert any(r.size for _, r in access), "expected gathers in this case"
    # mutation: the last launch that gathers moves in front of the DIAG launch before it
    k = max(i for i, (_, r) in enumerate(access) if r.size)
    j = max(i for i in range(k) if access[i][0].size and f.program("selinv_launches")[i, 0] == SI_DIAG)
    mutated = access[:j] + [access[k]] + access[j:k] + access[k + 1:]
    assert check_order(mutated, arena) != []


def test_diag_positions():
    A = matgen.poisson2d(9)
    f, _ = make_case(A, nb=8, nemin=4)
    L = dense_arena(f, A)
    P = np.empty(f.n, dtype=np.int64)
    P[f.sym("order")] = np.arange(f.n)
    import scipy.linalg as sl
    Ld = sl.cholesky(A.toarray()[np.ix_(P, P)], lower=True)
    assert np.allclose(L[f.program("selinv_diag")], np.diag(Ld), rtol=0, atol=0)


def test_inverse_entries_lookup_on_pattern():
    """Factorization.inverse_entries (host lookup) on an emulated Z: the pattern of L in user
    indices, and ValueError off it"""
    A = matgen.poisson2d(10)
    f, _ = make_case(A, nb=8, nemin=4, panel_width=32)
    L = dense_arena(f, A)
    Z = emulate_selinv(f, L, panel_inverses(f, L))
    Ainv = np.linalg.inv(A.toarray())
    Lp = sp.tril(sp.csc_matrix(A)).tocoo()
    got = f.inverse_entries(Lp.row, Lp.col, Z=Z)             # A's own pattern lies inside L's
    assert np.abs(got - Ainv[Lp.row, Lp.col]).max() <= 1e-12 * np.abs(Ainv).max()
    assert np.allclose(f.inverse_entries(Lp.col, Lp.row, Z=Z), got, rtol=0, atol=0)
    assert np.allclose(f.inverse_entries(np.arange(f.n), np.arange(f.n), Z=Z), np.diag(Ainv), rtol=1e-12, atol=0)
    with pytest.raises(ValueError):
        f.inverse_entries(0, f.n - 1, Z=Z)                     # the two ends of the grid: not in L


@pytest.mark.parametrize("flags,chain4", [(0, "0"), (512, "0"), (0, "1"), (1 << 18, "0"), (4096, "0")])
def test_dinv_slots_are_where_the_factorization_writes_them(flags, chain4, monkeypatch):
    """every panel inverse the factor program writes (chain steps, fused panel steps, subtree-task
    nodes) sits at the slot the selinv unit of that panel reads: offset and row stride"""
    monkeypatch.setenv("SPLLT_CHAIN4", chain4)
    f, _ = make_case(matgen.nd_like((7, 7, 6), 2), nb=96, nemin=16, panel_width=32, engine_flags=flags)
    pw = f.program("panel_width")
    slot = {(int(u["off"]), int(u["c0"])): (int(u["dinv_off"]), int(u["dinv_ld"]), int(u["pn"]))
            for u in f.program("selinv_units")}
    seen = 0
    launches = f.program("launches")
    chains = f.program("chains")
    for kind, _, first, count in launches[:, :4]:
        if kind not in (4, 8):
            continue
        for q in chains[first:first + count]:
            cs, ce, ld = int(q["cs"]), int(q["ce"]), int(q["ce"] - q["cs"])
            for c0 in range(int(q["c0"]), int(q["c0"]) + int(q["pn"]), pw):
                if kind == 4:       # one panel: its rows of the chain block's inverse, stride ce - cs
                    want = (int(q["winv_off"]) + (c0 - cs), ld)
                else:               # a chain block: per panel the layout of the one-panel steps
                    pn = min(pw, int(q["c0"]) + int(q["pn"]) - c0)
                    want = (int(q["winv_off"]) + sum(min(pw, ce - c) ** 2 for c in range(cs, c0, pw)), pn)
                assert slot[(int(q["off"]), c0)][:2] == want
                seen += 1
    for p in f.program("panels"):
        assert slot[(int(p["off"]), int(p["c0"]))][:2] == (int(p["dinv_off"]), int(p["pn"]))
        seen += 1
    for nd in f.program("sub_nodes"):
        assert slot[(int(nd["off"]), 0)][:2] == (int(nd["dinv_off"]), int(nd["w"]))
        seen += 1
    assert seen > 0
