"""Backward-error tests of the factorization, the three solves and the batch on ill-conditioned, graded and
scaled SPD input, and the report of a failed or non-finite pivot wherever it can fall.

Bars.  On ill-conditioned input only backward metrics are used (hard_inputs: eta, omega, inv_resid, evaluated in
longdouble), never rel_err of L: two backward-stable factors already differ by cond(A) u.  Every bar is a ratio
to a CPU computation checked in tests/test_conditioning_cpu.py:

  eta_gpu   <= 16 max(eta of the emulated program, eta of the oracle)
  omega_gpu <= 16 max(omega of model_solve on the emulated factor, omega of the oracle's solve)

The emulated program (tests/emulate.py) and model_solve run the engine's ALGORITHM -- the rows below a panel and
the substitution as products with inv(L_pp) -- in LAPACK arithmetic.  The margin 16 covers what they do not
model: the 16 x 16 inverse-multiply inside a panel (one more term of the same order, u kappa of a sub-block
<= u kappa(L_pp)), pivots one or two ulp off from the Newton-refined rsq / rcp, and the summation order of the
matrix cores and the atomics.  A lost Newton step, a wrong K window or a dropped update is orders of magnitude
outside it.  With several right-hand sides the worst column of the device is held against the worst column of
the references (the rounding errors of two implementations are not correlated column by column; their sizes are).
Benign cases also meet absolute bars (eta <= 64 u, the reference's omega <= 1e-14); on the hard cases
(Hilbert + 1e-10 I: the algorithm itself crosses 1e-14) solve_refined must reach 1e-14.

Lines that start with ENVELOPE carry the measured figures of DESIGN.md section 20 (run with -s)."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg as sl
import scipy.sparse as sp

import hard_inputs as hi
from batch_emulate import BatchProgramView
from helpers import bwd_err, lower_mask, make_case, oracle_factor, rel_err
from spllt_amd import api, matgen
from test_gpu_parity import TOL_L

pytestmark = pytest.mark.gpu
U = hi.U
MARGIN = 16.0
DPP = C.POINTER(C.c_double)

# engine paths: (environment, engine flags)
PATHS = {
    "default": ({}, 0),
    "deterministic": ({}, 4096),
    "chain4": ({"SPLLT_CHAIN4": "1"}, 0),
    "subtrees": ({"SPLLT_SUBTREES": "1", "SPLLT_SUBTREE_US": "300"}, 0),
    "graph": ({}, 32768),
    "nofused": ({}, 512),
}


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _dev(torch, a, dtype=None):
    return torch.tensor(np.ascontiguousarray(a), device="cuda", dtype=dtype)


def _check_path(f, path, pw, need_subtree_task=True):
    """the program holds the kernel kinds the path is about; skips where the structure has no room for them
    (need_subtree_task=False: an input without a subtree task is such a structure, not a mistake of the case)"""
    kinds = f.program("launches")[:, 0]
    if path == "deterministic":
        assert (kinds == 6).any()                       # k_gather
    elif path == "chain4":
        if int(f.sym("bcol_width").max()) <= pw:
            pytest.skip(f"no block column of this case has two panels (widest {int(f.sym('bcol_width').max())}, panel {pw})")
        assert (kinds == 8).any() and (kinds == 9).any()   # k_chain_block, k_trsm_rows
    elif path == "subtrees":
        if need_subtree_task or (kinds == 10).any():
            assert (kinds == 10).sum() == 1             # k_subtree
        else:
            pytest.skip("the tree of this input has no subtree task: the program is the default one")
    elif path == "nofused":
        assert not (kinds == 7).any() and (kinds == 4).any()
    return kinds


CASE_PATHS = [(cid, path) for cid in hi.CASE_IDS for path in PATHS if path != "subtrees" or cid in hi.SPARSE]


@pytest.mark.parametrize("cid,path", CASE_PATHS)
def test_backward_error_of_factor_and_solves(cid, path, monkeypatch):
    _torch()
    env, flags = PATHS[path]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    A, b, f, val, pw, cls = hi.make(cid, engine_flags=flags)
    _check_path(f, path, pw)
    r = hi.references(f, A, val, b, pw, key=cid)
    f.factor(val).wait()
    if path == "graph":
        f.factor(val).wait()                            # the replay of the captured graph
    Lg = hi.dense_L(f, f.get_factor())
    assert np.isfinite(Lg).all()
    eta_gpu = hi.eta(r["Ap"], Lg)
    eta_ref = max(r["eta_emul"], r["eta_oracle"])
    uk = U * r["kappa"]
    om = {"solve": np.atleast_1d(hi.omega(A, f.solve(b[:, 0]), b[:, 0])),
          "solve_many": hi.omega(A, f.solve_many(b), b),
          "solve_reproducible": np.atleast_1d(hi.omega(A, f.solve_reproducible(b[:, 0]), b[:, 0]))}
    om_ref = {k: MARGIN * max(r["omega_model"][:v.size].max(), r["omega_oracle"][:v.size].max()) for k, v in om.items()}
    line = (f"ENVELOPE {cid} {path} {cls} kappa_pp={r['kappa']:.1e} eta_gpu={eta_gpu:.2e} eta_emul={r['eta_emul']:.2e} "
            f"eta_emul16={r['eta_emul16']:.2e} eta_oracle={r['eta_oracle']:.2e} eta_gpu/(u kappa)={eta_gpu / uk:.1e} "
            f"eta_emul/(u kappa)={r['eta_emul'] / uk:.1e} " +
            " ".join(f"omega_{k}={v.max():.2e}" for k, v in om.items()) +
            f" omega_model={r['omega_model'].max():.2e} omega_oracle={r['omega_oracle'].max():.2e}")
    if cls == "hard":
        xr, its, _ = f.solve_refined(val, b[:, :3], method="ir", tol=1e-14, max_iter=50)
        om_ir = hi.omega(A, xr, b[:, :3])
        line += f" refine_status={f.refine_status} ir_iterations={its.tolist()} omega_ir={om_ir.max():.2e}"
    print("\n" + line)
    assert eta_gpu <= MARGIN * eta_ref
    for k, v in om.items():
        assert v.max() <= om_ref[k], k
    # the remainder block of solve_many (column 33 alone) also against its OWN reference: behind the worst of the
    # 32 columns of the full block it could hide
    assert om["solve_many"][32] <= MARGIN * max(r["omega_model"][32], r["omega_oracle"][32])
    if cls == "benign":
        assert eta_gpu <= 64 * U
        for k, v in om.items():
            assert v.max() <= 1e-14, k
    else:
        assert f.refine_status == 0
        assert om_ir.max() <= 2e-14       # (the library's own residual is fp64, this one longdouble)
    f.close()


# ---- graded and scaled input ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("kind", hi.EQUI_KINDS)
@pytest.mark.parametrize("opts", range(len(hi.EQUI_OPTS)))
@pytest.mark.parametrize("base", range(len(hi.EQUI_BASES)))
def test_power_of_two_scaling_is_undone_exactly(base, opts, kind, path, monkeypatch):
    """D A D with D = diag(2**e): e seeded in [-100, 100] per variable (graded), or all 300 / -300 (A 2**600,
    A 2**-600), on every engine path (both matrices are sparse; under flags 32768 the scaled values are a replay
    of the graph captured with the values of A).  Unscaled exactly on the host, the factor meets the ordinary
    TOL_L against the oracle's factor of the UNSCALED A, and with b = D A 1, D x is the vector of ones to the
    suite's 1e-9.  (2**+-1000 is out of range by design -- y * y in the POTRF -- and not tested.)  Flags 4096:
    whether the unscaled factor is bit-identical to the factor of A is printed, not asserted (it depends on
    v_rsq_f64 being exponent-equivariant)."""
    _torch()
    env, flags = PATHS[path]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    name, gen = hi.EQUI_BASES[base]
    A = gen()
    f, val = make_case(A, engine_flags=flags, **hi.EQUI_OPTS[opts])
    _check_path(f, path, int(f.program("panel_width")))
    e = hi.equi_scaling(kind, f.n, seed=11 + base)
    n, ptr, row, vs = api.csc_lower_1based(hi.graded(A, e))
    assert np.array_equal(ptr, f.ptr) and np.array_equal(row, f.row)
    o, rc = oracle_factor(f, val)
    assert rc == 0
    Lo = hi.dense_L(f, o.arena())
    L0 = hi.dense_L(f, f.factor(val).wait().get_factor())
    Ls = hi.dense_L(f, f.factor(vs).wait().get_factor())
    assert np.isfinite(Ls).all()
    ep = e[hi.pivot_perm(f)].astype(np.int32)
    Lu = np.ldexp(Ls, -ep[:, None])
    err = rel_err(Lu, Lo)
    b = np.ldexp(A @ np.ones(f.n), e.astype(np.int32))
    x = f.solve(b)
    Dx = np.ldexp(x, e.astype(np.int32))
    print(f"\nENVELOPE scaling {name} opts{opts} {kind} {path} unscaled L vs oracle {err:.2e} max|Dx-1|={np.abs(Dx - 1).max():.2e}"
          + (f" bit-identical to the factor of A: {np.array_equal(Lu, L0)}" if flags == 4096 else ""))
    assert err <= TOL_L
    np.testing.assert_allclose(Dx, np.ones(f.n), rtol=0, atol=1e-9)
    f.close()


# ---- the batch (batch.hip has its own POTRF) -------------------------------------------------------------------------
def test_batch_of_benign_hard_and_scaled_members():
    _torch()
    A0, _, f, v0, pw, _ = hi.make("h192-s2")
    members = [("benign", A0), ("hard", hi.case_inputs("h192-s10")["A"]), ("benign", hi.scaled(A0, 600))]
    vals, bs = [], []
    for _, Am in members:
        n, ptr, row, v = api.csc_lower_1based(Am)
        assert np.array_equal(ptr, f.ptr) and np.array_equal(row, f.row)
        vals.append(v)
        bs.append(hi.rhs(Am, nrhs=3))
    assert f.factor_batch(np.stack(vals)) == 0
    xb = f.solve_batch(np.stack([b.T for b in bs]))            # (B, nrhs, n)
    for m, (cls, Am) in enumerate(members):
        r = hi.references(f, Am, vals[m], bs[m], pw, prog=BatchProgramView(f))
        eta_gpu = hi.eta(r["Ap"], hi.dense_L(f, f.get_factor_batch(m)))
        om = hi.omega(Am, xb[m].T, bs[m])
        print(f"\nENVELOPE batch member {m} {cls} kappa_pp={r['kappa']:.1e} eta_gpu={eta_gpu:.2e} eta_emul={r['eta_emul']:.2e} "
              f"eta_oracle={r['eta_oracle']:.2e} omega_gpu={om.max():.2e} omega_model={r['omega_model'].max():.2e} "
              f"omega_oracle={r['omega_oracle'].max():.2e}")
        assert eta_gpu <= MARGIN * max(r["eta_emul"], r["eta_oracle"])
        assert om.max() <= MARGIN * max(r["omega_model"].max(), r["omega_oracle"].max())
        if cls == "benign":
            assert eta_gpu <= 64 * U and om.max() <= 1e-14
    f.close()


# ---- kernel twins under conditioning: the panel without the program ----------------------------------------------------
@pytest.mark.parametrize("n", [16, 17, 48, 63, 64])
def test_twin_factor_and_inverse_of_a_hilbert_block(n):
    """spllt_factor_diag_block_hip with m = 2 n and the identity below (tests/test_potrf_small_gpu.py): the tile comes
    back as [L; inv(L)^T], on the leading block of Hilbert + 1e-10 I.
    Reference of eta: the oracle's twin and LAPACK for n = 16; for n > 16 ALSO the 16-blocked inverse-multiply
    model of the panel (hard_inputs.panel_chol16, steps A1-A3 of potrf64_body in LAPACK arithmetic).  Measured on
    the MI355X, n = 17 / 48 / 63 / 64: eta_gpu = 1.6e-15 / 4.1e-15 / 4.2e-15 / 4.2e-15 against LAPACK's 3e-17 ..
    7e-17 (24 .. 60 times the margin), and against the model's 1.3e-15 / 3.5e-15 / 3.7e-15 / 3.7e-15 (a factor
    1.1 - 1.2); n = 16, a single block, meets LAPACK's.  The excess is the documented step A3 -- the blocks below
    a 16 x 16 diagonal block are a product with its explicit inverse, kappa(D_J) = 1.4e5 here -- and not a
    defect of the kernel."""
    torch = _torch()
    from oracle import pyoracle
    S = hi.hilbert_shift(n, 1e-10).toarray()
    tile = np.vstack([np.tril(S), np.eye(n)])
    exp = tile.copy()
    assert pyoracle.load("plain").spo_factor_diag_block(2 * n, n, exp.ctypes.data_as(DPP)) == 0
    Ll = np.linalg.cholesky(S)
    d = _dev(torch, tile)
    assert api._lib.load().spllt_factor_diag_block_hip(None, 2 * n, n, d.data_ptr(), None) == 0
    got = d.cpu().numpy()
    L, W = np.tril(got[:n]), got[n:].T
    e_gpu, e_or, e_la = hi.eta(S, L), hi.eta(S, np.tril(exp[:n])), hi.eta(S, Ll)
    e_16 = hi.eta(S, hi.panel_chol16(S)[0])
    i_gpu, i_la = hi.inv_resid(L, W), hi.inv_resid(Ll, sl.solve_triangular(Ll, np.eye(n), lower=True))
    print(f"\nENVELOPE twin potrf n={n} kappa(L)={np.linalg.cond(Ll):.1e} eta gpu {e_gpu:.2e} oracle {e_or:.2e} lapack {e_la:.2e} 16-blocked model {e_16:.2e} "
          f"inv_resid gpu {i_gpu:.2e} lapack {i_la:.2e}")
    assert np.isfinite(got).all()
    assert e_gpu <= MARGIN * max(e_or, e_la, e_16)
    assert i_gpu <= MARGIN * i_la


@pytest.mark.parametrize("m,n", [(7, 5), (100, 64), (129, 130)])
def test_twin_solve_block_against_a_hilbert_factor(m, n):
    """spllt_solve_block_hip: X L_kk^T = B with L_kk the longdouble factor of Hilbert + 1e-10 I, rounded"""
    torch = _torch()
    from oracle import pyoracle
    Lkk = np.ascontiguousarray(hi.chol_ld(hi.hilbert_shift(n, 1e-10).toarray()).astype(np.float64))
    B = np.random.default_rng(m + 7 * n).standard_normal((m, n))
    exp = B.copy()
    pyoracle.load("plain").spo_solve_block(m, n, exp.ctypes.data_as(DPP), Lkk.ctypes.data_as(DPP))
    Xinv = B @ sl.solve_triangular(Lkk, np.eye(n), lower=True).T
    dk, dx = _dev(torch, Lkk), _dev(torch, B)
    assert api._lib.load().spllt_solve_block_hip(None, m, n, dk.data_ptr(), dx.data_ptr()) == 0
    X = dx.cpu().numpy()

    def resid(X):
        Xl, Ll = X.astype(hi.LD), Lkk.astype(hi.LD)
        return float(hi._fro(Xl @ Ll.T - B.astype(hi.LD)) / (hi._fro(Xl) * hi._fro(Ll)))
    r_gpu, r_inv, r_or = resid(X), resid(Xinv), resid(exp)
    print(f"\nENVELOPE twin trsm m={m} n={n} kappa(L)={np.linalg.cond(Lkk):.1e} resid gpu {r_gpu:.2e} product with inv {r_inv:.2e} "
          f"oracle {r_or:.2e}")
    assert np.isfinite(X).all()
    assert r_gpu <= MARGIN * max(r_inv, r_or)


# ---- where a pivot fails ------------------------------------------------------------------------------------------------
def _spd(n, seed):
    B = np.random.default_rng(seed).standard_normal((n, n))
    return sp.csc_matrix(B @ B.T + n * np.eye(n))


def _diag_index(f, v):
    """index into val of the diagonal entry of variable v (CSC lower, sorted: the first of its column)"""
    k = int(f.ptr[v]) - 1
    assert int(f.row[k]) - 1 == v
    return k


def _break_pivot(f, A, val, p):
    """pivots before position p untouched, pivot p clearly negative in any arithmetic: 1.5 T[p,p]^2 is taken
    from the diagonal entry of the variable eliminated there (T the longdouble factor of P A P^T)"""
    T = hi.chol_ld(hi.permuted(f, A))
    v = int(hi.pivot_perm(f)[p])
    bad = val.copy()
    bad[_diag_index(f, v)] -= 1.5 * float(T[p, p]) ** 2
    return bad, v


def _check_failed_pivot(f, A, val, bad, p):
    """-20 from the engine, failure from the oracle on the same values, LAPACK names the column; the next
    factorization of the clean values is clean; (clean, broken, clean) through factor_batch (also under
    SPLLT_CHAIN4=1 / SPLLT_SUBTREES=1, which the batch program ignores)"""
    P = hi.pivot_perm(f)
    Ab = sp.csc_matrix(A).toarray()
    i = np.arange(f.n)
    Ab[i, i] = bad[[_diag_index(f, int(v)) for v in i]]
    _, info = sl.lapack.dpotrf(Ab[np.ix_(P, P)], lower=1)
    assert info == p + 1
    o, rc = oracle_factor(f, bad)
    assert rc != 0
    with pytest.raises(api.SplltError) as ei:
        f.factor(bad).wait()
    assert ei.value.flag == -20
    assert "pivot column %d " % (p + 1) in f.last_error(), f.last_error()     # 1-based, in elimination order
    o, rc = oracle_factor(f, val)
    assert rc == 0
    ref, mask = o.arena(), lower_mask(f)
    got = f.factor(val).wait().get_factor()
    assert rel_err(got, ref, mask) <= TOL_L
    b = A @ np.ones(f.n)
    assert bwd_err(A, f.solve(b), b) <= 1e-14
    assert f.factor_batch(np.stack([val, bad, val])) == -20
    flags, cols = f.batch_status()
    assert flags.tolist() == [0, -20, 0]
    assert cols.tolist() == [0, p + 1, 0]
    for m in (0, 2):
        assert rel_err(f.get_factor_batch(m), ref, mask) <= TOL_L


def _bcol_of(f, p):
    """(block column, offset in it) of pivot position p"""
    t = hi.sym_tables(f)
    for b in range(len(t["bcol_off"])):
        c0 = int(t["sptr"][int(t["bcol_node"][b])]) + int(t["bcol_r0"][b])
        if c0 <= p < c0 + int(t["bcol_width"][b]):
            return b, p - c0
    raise AssertionError(p)


@pytest.mark.parametrize("pw,p", [(None, 31), (None, 47), (None, 63),     # last column of the 2nd, 3rd, 4th 16-block
                                  (48, 48),                              # first column of a second panel
                                  (48, 60)])                             # inside the ragged last panel (48 + 16)
def test_failed_pivot_inside_a_dense_root(pw, p):
    _torch()
    A = _spd(130, 5)
    f, val = make_case(A, nb=64, nemin=4, panel_width=pw)
    b, k = _bcol_of(f, p)
    assert len(f.sym("sparent")) == 1 and int(f.sym("bcol_width")[b]) == 64 and b == 0 and k == p
    assert int(f.program("panel_width")) == (pw or 64)
    bad, _ = _break_pivot(f, A, val, p)
    _check_failed_pivot(f, A, val, bad, p)
    f.close()


def test_failed_pivot_in_the_third_panel_of_a_chain_block(monkeypatch):
    _torch()
    monkeypatch.setenv("SPLLT_CHAIN4", "1")
    A = _spd(260, 6)
    f, val = make_case(A, nb=256, nemin=4)
    ch = f.program("chains")
    kinds = f.program("launches")[:, 0]
    assert (kinds == 8).any() and len(ch) == 1 and int(ch[0]["c0"]) == 0 and int(ch[0]["pn"]) == 256
    p = 2 * 64 + 21
    bad, _ = _break_pivot(f, A, val, p)
    _check_failed_pivot(f, A, val, bad, p)
    f.close()


@pytest.mark.parametrize("flags", [0, 4096, 32768])
@pytest.mark.parametrize("which", ["nd887", "bih2d-20"])
def test_failed_pivot_in_the_root_front_after_the_updates(which, flags):
    """nd887: a column of the root front of nd_like((8,8,7),2).  bih2d-20: a root column whose diagonal entry is
    still POSITIVE in the input after 1.5 T[p,p]^2 is taken from it (the updates take more than a third of a_vv
    there; no column of the diagonally dominant nd_like has that): the pivot only fails once the updates of the
    descendants have arrived."""
    _torch()
    A = matgen.nd_like((8, 8, 7), 2) if which == "nd887" else hi.biharmonic2d(20)
    f, val = make_case(A, nb=48, nemin=8, engine_flags=flags)
    sptr = f.sym("sptr")
    root0 = int(sptr[-2])
    assert len(sptr) > 2 and int(sptr[-1]) == f.n
    if which == "nd887":
        p = root0 + 37
        bad, v = _break_pivot(f, A, val, p)
    else:
        T = hi.chol_ld(hi.permuted(f, A))
        P = hi.pivot_perm(f)
        d = A.diagonal()
        ok = [q for q in range(root0, f.n) if d[P[q]] - 1.5 * float(T[q, q]) ** 2 > 0.25 * d[P[q]]]
        assert ok, "no root column stays positive in the input"
        p = ok[len(ok) // 2]
        bad, v = _break_pivot(f, A, val, p)
        assert bad[_diag_index(f, v)] > 0
    assert root0 <= p < f.n
    _check_failed_pivot(f, A, val, bad, p)
    f.close()


def test_failed_pivot_in_a_node_inside_a_subtree_task(monkeypatch):
    _torch()
    monkeypatch.setenv("SPLLT_SUBTREES", "1")
    monkeypatch.setenv("SPLLT_SUBTREE_US", "300")
    A = matgen.nd_like((8, 8, 7), 2)
    f, val = make_case(A, nb=48, nemin=8)
    assert (f.program("launches")[:, 0] == 10).sum() == 1
    tasks, nodes = f.program("sub_tasks"), f.program("sub_nodes")
    t = tasks[len(tasks) // 2]
    assert int(t["node_count"]) >= 3
    nd = nodes[int(t["node_first"]) + 1]                # neither the task's first node nor its root
    assert not int(nd["root"])
    p = int(nd["gcol"]) + int(nd["w"]) // 2
    bad, _ = _break_pivot(f, A, val, p)
    _check_failed_pivot(f, A, val, bad, p)
    f.close()


def test_failed_pivot_in_a_fused_panel_step(monkeypatch):
    _torch()
    monkeypatch.setenv("SPLLT_FUSED_PANEL_MAX", "1000000")
    monkeypatch.setenv("SPLLT_SUBTREES", "0")
    A = matgen.poisson2d(6)
    f, val = make_case(A, nb=64, nemin=4)
    assert (f.program("launches")[:, 0] == 7).any()      # k_panel
    q = max(f.program("panels"), key=lambda u: int(u["pn"]))
    assert not int(q["pad_"]) & 1                        # the fused launch factors the panel itself
    p = int(q["gcol"]) + int(q["pn"]) - 1
    bad, _ = _break_pivot(f, A, val, p)
    _check_failed_pivot(f, A, val, bad, p)
    f.close()


def test_exactly_zero_pivot():
    """block_diag(poisson2d(6), [[1, 1], [1, 1]]): the last pivot, 1 - 1 * 1, is exactly 0 in every arithmetic"""
    _torch()
    Z = sp.block_diag([matgen.poisson2d(6), np.ones((2, 2))]).tocsc()
    G = sp.block_diag([matgen.poisson2d(6), np.array([[2.0, 1.0], [1.0, 2.0]])]).tocsc()   # the same pattern, SPD
    f, bad = make_case(Z, nb=64, nemin=4)
    n, ptr, row, val = api.csc_lower_1based(G)
    assert np.array_equal(ptr, f.ptr) and np.array_equal(row, f.row)
    order = f.sym("order")
    assert sorted(order[36:].tolist()) == [36, 37]       # the 2 x 2 block is eliminated last
    _check_failed_pivot(f, G, val, bad, 37)
    f.close()


# ---- non-finite values ------------------------------------------------------------------------------------------------
NONFINITE_PATHS = ["default", "nofused", "subtrees", "graph"]


def _expect_not_posdef(f, bad, what):
    """the failure to guard against is flag 0 with a non-finite entry in the factor"""
    try:
        f.factor(bad).wait()
        flag = 0
    except api.SplltError as e:
        flag = e.flag
    note = ""
    if flag == 0:
        note = f"; the factor holds {int((~np.isfinite(f.get_factor())).sum())} non-finite entries"
    assert flag == -20, f"{what}: flag {flag}{note}"


def _leaf_last_pivot(f):
    """the last pivot position of a leaf supernode (it has rows below it)"""
    sptr, spar = f.sym("sptr"), f.sym("sparent")
    leaves = [s for s in range(len(spar)) if s not in set(spar.tolist())]
    return int(sptr[leaves[len(leaves) // 2] + 1]) - 1


@pytest.mark.parametrize("path", NONFINITE_PATHS)
@pytest.mark.parametrize("what", ["nan-offdiag", "nan-diag", "inf-leaf", "inf-isolated16", "inf-last64"])
def test_non_finite_values_are_reported(what, path, monkeypatch):
    """NaN anywhere, and +Inf on the diagonal of a LAST pivot, are 'not positive definite' (-20), as they are in
    the batch (batch.hip: positive AND finite).  The +Inf pivots:
      inf-leaf        last pivot of a leaf of nd_like((8,8,7),2): rows below it, a parent behind it;
      inf-isolated16  last pivot of a dense component of order 16 = one 16 x 16 block of the POTRF, nothing behind;
      inf-last64      last pivot of a dense matrix of order 64 = the last column of a full panel.
    rsq(Inf) = 0 and rcp(Inf) = 0 turn into NaN in the first Newton step, and that NaN reaches a LATER pivot of
    the same 16 x 16 block (identity padding included) or of an ancestor, where `!(d > 0)` catches it -- except
    where no pivot follows at all: the last two cases.  There the predicate `!(d > 0)` alone returned flag 0 and
    a factor with NaN in it.  Path "subtrees" is run where the pivot's node is inside a subtree task and skipped
    where the input has none (the dense matrix of order 64 is one node, the root)."""
    _torch()
    env, flags = PATHS[path]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if what == "inf-isolated16":
        A = sp.block_diag([matgen.poisson2d(6), _spd(16, 8)]).tocsc()
        f, val = make_case(A, nb=64, nemin=4, engine_flags=flags)
        P = hi.pivot_perm(f)
        p = max(q for q in range(f.n) if P[q] >= 36)    # the last pivot of the dense component
        s = int(np.searchsorted(f.sym("sptr"), p, side="right")) - 1
        rptr = f.sym("rptr")
        assert int(f.sym("sptr")[s + 1]) - int(f.sym("sptr")[s]) == 16 == int(rptr[s + 1] - rptr[s])
        assert p == int(f.sym("sptr")[s + 1]) - 1
        _check_path(f, path, int(f.program("panel_width")), need_subtree_task=False)
    elif what == "inf-last64":
        A = _spd(64, 9)
        f, val = make_case(A, nb=64, nemin=4, engine_flags=flags)
        assert len(f.sym("sparent")) == 1
        p = 63
        _check_path(f, path, int(f.program("panel_width")), need_subtree_task=False)
    else:
        A = matgen.nd_like((8, 8, 7), 2)
        f, val = make_case(A, nb=48, nemin=8, engine_flags=flags)
        _check_path(f, path, int(f.program("panel_width")))
        p = _leaf_last_pivot(f)
    if path == "subtrees" and not any(int(nd["gcol"]) <= p < int(nd["gcol"]) + int(nd["w"]) for nd in f.program("sub_nodes")):
        pytest.skip("the node of this pivot is in no subtree task: it would go through the default path's kernels")
    bad = val.copy()
    v = int(hi.pivot_perm(f)[p])
    if what == "nan-offdiag":
        k = _diag_index(f, v) + 1
        assert k < int(f.ptr[v + 1]) - 1                # an entry below the diagonal in the column of v
        bad[k] = np.nan
    elif what == "nan-diag":
        bad[_diag_index(f, v)] = np.nan
    else:
        bad[_diag_index(f, v)] = np.inf
    o, rc = oracle_factor(f, val)
    assert rc == 0
    # the broken values as the first factorization of the handle and again behind a clean one (flags 32768: the
    # capture of the graph, then a replay of it); the factorization after each is clean
    for _ in range(2):
        _expect_not_posdef(f, bad, what)
        got = f.factor(val).wait().get_factor()
        assert rel_err(got, o.arena(), lower_mask(f)) <= TOL_L
    assert f.factor_batch(np.stack([val, bad])) == -20
    flags_b, cols = f.batch_status()
    assert flags_b.tolist() == [0, -20]
    if what != "nan-offdiag":
        assert cols.tolist() == [0, p + 1]
    f.close()
