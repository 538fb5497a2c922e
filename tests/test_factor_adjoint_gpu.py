"""GPU tests of the factor adjoint (spllt_hip_factor_adjoint and friends, SparseCholesky.factor_apply / rsample):
the sweep against the dense formula and against the numpy interpretation of the same program
(tests/factor_adjoint_emulate.py) on the GPU's own L, the seed kernel against its fma chain, the states of the
adjoint arena, and the PyTorch operations against gradcheck and dense CPU autograd."""
import functools

import numpy as np
import pytest
import scipy.linalg as sl
import scipy.sparse as sp

import factor_adjoint_emulate as fe
from helpers import bwd_err, lower_mask, make_case
from selinv_emulate import panel_inverses
from spllt_amd import api, matgen

pytestmark = pytest.mark.gpu

# The error bar of every comparison with a dense reference: 100 x e_max, e_max = 4.45e-15 the largest relative
# error of the numpy interpretation of the sweep against the dense computation over the cases and seeds of
# tests/test_factor_adjoint_cpu.py::test_emulated_sweep_matches_the_dense_formula (p2d64-nb100-pw32, the seed
# of log det against (2 - delta) inv(A)).  The factor 100 is for what the interpreter does not have: sums in
# MFMA order and the inverted panels of the factorization.  The reference is the dense computation, never the
# code under test.
E_MAX = 4.45e-15
B = 100 * E_MAX
assert B <= 1e-11          # the bar of the selected inversion against the dense inverse

U53 = 2.0 ** -53
IDS = [c[0] for c in fe.CASES]


@functools.lru_cache(maxsize=None)
def _case(name):
    """the factorized handle of a case and its dense references: built once, shared, never modified (a test that
    factorizes other values makes its own handle)"""
    _, gen, nb, nemin, pw = fe.CASES[IDS.index(name)]
    A = gen()
    f, val = make_case(A, nb=nb, nemin=nemin, panel_width=pw)
    f.factor(val).wait()
    mask = lower_mask(f)
    rng = np.random.default_rng(17)
    lbar = np.where(mask, rng.standard_normal(mask.shape), np.nan)      # NaN where nothing may be read
    return dict(A=A, f=f, val=val, mask=mask, lbar=lbar)


@functools.lru_cache(maxsize=None)
def _dense_factor(name):
    c = _case(name)
    return sl.cholesky(fe.pivot_matrix(c["f"], c["A"]), lower=True)


def _porder(f):
    p = np.empty(f.n, dtype=np.int64)
    p[f.sym("order")] = np.arange(f.n)
    return p


# ---- 1. the sweep -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", IDS)
def test_sweep_matches_dense_formula_and_emulator(name):
    c = _case(name)
    f, mask, lbar = c["f"], c["mask"], c["lbar"]
    f.set_factor_adjoint(lbar)
    assert np.array_equal(f.get_factor_adjoint()[mask], lbar[mask])
    gval = f.factor_adjoint()
    G = f.get_factor_adjoint()
    assert np.isfinite(G[mask]).all()
    e_dense = fe.rel(G, fe.dense_factor_adjoint(f, _dense_factor(name), np.where(mask, lbar, 0.0)), mask)
    L = f.get_factor()
    e_emul = fe.rel(G, fe.emulate_factor_adjoint(f, L, panel_inverses(f, L), lbar), mask)
    print(f"{name}: against dense {e_dense:.2e}, against the emulator {e_emul:.2e}, B = {B:.2e}")
    assert e_dense <= B, e_dense
    assert e_emul <= B, e_emul
    assert np.array_equal(gval, fe.on_pattern(f, G))


# ---- 2. the seed of log det ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", IDS)
def test_logdet_seed_gives_the_weighted_selected_inverse(name):
    c = _case(name)
    f, mask = c["f"], c["mask"]
    f.set_factor_adjoint(fe.logdet_seed(f, f.get_factor()))
    gval = f.factor_adjoint()
    G = f.get_factor_adjoint()
    f.selected_inverse()
    weight = np.full(mask.shape, 2.0)
    weight[f.program("selinv_diag")] = 1.0
    e_arena = fe.rel(G, weight * f.get_inverse(), mask)
    prow, pcol = f.pattern_tables()
    want = np.where(prow == pcol, 1.0, 2.0) * f.inverse_on_pattern()
    e_pat = float(np.abs(gval - want).max() / np.abs(want).max())
    print(f"{name}: arena {e_arena:.2e}, pattern {e_pat:.2e}, B = {B:.2e}")
    assert e_arena <= B, e_arena
    assert e_pat <= B, e_pat


# ---- 3. the seed kernel ------------------------------------------------------------------------------------
def _arena_ld(f, M):
    out = np.zeros(f.sym_info()["arena"], dtype=np.longdouble)
    for off, nr, w, rows, cols in fe._blocks(f):
        out[off:off + nr * w] = M[np.ix_(rows, cols)].ravel()
    return out


def _seed_dev(f, a, b, alpha, accumulate, flags, pad=0):
    """a, b: (n, nvec) host arrays -> spllt_hip_factor_adjoint_seed_dev with ld = n + pad, NaN in the padding"""
    import torch
    n, nvec = a.shape
    bufs = []
    for v in (a, b):
        t = torch.full((max(nvec, 1), n + pad), float("nan"), dtype=torch.float64, device="cuda")
        t[:nvec, :n] = torch.as_tensor(np.ascontiguousarray(v.T))
        bufs.append(t)
    torch.cuda.synchronize()
    f.factor_adjoint_seed_dev(bufs[0].data_ptr(), bufs[1].data_ptr(), nvec, ld=n + pad, alpha=alpha,
                              accumulate=accumulate, a_pivot_order=bool(flags & 1), b_pivot_order=bool(flags & 2))
    return f.get_factor_adjoint().copy()


@pytest.mark.parametrize("name", ["p2d16-nb8-pw32", "box8-nb96"])
@pytest.mark.parametrize("nvec", [1, 4, 5, 33])
def test_seed_meets_the_rounding_bound_of_its_fma_chain(name, nvec):
    """Per lower position the kernel computes acc_0 = 0, acc_q = fma(a_q, b_q, acc_{q-1}), q ascending, and stores
    alpha * acc (+ the old value): every product reaches alpha * acc through at most nvec + 1 roundings, gamma_{nvec
    + 1} <= (nvec + 3/2) u, plus u / 2 per unit for the long-double reference, as in
    test_pattern_outer_meets_the_rounding_bound_of_its_fma_chain: (nvec + 2) u |alpha| sum |a_q b_q|; the sum with
    the old value rounds once more, u (|old| + |alpha sum|) at the most."""
    c = _case(name)
    f, mask = c["f"], c["mask"]
    n, por = f.n, _porder(f)
    rng = np.random.default_rng(100 + nvec)
    for flags in range(4):
        a, b = rng.standard_normal((n, nvec)), rng.standard_normal((n, nvec))
        alpha = -0.37 if flags & 1 else 1.7
        ap = (a if flags & 1 else a[por]).astype(np.longdouble)        # pivot order: x_pivot[p] = x_user[porder[p]]
        bp = (b if flags & 2 else b[por]).astype(np.longdouble)
        ref = _arena_ld(f, np.longdouble(alpha) * (ap @ bp.T))
        mag = _arena_ld(f, abs(alpha) * (np.abs(ap) @ np.abs(bp).T))
        bar = (nvec + 2) * np.longdouble(U53) * mag
        got = _seed_dev(f, a, b, alpha, False, flags, pad=3 * flags)
        err = np.abs(got.astype(np.longdouble) - ref)
        worst = float((err[mask] / np.maximum(bar[mask], np.longdouble(1e-300))).max())
        print(f"{name} nvec={nvec} flags={flags}: max err / bar = {worst:.3f}")
        assert (err[mask] <= bar[mask]).all(), (flags, worst)
        # the host entry point runs the same chain
        f.factor_adjoint_seed(a, b, alpha=alpha, a_pivot_order=bool(flags & 1), b_pivot_order=bool(flags & 2))
        assert np.array_equal(f.get_factor_adjoint()[mask], got[mask])
        # accumulate: the same chain on top of what is there
        got2 = _seed_dev(f, b, a, 0.5, True, flags ^ 3 if flags in (1, 2) else flags)
        ref2 = got.astype(np.longdouble) + _arena_ld(f, np.longdouble(0.5) * (bp @ ap.T))
        bar2 = (nvec + 2) * np.longdouble(U53) * 0.5 * _arena_ld(f, np.abs(bp) @ np.abs(ap).T) \
            + np.longdouble(U53) * (np.abs(got) + np.abs(ref2 - got))
        err2 = np.abs(got2.astype(np.longdouble) - ref2)
        assert (err2[mask] <= bar2[mask]).all(), flags


def test_seed_is_bit_identical_across_calls_and_group_positions_and_zeroes_for_no_vectors():
    c = _case("box8-nb96")
    f, mask = c["f"], c["mask"]
    n = f.n
    rng = np.random.default_rng(3)
    a, b = rng.standard_normal((n, 33)), rng.standard_normal((n, 33))
    g0 = _seed_dev(f, a, b, -1.0, False, 0)
    assert np.array_equal(g0[mask], _seed_dev(f, a, b, -1.0, False, 0)[mask])
    assert np.array_equal(g0[mask], _seed_dev(f, a, b, -1.0, False, 0, pad=11)[mask])   # another leading dimension
    # one vector alone and at places 0, 31 and 32 of a group of 33 whose other vectors are zero
    alone = _seed_dev(f, a[:, :1], b[:, :1], 0.7, False, 3)
    for place in (0, 31, 32):
        az, bz = np.zeros((n, 33)), np.zeros((n, 33))
        az[:, place], bz[:, place] = a[:, 0], b[:, 0]
        assert np.array_equal(alone[mask], _seed_dev(f, az, bz, 0.7, False, 3)[mask]), place
    # vectors 32 .. (the second pass of the kernel) added by a second call: the chain restarts, so only the bound
    # holds there -- but the first 32 alone are the chain's first 32 links
    first = _seed_dev(f, a[:, :32], b[:, :32], -1.0, False, 0)
    chain = _seed_dev(f, np.hstack([a[:, :32], np.zeros((n, 1))]), np.hstack([b[:, :32], np.zeros((n, 1))]), -1.0,
                      False, 0)
    assert np.array_equal(first[mask], chain[mask])
    # no vectors: the arena is zeroed (the arrays are not read, but their addresses must not be null)
    z = _seed_dev(f, a[:, :0], b[:, :0], 2.0, False, 0)
    assert (z[mask] == 0.0).all()


# ---- 4. reproducibility ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [fe.KSLICE_CASE, "box11-nb100-pw48"])
def test_two_seeded_sweeps_are_bit_identical(name):
    c = _case(name)
    f, mask = c["f"], c["mask"]
    if name == fe.KSLICE_CASE:
        assert (f.program("selinv_units")["nsplit"] >= 2).any()
    rng = np.random.default_rng(8)
    a, b = rng.standard_normal((f.n, 5)), rng.standard_normal((f.n, 5))
    runs = []
    for _ in range(2):
        f.factor_adjoint_seed(a, b, alpha=0.3)
        f.factor_adjoint_seed(b, a, alpha=-1.1, accumulate=True, b_pivot_order=True)
        gval = f.factor_adjoint()
        runs.append((gval, f.get_factor_adjoint().copy()))
    assert np.array_equal(runs[0][0], runs[1][0])
    assert np.array_equal(runs[0][1][mask], runs[1][1][mask])


# ---- 5. states ---------------------------------------------------------------------------------------------------
def test_states_of_the_adjoint_arena():
    A = matgen.poisson2d(20)
    f, val = make_case(A, nb=16, nemin=8)
    v = np.ones(f.n)

    def refused(call, word):
        with pytest.raises(api.SplltError) as ei:
            call()
        assert ei.value.flag == -10 and word in f.last_error(), f.last_error()

    refused(lambda: f.factor_adjoint_seed(v, v), "factorized")
    f.factor(val).wait()
    refused(f.factor_adjoint, "seeded")                                   # unseeded
    refused(f.get_factor_adjoint, "seed")
    refused(lambda: f.factor_adjoint_seed(v, v, accumulate=True), "seeded")
    assert not f.device_factor_adjoint_ptr()
    mask = lower_mask(f)
    rng = np.random.default_rng(2)
    lbar = np.where(mask, rng.standard_normal(mask.shape), 0.0)
    b = A @ rng.standard_normal(f.n)
    x0 = f.solve(b)
    f.selected_inverse()
    Z0 = f.get_inverse().copy()
    f.set_factor_adjoint(lbar)
    assert f.device_factor_adjoint_ptr()
    g1 = f.factor_adjoint()
    refused(f.factor_adjoint, "swept")                                    # a second sweep
    refused(lambda: f.factor_adjoint_seed(v, v, accumulate=True), "swept")
    # the solve and the selected inverse have not noticed
    assert np.array_equal(f.get_inverse(), Z0)
    assert np.array_equal(f.solve(b), x0) or bwd_err(A, f.solve(b), b) <= 1e-14
    f.selected_inverse()
    assert np.array_equal(f.get_inverse(), Z0)
    # the inverse released while the adjoint arena is resident: the shared scratch stays
    f.release_inverse()
    f.set_factor_adjoint(lbar)
    assert np.array_equal(f.factor_adjoint(), g1)
    # a new factorization makes the arena stale
    A2 = A + sp.identity(A.shape[0]) * 0.5
    val2 = api.csc_lower_1based(A2)[3]
    f.factor(val2).wait()
    refused(f.get_factor_adjoint, "seed")
    refused(f.factor_adjoint, "seeded")
    refused(lambda: f.factor_adjoint_seed(v, v, accumulate=True), "seeded")
    f.set_factor_adjoint(lbar)
    f.factor_adjoint()
    Ld = sl.cholesky(fe.pivot_matrix(f, A2), lower=True)
    assert fe.rel(f.get_factor_adjoint(), fe.dense_factor_adjoint(f, Ld, lbar), mask) <= B
    # release, then again from scratch
    f.release_factor_adjoint()
    refused(f.get_factor_adjoint, "seed")
    refused(f.factor_adjoint, "seeded")
    f.set_factor_adjoint(lbar)
    f.factor_adjoint()
    assert bwd_err(A2, f.solve(b), b) <= 1e-14
    f.close()


def test_partitioned_factor_returns_unimplemented_after_factor():
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
    v = np.ones(A.shape[0])
    for f in fs:
        f.wait()
        for call in (lambda: f.factor_adjoint_seed(v, v), f.factor_adjoint):
            with pytest.raises(api.SplltError) as ei:
                call()
            assert ei.value.flag == -98 and "partitioned" in f.last_error()
    for f in fs:
        f.close()


# ---- 6. torch: gradcheck ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _small_chol():
    import torch
    import spllt_amd
    A = matgen.poisson2d(6)
    n, ptr, row, val = api.csc_lower_1based(A)
    chol = spllt_amd.SparseCholesky(A, nb=16, nemin=4, reproducible=True)
    return chol, torch.tensor(val, device="cuda", requires_grad=True), n


@pytest.mark.parametrize("shape", ["matrix", "vector"])
@pytest.mark.parametrize("op", ["L", "Lt", "Linv", "Ltinv"])
def test_gradcheck_of_factor_apply(op, shape):
    """default eps, atol, rtol and nondet_tol = 0; v.clone() as in test_gradcheck_of_solve_and_logdet"""
    import torch
    chol, tv, n = _small_chol()
    rng = np.random.default_rng(6)
    x = rng.standard_normal((n, 3) if shape == "matrix" else n)
    tx = torch.tensor(x, device="cuda", requires_grad=True)
    assert torch.autograd.gradcheck(lambda v, X: chol.factor_apply(v.clone(), X, op), (tv, tx), nondet_tol=0.0)


@pytest.mark.parametrize("with_mean", [False, True])
@pytest.mark.parametrize("kind", ["precision", "covariance"])
def test_gradcheck_of_rsample(kind, with_mean):
    import torch
    chol, tv, n = _small_chol()
    if with_mean:
        tm = torch.tensor(np.random.default_rng(9).standard_normal(n), device="cuda", requires_grad=True)
        assert torch.autograd.gradcheck(lambda v, m: chol.rsample(v.clone(), 3, seed=5, kind=kind, mean=m), (tv, tm),
                                        nondet_tol=0.0)
    else:
        assert torch.autograd.gradcheck(lambda v: chol.rsample(v.clone(), 3, seed=5, kind=kind), (tv,), nondet_tol=0.0)


# ---- 7. torch: identities ----------------------------------------------------------------------------------------
def _torch_case(name, **kw):
    import torch
    from spllt_amd.torch_ops import SparseCholesky
    _, gen, nb, nemin, pw = fe.CASES[IDS.index(name)]
    A = gen()
    val = api.csc_lower_1based(A)[3]
    extra = {} if pw is None else {"panel_width": pw}
    chol = SparseCholesky(A, nb=nb, nemin=nemin, reproducible=True, **extra, **kw)
    return torch, A, chol, torch.tensor(val, device="cuda", requires_grad=True)


@pytest.mark.parametrize("name", ["p2d32-nb16", "box8-nb96"])
def test_rsample_equals_sample_and_matches_dense_autograd(name):
    """nsamp = 40: two seed groups.  The reference: torch CPU autograd through torch.linalg.cholesky of the dense
    P A P^T, x = mean + P^T L^-T z or mean + P^T L z with the z that white_noise_dev writes"""
    torch, A, chol, tv = _torch_case(name)
    n, ns = chol.n, 40
    rng = np.random.default_rng(21)
    tm = torch.tensor(rng.standard_normal(n), device="cuda", requires_grad=True)
    W = rng.standard_normal((n, ns))
    prow, pcol = (torch.as_tensor(np.asarray(v, dtype=np.int64)) for v in chol.f.pattern_tables())
    order = torch.as_tensor(np.asarray(chol.f.sym("order"), dtype=np.int64))
    por = torch.as_tensor(_porder(chol.f))
    for kind in ("precision", "covariance"):
        x = chol.rsample(tv, ns, seed=7, kind=kind, mean=tm)
        assert torch.equal(x.detach(), chol.sample(tv, ns, seed=7, kind=kind, mean=tm).detach())
        assert torch.equal(chol.rsample(tv, ns, seed=7, kind=kind).detach(), chol.sample(tv, ns, seed=7, kind=kind))
        tv.grad = tm.grad = None
        (x * torch.as_tensor(W, device="cuda")).sum().backward()
        z = torch.as_tensor(np.ascontiguousarray(chol.f.white_noise(ns, seed=7)))        # (n, ns), pivot order
        cv = tv.detach().cpu().requires_grad_(True)
        cm = tm.detach().cpu().requires_grad_(True)
        Ad = torch.zeros((n, n), dtype=torch.float64).index_put((prow, pcol), cv).index_put((pcol, prow), cv)
        Lt = torch.linalg.cholesky(Ad[por][:, por])
        y = torch.linalg.solve_triangular(Lt.T, z, upper=True) if kind == "precision" else Lt @ z
        xr = y[order] + cm[:, None]                                                        # x_user[i] = y[order[i]]
        (xr * torch.as_tensor(W)).sum().backward()
        e_x = float((x.detach().cpu() - xr.detach()).abs().max() / xr.detach().abs().max())
        e_v = float((tv.grad.cpu() - cv.grad).abs().max() / cv.grad.abs().max())
        e_m = float((tm.grad.cpu() - cm.grad).abs().max() / cm.grad.abs().max())
        print(f"{name} {kind}: sample {e_x:.2e}, val gradient {e_v:.2e}, mean gradient {e_m:.2e}, B = {B:.2e}")
        assert e_v <= B, (kind, e_v)
        assert e_m <= B, (kind, e_m)
    chol.close()


def test_factor_apply_round_trip_has_no_gradient_to_val():
    torch, A, chol, tv = _torch_case("box8-nb96")
    n = chol.n
    rng = np.random.default_rng(4)
    X = torch.tensor(rng.standard_normal((n, 5)), device="cuda", requires_grad=True)
    Wt = torch.as_tensor(rng.standard_normal((n, 5)), device="cuda")
    (chol.factor_apply(tv, X, "L") * Wt).sum().backward()
    scale = float(tv.grad.abs().max())             # the gradient of one of the two operations alone
    tv.grad = X.grad = None
    Y = chol.factor_apply(tv, chol.factor_apply(tv, X, "L"), "Linv")
    e_y = float((Y.detach() - X.detach()).abs().max() / X.detach().abs().max())
    (Y * Wt).sum().backward()
    e_v = float(tv.grad.abs().max()) / scale
    e_x = float((X.grad - Wt).abs().max() / Wt.abs().max())
    print(f"round trip: Y {e_y:.2e}, val gradient / one operation's {e_v:.2e}, X gradient {e_x:.2e}, B = {B:.2e}")
    assert e_y <= B and e_x <= B
    assert e_v <= B, e_v
    chol.close()


def test_torch_errors_are_raised_before_any_library_call():
    torch, A, chol, tv = _torch_case("p2d12-nb4")
    n = chol.n
    X = torch.zeros((n, 2), dtype=torch.float64, device="cuda")
    serial = chol.f.factor_serial(0)
    with pytest.raises(ValueError):
        chol.factor_apply(tv, X, "LLt")
    with pytest.raises(TypeError):
        chol.factor_apply(tv.float(), X, "L")
    with pytest.raises(TypeError):
        chol.factor_apply(tv, X.float(), "L")
    with pytest.raises(ValueError):
        chol.factor_apply(tv.cpu(), X, "L")
    with pytest.raises(ValueError):
        chol.factor_apply(tv, X[:-1], "L")
    with pytest.raises(ValueError):
        chol.factor_apply(tv[:-1], X, "Linv")
    with pytest.raises(TypeError):
        chol.rsample(tv.float(), 2)
    with pytest.raises(ValueError):
        chol.rsample(tv, 2, mean=X[:, 0].cpu())
    with pytest.raises(ValueError):
        chol.rsample(tv, 2, mean=X[:-1, 0])
    with pytest.raises(ValueError):
        chol.rsample(tv, 2, kind="variance")
    assert chol.f.factor_serial(0) == serial and chol.device is None      # nothing has reached the library
    chol.close()
