"""GPU tests of the batch's factor adjoint (include/spllt_hip_batch_adjoint.h) and of the PyTorch operations on it.

References: the dense formula on a LAPACK factor of P A_b P^T, and the numpy interpreter of
tests/factor_adjoint_emulate.py on the batch tables with the GPU's own L_b -- never the code under test.  The bar is
B = 100 e_max, e_max the error of the interpreter against the dense formula measured by
tests/test_batch_adjoint_cpu.py (batch_adjoint_emulate.E_MAX): the factor 100 is for what the interpreter lacks,
the summation order of the matrix cores and the inverted panels of the batch factorization.

Across two factorizations: the batch factorization adds its updates with fp64 atomics, so
two spllt_hip_factor_batch calls on the same values need not leave the same bits in L_b, and the sweep is a function
of those bits.  Where a test has to compare sweeps across two factorizations (a member alone against inside a batch,
the two grid mappings, a batch with and without a failed member) it therefore reads both factors back: the sweeps
have to agree bit for bit when the factors do, and to B otherwise (_same_bits_or_close prints which it was).  What
does not need a second factorization is asserted bit for bit without condition: the other members' seeds, a
member-range split down to ONE member per launch, two sweeps of one batch.  On the cases here the two
factorizations differed in bits every time, so the conditional bit-for-bit branch hardly ever runs: the real
"a member alone" check is the run with batch_grid_limit=1, in which every kernel of the sweep and the reader is
launched per member and sees nbatch = 1, on the SAME factor bits as the whole-batch run it is compared with.

Shapes: the smallest of factor_adjoint_emulate.CASES at which each path can go wrong (every step fused with panels
narrower than 64; fused and three-launch steps mixed; ragged panels with 3 K slices; 4 K slices and block columns
of several 64-panels), three members."""
import functools

import numpy as np
import pytest

import batch_adjoint_emulate as be
import batch_adjoint_ladder as ladder
import capi_ladder
import factor_adjoint_emulate as fe
from helpers import make_case
from selinv_emulate import panel_inverses
from spllt_amd import _lib, api, matgen

pytestmark = pytest.mark.gpu

B = be.GPU_BAR
assert B <= 1e-11
U53 = 2.0 ** -53
NB = 3
SWEEP_CASES = ["p2d12-nb4", "p2d32-nb16", "box11-nb100-pw48", "box12-nb256"]


@pytest.fixture(autouse=True)
def _default_hooks():
    """After every test both process-wide hooks are back at their defaults (fused steps off, the hardware grid
    limit).  The C boundary has no getter for either, so "the previous setting" cannot be read and put back; every
    test of the suite starts from the defaults and no other test file changes batch_fadj_fused."""
    yield
    lib = _lib.load()
    lib.spllt_hip_debug(b"batch_fadj_fused=0")     # (the default: what every test found)
    lib.spllt_hip_debug(b"batch_grid_limit=0")


def _fused(f, on):
    assert f.lib.spllt_hip_debug(b"batch_fadj_fused=1" if on else b"batch_fadj_fused=0") == 0


def _values(name, members=range(NB)):
    return np.stack([be.member(name, b)["val"] for b in members])


@functools.lru_cache(maxsize=None)
def _seeds(name):
    """a random Lbar per member, NaN off the lower pattern (what is never read)"""
    c = be.case(name)
    return tuple(np.where(c["mask"], np.random.default_rng(900 + b).standard_normal(c["mask"].shape), np.nan)
                 for b in range(NB))


@functools.lru_cache(maxsize=None)
def _dense_ref(name, b):
    c, m = be.case(name), be.member(name, b)
    return fe.dense_factor_adjoint(c["f"], m["Ld"], np.nan_to_num(_seeds(name)[b]))


def _sweep(name, fused, members=range(NB), seeds=None, factor=True):
    """factor the members, upload their seeds, sweep: (gval, [G_b], launches)"""
    f = be.case(name)["f"]
    if factor:
        assert f.factor_batch(_values(name, members)) == 0
    _fused(f, fused)
    f.set_factor_adjoint_batch(np.stack(seeds if seeds is not None else [_seeds(name)[b] for b in members]))
    gval = f.factor_adjoint_batch()
    return gval, [f.get_factor_adjoint_batch(i).copy() for i in range(len(members))], f.batch_adjoint_launches()


def _factors(f, n):
    return [f.get_factor_batch(b).copy() for b in range(n)]


def _same_bits_or_close(what, La, Lb, Xa, Xb, mask=None):
    """sweeps Xa, Xb of the factors La, Lb (two factorizations of the same values): see the module docstring"""
    sel = (lambda v: v[mask]) if mask is not None and Xa.shape == mask.shape else (lambda v: v)
    if np.array_equal(La, Lb):
        print(f"{what}: the factors agree bit for bit, so must the sweeps")
        assert np.array_equal(sel(Xa), sel(Xb)), what
    else:
        e = float(np.abs(sel(Xa) - sel(Xb)).max() / np.abs(sel(Xb)).max())
        print(f"{what}: the two factorizations differ in the last bits (atomic adds), sweeps agree to {e:.2e}")
        assert e <= B, (what, e)


def _check_member(name, b, G, what):
    c = be.case(name)
    f, mask = c["f"], c["mask"]
    assert np.isfinite(G[mask]).all(), (what, b)
    e_dense = fe.rel(G, _dense_ref(name, b), mask)
    L = f.get_factor_batch(b)
    emu = fe.emulate_factor_adjoint(f, L, panel_inverses(f, L, c["t"]), np.nan_to_num(_seeds(name)[b]), c["t"])
    e_emu = fe.rel(G, emu, mask)
    print(f"{name} {what} member {b}: vs dense {e_dense:.2e}, vs interpreter {e_emu:.2e} (bar {B:.1e})")
    assert e_dense <= B, (what, b, e_dense)
    assert e_emu <= B, (what, b, e_emu)


# ---- 1, 2: the sweep of an uploaded seed, fused and in the three-launch form ----------------------------
@pytest.mark.parametrize("name", SWEEP_CASES)
def test_sweep_of_an_uploaded_seed_in_both_forms(name):
    c = be.case(name)
    f, mask, t = c["f"], c["mask"], c["t"]
    gv1, G1, n1 = _sweep(name, True)
    for b in range(NB):
        _check_member(name, b, G1[b], "fused")
        assert np.array_equal(gv1[b], fe.on_pattern(f, G1[b]))
    gv0, G0, n0 = _sweep(name, False, factor=False)
    for b in range(NB):
        _check_member(name, b, G0[b], "three-launch")
        assert np.array_equal(gv0[b], fe.on_pattern(f, G0[b]))
        e = fe.rel(G1[b], G0[b], mask)
        print(f"{name} member {b}: fused vs three-launch {e:.2e}")
        assert e <= B
    print(f"{name}: launches fused {n1}, three-launch {n0}")
    assert n1 == be.expected_launches(t, True) and n0 == be.expected_launches(t, False)
    if name == "p2d12-nb4":
        assert n1 < n0, "the fused kernel did not run"
    if name in ("box11-nb100-pw48", "box12-nb256"):
        assert int(t["units"]["nsplit"].max()) >= 3 and n1 < n0


# ---- 3: the seed of log det ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["p2d32-nb16", "box11-nb100-pw48"])
def test_logdet_seed_gives_the_selected_inverse(name):
    c = be.case(name)
    f, mask = c["f"], c["mask"]
    assert f.factor_batch(_values(name)) == 0
    assert f.selected_inverse_batch() == 0
    Z = [f.get_inverse_batch(b).copy() for b in range(NB)]
    zp = f.inverse_on_pattern_batch()
    seeds = [fe.logdet_seed(f, f.get_factor_batch(b)) for b in range(NB)]
    f.set_factor_adjoint_batch(np.stack(seeds))
    f.factor_adjoint_batch()
    w = be.logdet_weight(f)
    for b in range(NB):
        e = fe.rel(f.get_factor_adjoint_batch(b), w * Z[b], mask)
        print(f"{name} member {b}: log-det seed against (2 - delta) Z_b {e:.2e}")
        assert e <= B
        assert np.array_equal(f.get_inverse_batch(b)[mask], Z[b][mask]), "the adjoint run changed Z"
    assert np.array_equal(f.inverse_on_pattern_batch(), zp)


# ---- 4: the seed kernel ------------------------------------------------------------------------------------
def _dev(x):
    import torch
    return torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device="cuda")


def _arena_ld(f, M):
    """M (n x n, pivot order, long double) at L's arena positions, in long double"""
    out = np.zeros(f.sym_info()["arena"], dtype=np.longdouble)
    for off, nr, w, rows, cols in fe._blocks(f):
        out[off:off + nr * w] = M[np.ix_(rows, cols)].ravel()
    return out


def _pivot_ld(x, pivot, por_inv):
    """(nvec, n) -> (n, nvec) in pivot order, long double"""
    return (x if pivot else x[:, por_inv]).T.astype(np.longdouble)


def _single_seed(f, a, b, alpha, accumulate=False, flags=0):
    """the single handle's seed of one member's vectors a, b (nvec, n)"""
    import torch
    ta, tb = _dev(a), _dev(b)
    torch.cuda.synchronize()
    f.factor_adjoint_seed_dev(ta.data_ptr(), tb.data_ptr(), a.shape[0], ld=f.n, alpha=alpha, accumulate=accumulate,
                              a_pivot_order=bool(flags & 1), b_pivot_order=bool(flags & 2))
    return f.get_factor_adjoint().copy()


def _batch_seed(f, a, b, alpha, accumulate=False, flags=0):
    """a, b: (nbatch, nvec, n)"""
    import torch
    ta, tb = _dev(a), _dev(b)
    torch.cuda.synchronize()
    f.factor_adjoint_seed_batch_dev(ta.data_ptr(), tb.data_ptr(), a.shape[1], ld=f.n, alpha=alpha, accumulate=accumulate,
                                    a_pivot_order=bool(flags & 1), b_pivot_order=bool(flags & 2))
    return [f.get_factor_adjoint_batch(m).copy() for m in range(a.shape[0])]


@pytest.mark.parametrize("nvec,flags", [(1, 0), (33, 1), (70, 2), (5, 3)])
def test_seed_kernel_writes_the_bits_of_the_single_handle(nvec, flags):
    name = "p2d32-nb16"
    c = be.case(name)
    f, mask, n = c["f"], c["mask"], c["f"].n
    f.factor(be.member(name, 0)["val"]).wait()            # (the single seed wants a factor; it does not read it)
    assert f.factor_batch(_values(name)) == 0
    rng = np.random.default_rng(40 + nvec)
    a, b = rng.standard_normal((NB, nvec, n)), rng.standard_normal((NB, nvec, n))
    alpha = -0.7
    got = _batch_seed(f, a, b, alpha, flags=flags)
    por = f.sym("order")
    por_inv = np.empty(n, dtype=np.int64)
    por_inv[por] = np.arange(n)
    for m in range(NB):
        want = _single_seed(f, a[m], b[m], alpha, flags=flags)
        assert np.array_equal(got[m][mask], want[mask]), (nvec, flags, m)
        # the rounding bound of one fma chain with alpha applied once, (nvec + 2) u |alpha| sum |a b| (DESIGN.md
        # section 19); reference, magnitude and error stay in long double as in tests/test_factor_adjoint_gpu.py
        ap, bp = _pivot_ld(a[m], flags & 1, por_inv), _pivot_ld(b[m], flags & 2, por_inv)
        ref = _arena_ld(f, np.longdouble(alpha) * (ap @ bp.T))
        bar = (nvec + 2) * np.longdouble(U53) * _arena_ld(f, abs(alpha) * (np.abs(ap) @ np.abs(bp).T))
        err = np.abs(got[m].astype(np.longdouble) - ref)
        assert (err[mask] <= bar[mask]).all(), (nvec, flags, m)
    if nvec == 70:
        # two groups with accumulate: the bits of the single handle's two groups, and section 19's bound of an
        # accumulating seed on top of what the first group left: (nvec2 + 2) u |alpha| sum |a b| of the second
        # group, plus one rounding u (|old| + |alpha sum|) of the sum with the old value
        one = _batch_seed(f, a[:, :40], b[:, :40], alpha, flags=flags)
        two = _batch_seed(f, a[:, 40:], b[:, 40:], alpha, accumulate=True, flags=flags)
        for m in range(NB):
            _single_seed(f, a[m, :40], b[m, :40], alpha, flags=flags)
            want = _single_seed(f, a[m, 40:], b[m, 40:], alpha, accumulate=True, flags=flags)
            assert np.array_equal(two[m][mask], want[mask])
            ap, bp = _pivot_ld(a[m, 40:], flags & 1, por_inv), _pivot_ld(b[m, 40:], flags & 2, por_inv)
            old = one[m].astype(np.longdouble)
            ref2 = old + _arena_ld(f, np.longdouble(alpha) * (ap @ bp.T))
            bar2 = (nvec - 40 + 2) * np.longdouble(U53) * _arena_ld(f, abs(alpha) * (np.abs(ap) @ np.abs(bp).T)) \
                + np.longdouble(U53) * (np.abs(old) + np.abs(ref2 - old))
            err2 = np.abs(two[m].astype(np.longdouble) - ref2)
            assert (err2[mask] <= bar2[mask]).all(), (flags, m)
        # the host entry point: groups of 32 per member, each one such call
        f.factor_adjoint_seed_batch(a, b, alpha=alpha, a_pivot_order=bool(flags & 1), b_pivot_order=bool(flags & 2))
        host = [f.get_factor_adjoint_batch(m).copy() for m in range(NB)]
        for q in range(0, nvec, 32):
            grp = _batch_seed(f, a[:, q:q + 32], b[:, q:q + 32], alpha, accumulate=q > 0, flags=flags)
        for m in range(NB):
            assert np.array_equal(host[m][mask], grp[m][mask])
    if nvec == 1:
        zero = np.zeros((NB, 0, n))
        f.factor_adjoint_seed_batch(zero, zero)
        for m in range(NB):
            assert (f.get_factor_adjoint_batch(m)[mask] == 0.0).all()




# ---- 5: bit reproducibility ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["p2d32-nb16", fe.KSLICE_CASE])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "three-launch"])
def test_a_members_bits_depend_on_nothing_but_the_member(name, fused):
    c = be.case(name)
    f, mask, t = c["f"], c["mask"], c["t"]
    gv, G, whole = _sweep(name, fused)
    L3 = _factors(f, NB)
    gv2, G2, _ = _sweep(name, fused, factor=False)
    assert np.array_equal(gv, gv2) and all(np.array_equal(x[mask], y[mask]) for x, y in zip(G, G2))
    # other seeds for the other members
    other = [_seeds(name)[1] * 3.0, _seeds(name)[1], _seeds(name)[0] - 1.0]
    _, G3, _ = _sweep(name, fused, seeds=other, factor=False)
    assert np.array_equal(G3[1][mask], G[1][mask])
    # a member-range split: at most two members per launch, then ONE (every kernel sees nbatch = 1: a member alone)
    biggest = int(t["launches"][:, 3].max())
    for limit in (2 * biggest, 1):
        assert f.lib.spllt_hip_debug(("batch_grid_limit=%d" % limit).encode()) == 0
        try:
            gvs, Gs, split = _sweep(name, fused, factor=False)
        finally:
            assert f.lib.spllt_hip_debug(b"batch_grid_limit=0") == 0
        assert split > whole
        assert np.array_equal(gvs, gv) and all(np.array_equal(x[mask], y[mask]) for x, y in zip(Gs, G))
    assert split == NB * whole
    # member 1 alone: a batch of one (a second factorization)
    gva, Ga, alone = _sweep(name, fused, members=[1])
    assert alone == whole, "the number of launches depends on nbatch"
    L1 = _factors(f, 1)[0]
    _same_bits_or_close(f"{name} member 1 alone, gval", L1, L3[1], gva[0], gv[1])
    _same_bits_or_close(f"{name} member 1 alone, arena", L1, L3[1], Ga[0], G[1], mask)


@pytest.mark.parametrize("fast", ["0", "1"])
def test_both_grid_mappings_give_the_same_bits(fast, monkeypatch):
    name = "box11-nb100-pw48"
    gv, G, _ = _sweep(name, True)
    L = _factors(be.case(name)["f"], NB)
    monkeypatch.setenv("SPLLT_BATCH_MEMBER_FAST", fast)
    _, gen, nb, nemin, pw = fe.CASES[be.IDS.index(name)]
    f2, _ = make_case(gen(), nb=nb, nemin=nemin, panel_width=be.handle_panel_width(pw))   # (read at the first batch)
    mask = be.case(name)["mask"]
    for on in (True, False):
        assert f2.factor_batch(_values(name)) == 0
        _fused(f2, on)
        f2.set_factor_adjoint_batch(np.stack(_seeds(name)))
        gv2 = f2.factor_adjoint_batch()
        L2 = _factors(f2, NB)
        for b in range(NB):        # (the two forms give the same bits: test_sweep_of_an_uploaded_seed_in_both_forms)
            what = f"{name} member_fast={fast} {'fused' if on else 'three-launch'} member {b}"
            _same_bits_or_close(what + ", gval", L2[b], L[b], gv2[b], gv[b])
            _same_bits_or_close(what + ", arena", L2[b], L[b], f2.get_factor_adjoint_batch(b), G[b], mask)
    f2.close()


# ---- 6: a member that is not positive definite ------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "three-launch"])
def test_one_bad_member_is_skipped_and_the_others_are_served(fused):
    name = "p2d32-nb16"
    c = be.case(name)
    f, mask = c["f"], c["mask"]
    gv, G, _ = _sweep(name, fused, members=[0, 2])
    Lgood = _factors(f, 2)
    vals = _values(name).copy()
    vals[1, f.ptr[f.n // 2] - 1] *= -1.0          # the diagonal entry of one variable of the middle member
    assert f.factor_batch(vals) == -20
    _fused(f, fused)
    seeds = np.stack([np.nan_to_num(s) for s in _seeds(name)])
    f.set_factor_adjoint_batch(seeds)
    before = f.get_factor_adjoint_batch(1).copy()
    out = np.zeros((NB, f.nnz))
    rc = f.lib.spllt_hip_factor_adjoint_batch(f.fkeep, api._dp(out), f.nnz)
    assert rc == -20 and "skipped" in f.last_error()
    assert np.isnan(out[1]).all()
    assert np.array_equal(f.get_factor_adjoint_batch(1), before)
    for b, g in ((0, 0), (2, 1)):       # member b against member g of the batch without the bad member
        Lb = f.get_factor_batch(b)
        _same_bits_or_close(f"{name} member {b} beside a bad member, gval", Lb, Lgood[g], out[b], gv[g])
        _same_bits_or_close(f"{name} member {b} beside a bad member, arena", Lb, Lgood[g], f.get_factor_adjoint_batch(b),
                            G[g], mask)
    # the Python call hands the rows on without raising; the handle is still good
    f.set_factor_adjoint_batch(seeds)
    assert np.isnan(f.factor_adjoint_batch()[1]).all()
    assert f.factor_batch(_values(name)) == 0


# ---- 7: states ------------------------------------------------------------------------------------------------
def test_states_storage_and_the_single_handle():
    name = "p2d12-nb4"
    A = be.case(name)["A"]
    f, val = make_case(A, nb=4, nemin=4, panel_width=32)
    mask = be.case(name)["mask"]
    n, arena = f.n, f.sym_info()["arena"]
    v = np.ones((NB, n))

    def refused(call, word):
        with pytest.raises(api.SplltError) as ei:
            call()
        assert ei.value.flag == -10 and word in f.last_error(), f.last_error()

    # the single handle's adjoint: seeded before anything of the batch happens
    f.factor(val).wait()
    single = np.where(mask, np.random.default_rng(3).standard_normal(arena), 0.0)
    f.set_factor_adjoint(single)
    assert f.factor_batch(_values(name)) == 0
    refused(f.factor_adjoint_batch, "seeded")                                     # unseeded
    refused(lambda: f.factor_adjoint_seed_batch(v, v, accumulate=True), "seeded")
    refused(lambda: f.get_factor_adjoint_batch(0), "seed")
    assert f.device_factor_adjoint_batch_ptr() == (None, 0) and f.batch_adjoint_launches() == 0
    seeds = np.stack([np.nan_to_num(s) for s in _seeds(name)])
    f.set_factor_adjoint_batch(seeds)
    f.factor_adjoint_seed_batch(v, 2.0 * v, accumulate=True)
    p, stride = f.device_factor_adjoint_batch_ptr()
    assert p and stride >= arena
    g1 = f.factor_adjoint_batch()
    assert f.batch_adjoint_launches() > 0
    refused(f.factor_adjoint_batch, "swept")                                      # a second sweep
    refused(lambda: f.factor_adjoint_seed_batch(v, v, accumulate=True), "swept")
    f.get_factor_adjoint_batch(2)                                                 # swept: readable
    # a new batch makes it stale
    assert f.factor_batch(_values(name)) == 0
    refused(f.factor_adjoint_batch, "seeded")
    refused(lambda: f.get_factor_adjoint_batch(0), "seed")
    # a larger batch takes the arenas again
    big = np.stack([be.member(name, b % NB)["val"] for b in range(5)])
    assert f.factor_batch(big) == 0
    f.set_factor_adjoint_batch(np.stack([seeds[b % NB] for b in range(5)]))
    f.factor_adjoint_seed_batch(np.ones((5, n)), 2.0 * np.ones((5, n)), accumulate=True)
    g5 = f.factor_adjoint_batch()
    close = lambda x, y: float(np.abs(x - y).max() / np.abs(y).max()) <= B      # noqa: E731  (other factorizations)
    assert close(g5[:NB], g1) and close(g5[3], g1[0])
    # the two releases in either order leave the other usable
    assert f.selected_inverse_batch() == 0
    z = f.inverse_on_pattern_batch()
    f.release_factor_adjoint_batch()
    assert f.device_factor_adjoint_batch_ptr() == (None, 0)
    assert f.selected_inverse_batch() == 0 and np.array_equal(f.inverse_on_pattern_batch(), z)
    f.set_factor_adjoint_batch(np.stack([seeds[b % NB] for b in range(5)]))
    f.release_inverse_batch()
    f.factor_adjoint_seed_batch(np.ones((5, n)), 2.0 * np.ones((5, n)), accumulate=True)
    assert np.array_equal(f.factor_adjoint_batch(), g5)
    assert f.selected_inverse_batch() == 0 and np.array_equal(f.inverse_on_pattern_batch(), z)
    # release_batch drops all
    f.release_batch()
    assert f.device_factor_adjoint_batch_ptr() == (None, 0) and f.batch_adjoint_launches() == 0
    refused(f.factor_adjoint_batch, "no batch")
    # the single handle's arena and state went through all of this untouched
    assert np.array_equal(f.get_factor_adjoint()[mask], single[mask])
    f.factor_adjoint()
    f.close()


@pytest.mark.parametrize("state", ladder.GPU_STATES)
def test_ladder_with_a_device(state):
    c = capi_ladder.Ctx(_lib.load(), True)
    assert ladder.check_state(c, state, ladder.golden(True)) == ladder.ROWS_PER_STATE


# ---- 8: PyTorch ---------------------------------------------------------------------------------------------------
# gradcheck with its default eps, atol and rtol; v.clone() as in tests/test_autograd_gpu.py (gradcheck perturbs its
# input behind the version counter, a clone is a fresh tensor and is factorized).  nondet_tol: gradcheck runs the
# backward pass twice on two factorizations of the same values, whose last bits differ (atomic adds, module
# docstring); the gradients are O(1) and differ by some 1e-15 then.
NONDET = 1e-10


def _chol(A, **kw):
    from spllt_amd.torch_ops import SparseCholesky
    return SparseCholesky(A, nb=8, nemin=4, **kw)


def _torch_vals(A, nbatch):
    import torch
    n, ptr, row, _ = api.csc_lower_1based(A)
    from batch_emulate import member_values
    return torch.tensor(np.stack([member_values(A, b, ptr, row)[1] for b in range(nbatch)]), device="cuda",
                        requires_grad=True)


@pytest.mark.parametrize("op", ["L", "Lt", "Linv", "Ltinv"])
def test_gradcheck_factor_apply_batch(op):
    import torch
    A = matgen.poisson2d(6)
    ch = _chol(A)
    vals = _torch_vals(A, 2)
    X = torch.tensor(np.random.default_rng(1).standard_normal((2, ch.n, 2)), device="cuda", requires_grad=True)
    assert torch.autograd.gradcheck(lambda v, x: ch.factor_apply_batch(v.clone(), x, op), (vals, X), nondet_tol=NONDET)
    ch.close()


@pytest.mark.parametrize("kind", ["precision", "covariance"])
@pytest.mark.parametrize("mean_shape", [None, "n", "bn"])
@pytest.mark.parametrize("common", [False, True])
def test_gradcheck_rsample_batch(kind, mean_shape, common):
    import torch
    A = matgen.poisson2d(6)
    ch = _chol(A)
    vals = _torch_vals(A, 2)
    rng = np.random.default_rng(2)
    mean = None if mean_shape is None else torch.tensor(
        rng.standard_normal((ch.n,) if mean_shape == "n" else (2, ch.n)), device="cuda", requires_grad=True)
    args = (vals,) if mean is None else (vals, mean)
    fn = lambda v, m=None: ch.rsample_batch(v.clone(), 3, seed=11, kind=kind, mean=m, common_noise=common)   # noqa: E731
    assert torch.autograd.gradcheck(fn, args, nondet_tol=NONDET)
    # the forward pass is the library call of sample_batch with the same arguments, on the cached factors of ONE
    # tensor: the covariance kind (products without atomic adds) gives the same bits; the precision kind runs the
    # backward sweep of solve_batch, whose strips add with fp64 atomics and repeat to rounding only (DESIGN.md
    # sections 11 and 21) -- n = 36, condition number below 1e3: 1e-13 of the largest entry
    with torch.no_grad():
        vd = vals.detach()
        m0 = None if mean is None else mean.detach()
        same = ch.sample_batch(vd, 3, seed=11, kind=kind, mean=m0, common_noise=common)
        got = ch.rsample_batch(vd, 3, seed=11, kind=kind, mean=m0, common_noise=common)
        assert got.shape == same.shape == (2, ch.n, 3)
        if kind == "covariance":
            assert torch.equal(got, same)
        else:
            assert float((got - same).abs().max() / same.abs().max()) <= 1e-13
    ch.close()


@pytest.mark.parametrize("kind", ["precision", "covariance"])
def test_rsample_batch_gradient_against_dense_autograd(kind):
    """40 samples per member (two seed passes) on p2d16-nb8-pw32: d/dvals of sum(w * x) against torch's dense
    autograd through a dense Cholesky of P A_b P^T with the library's own noise"""
    import torch
    from spllt_amd.torch_ops import SparseCholesky
    name = "p2d16-nb8-pw32"
    c = be.case(name)
    f0, A = c["f"], c["A"]
    ch = SparseCholesky(A, nb=8, nemin=4, panel_width=32)
    n, nnz, nsamp = ch.n, ch.nnz, 40
    vals = torch.tensor(_values(name, range(2)), device="cuda", requires_grad=True)
    w = torch.tensor(np.random.default_rng(8).standard_normal((2, n, nsamp)), device="cuda")
    x = ch.rsample_batch(vals, nsamp, seed=5, kind=kind)
    (x * w).sum().backward()
    z = ch.f.white_noise_batch(nsamp, 5)                        # (B, n, nsamp), pivot order
    prow, pcol = ch.f.pattern_tables()
    order = ch.f.sym("order")                                  # user variable -> pivot position
    pr, pc = order[prow], order[pcol]
    for b in range(2):
        v = torch.tensor(vals.detach().cpu().numpy()[b], requires_grad=True)
        M = torch.zeros((n, n), dtype=torch.float64)
        M = M.index_put((torch.as_tensor(pr), torch.as_tensor(pc)), v)
        M = M.index_put((torch.as_tensor(pc), torch.as_tensor(pr)), v)
        Ld = torch.linalg.cholesky(M)
        zb = torch.tensor(z[b])
        yp = torch.linalg.solve_triangular(Ld.T, zb, upper=True) if kind == "precision" else Ld @ zb
        wp = torch.tensor(w[b].cpu().numpy()[np.argsort(order)])     # row p = pivot position p
        (yp * wp).sum().backward()
        e = float((vals.grad[b].cpu() - v.grad).abs().max() / v.grad.abs().max())
        xe = float((x[b].detach().cpu()[np.argsort(order)] - yp.detach()).abs().max() / yp.detach().abs().max())
        print(f"{name} {kind} member {b}: gradient vs dense autograd {e:.2e}, samples {xe:.2e}")
        assert xe <= 1e-12 and e <= 1e-10
    ch.close()


@pytest.mark.parametrize("kind", ["Linv", "Ltinv", "precision"])
def test_the_blocked_batch_solve_serves_forward_and_backward(kind):
    """batch_blocked=True: the solves of factor_apply_batch and the precision kind of rsample_batch go through
    solve_many_batch_dev.  Forward and gradients against the default routing on a handle of its own: two
    backward-stable solves of matrices with a condition number below 1e3 (poisson2d(6) scaled by member_matrix), and
    two factorizations: 1e-12 of the largest entry."""
    import torch
    A = matgen.poisson2d(6)
    out = []
    for blocked in (False, True):
        ch = _chol(A, batch_blocked=blocked)
        vals = _torch_vals(A, 2)
        X = torch.tensor(np.random.default_rng(4).standard_normal((2, ch.n, 35)), device="cuda", requires_grad=True)
        W = torch.tensor(np.random.default_rng(5).standard_normal((2, ch.n, 35)), device="cuda")
        launches0 = ch.f.solve_many_batch_info()["launches"]
        if kind == "precision":
            y = ch.rsample_batch(vals, 35, seed=3, kind="precision")
        else:
            y = ch.factor_apply_batch(vals, X, kind)
        (y * W).sum().backward()
        used = ch.f.solve_many_batch_info()["launches"] > launches0
        assert used == blocked, "the routing switch did not decide the path"
        out.append((y.detach().cpu().numpy(), vals.grad.cpu().numpy(),
                    None if kind == "precision" else X.grad.cpu().numpy()))
        ch.close()
    for got, want in zip(out[1], out[0]):
        if want is not None:
            e = float(np.abs(got - want).max() / np.abs(want).max())
            print(f"{kind}: blocked against default routing {e:.2e}")
            assert e <= 1e-12


def test_reproducible_handle_refuses_the_batch_operations():
    import torch
    A = matgen.poisson2d(6)
    ch = _chol(A, reproducible=True)
    vals = _torch_vals(A, 2)
    with pytest.raises(NotImplementedError):
        ch.factor_apply_batch(vals, torch.zeros((2, ch.n, 1), dtype=torch.float64, device="cuda"), "L")
    with pytest.raises(NotImplementedError):
        ch.rsample_batch(vals, 2)
    ch.close()
