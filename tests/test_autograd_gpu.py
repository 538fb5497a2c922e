"""GPU tests of the differentiable front end (spllt_amd.torch_ops) and of what it stands on: the sampled outer
product on the pattern (pattern_outer.hip), the device-side readers of the selected inverse, the factor serial."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import autograd_emulate as em
from helpers import bwd_err
from spllt_amd import api, matgen

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53


def _arrowhead(n=300):
    """one column of n entries, every other column its diagonal alone (diagonally dominant)"""
    A = sp.lil_matrix((n, n))
    A.setdiag(float(n))
    A[:, 0] = 1.0
    A[0, :] = 1.0
    A[0, 0] = float(n)
    return sp.csc_matrix(A)


KERNEL_CASES = {
    "p2d40": (lambda: matgen.poisson2d(40), 16),                 # columns of 1 to 3 entries
    "box12": (lambda: matgen.nd_like((10, 12, 12), 3), 512),     # columns longer than one wavefront
    "arrow300": (_arrowhead, 64),
}
# the cases of test_refine_gpu.py
SOLVE_CASES = {
    "box11-nb64": (lambda: matgen.nd_like((11, 10, 9), 2), 64),
    "p3d14-nb384": (lambda: matgen.poisson3d(14), 384),
}


@functools.lru_cache(maxsize=None)
def _pattern(name):
    gen, nb = KERNEL_CASES[name]
    A = sp.csc_matrix(gen())
    n, ptr, row, val = api.csc_lower_1based(A)
    f = api.Factorization(n, ptr, row, nb=nb, nemin=16)
    prow = (row - 1).astype(np.int64)
    pcol = np.repeat(np.arange(n), np.diff(ptr))
    return f, prow, pcol


@functools.lru_cache(maxsize=None)
def _vectors(name, nvec):
    f, _, _ = _pattern(name)
    rng = np.random.default_rng(1000 + nvec)
    return rng.standard_normal((f.n, nvec)), rng.standard_normal((f.n, nvec))


def _outer_dev(f, U, V, alpha, pad_u=3, pad_v=7):
    """the device twin on padded arrays: NaN rows after each vector (a read of them would show in the result),
    a sentinel after the nnz outputs; returns (out, the three device arrays after the call, their images before)"""
    import torch
    n, nvec = U.shape
    ldu, ldv = n + pad_u, n + pad_v
    hu = np.full((nvec, ldu), np.nan)
    hv = np.full((nvec, ldv), np.nan)
    hu[:, :n], hv[:, :n] = U.T, V.T
    du, dv = torch.tensor(hu, device="cuda"), torch.tensor(hv, device="cuda")
    out = torch.full((f.nnz + 5,), -7.25, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    f.pattern_outer_dev(du.data_ptr(), dv.data_ptr(), nvec, out.data_ptr(), ldu=ldu, ldv=ldv, alpha=alpha)
    assert np.array_equal(du.cpu().numpy(), hu, equal_nan=True) and np.array_equal(dv.cpu().numpy(), hv, equal_nan=True)
    out = out.cpu().numpy()
    assert (out[f.nnz:] == -7.25).all()
    return out[:f.nnz]


@pytest.mark.parametrize("nvec", [1, 4, 5, 33])
@pytest.mark.parametrize("name", list(KERNEL_CASES))
def test_pattern_outer_meets_the_rounding_bound_of_its_fma_chain(name, nvec):
    """Per entry the kernel computes acc_0 = 0, acc_m = fma(a_m, b_m, acc_{m-1}) over the M <= 2 nvec products
    (u_i v_j, then u_j v_i, q ascending) and out = alpha * acc_M.  An fma rounds once, (a b + acc)(1 + d), |d| <= u =
    2^-53, and the final product once more, so every term reaches the result with at most M + 1 <= 2 nvec + 1 factors
    (1 + d):  |out - alpha sum| <= gamma_{2 nvec + 1} |alpha| sum |a_m b_m|, gamma_k = k u / (1 - k u).  For k <= 67,
    gamma_k <= (k + 1/2) u, which leaves u / 2 per unit of magnitude for the error of the long-double reference
    (<= (2 nvec + 1) 2^-64): the bar (2 nvec + 2) 2^-53 |alpha| sum_q (|u_i v_j| + |u_j v_i|)."""
    f, prow, pcol = _pattern(name)
    U, V = _vectors(name, nvec)
    for alpha in (-1.0, 0.37):
        ref = em.pattern_outer(prow, pcol, U, V, alpha, dtype=np.longdouble)
        bar = (2 * nvec + 2) * np.longdouble(U53) * em.pattern_outer_magnitude(prow, pcol, U, V, alpha)
        got_dev = _outer_dev(f, U, V, alpha)
        got_host = f.pattern_outer(U, V, alpha)
        for what, got in (("dev", got_dev), ("host", got_host)):
            err = np.abs(got.astype(np.longdouble) - ref)
            worst = float((err / np.maximum(bar, np.longdouble(1e-300))).max())
            print(f"{name} nvec={nvec} alpha={alpha} {what}: max err / bar = {worst:.3f}")
            assert (err <= bar).all(), (what, worst)
        assert np.array_equal(got_dev, got_host)      # (the same chain through both entry points)


def test_pattern_outer_is_bit_identical_across_calls_and_writes_zero_for_no_vectors():
    f, prow, pcol = _pattern("box12")
    U, V = _vectors("box12", 33)
    a = _outer_dev(f, U, V, -1.0)
    b = _outer_dev(f, U, V, -1.0, pad_u=11, pad_v=2)      # other leading dimensions, the same bits
    assert np.array_equal(a, b)
    assert np.array_equal(f.pattern_outer(U, V, -1.0), f.pattern_outer(U, V, -1.0))
    # no vectors: alpha * 0 everywhere (the arrays are not read, but their addresses must not be null)
    import torch
    assert (f.pattern_outer(U[:, :0], V[:, :0], 2.0) == 0.0).all()
    du = torch.full((4,), float("nan"), dtype=torch.float64, device="cuda")
    out = torch.full((f.nnz,), -7.25, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    f.pattern_outer_dev(du.data_ptr(), du.data_ptr(), 0, out.data_ptr(), alpha=2.0)
    assert (out.cpu().numpy() == 0.0).all()


@pytest.mark.parametrize("limit", [0, 20])
def test_pattern_outer_batch_equals_single_calls(limit):
    """nbatch = 3 in one launch (and, with the grid limit lowered below two members' workgroups, in three) against
    three single calls, bit for bit; an output stride > nnz with sentinels"""
    import torch
    f, prow, pcol = _pattern("p2d40")
    n, nnz, nvec, nbatch = f.n, f.nnz, 5, 3
    assert 2 * ((nnz + 255) // 256) > 20
    rng = np.random.default_rng(77)
    ldu, ldv, ldout = n + 1, n + 4, nnz + 3
    hu, hv = np.full((nbatch, nvec, ldu), np.nan), np.full((nbatch, nvec, ldv), np.nan)
    hu[:, :, :n], hv[:, :, :n] = rng.standard_normal((nbatch, nvec, n)), rng.standard_normal((nbatch, nvec, n))
    du, dv = torch.tensor(hu, device="cuda"), torch.tensor(hv, device="cuda")
    out = torch.full((nbatch, ldout), -7.25, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    assert f.lib.spllt_hip_debug(b"batch_grid_limit=%d" % limit) == 0
    try:
        f.pattern_outer_batch_dev(du.data_ptr(), dv.data_ptr(), nbatch, nvec, out.data_ptr(), ldu=ldu, ldv=ldv,
                                  ldout=ldout, alpha=-1.0)
    finally:
        f.lib.spllt_hip_debug(b"batch_grid_limit=0")
    out = out.cpu().numpy()
    assert (out[:, nnz:] == -7.25).all()
    for b in range(nbatch):
        single = _outer_dev(f, hu[b, :, :n].T, hv[b, :, :n].T, -1.0)
        assert np.array_equal(out[b, :nnz], single), b


# ---- readers ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _matrix(name):
    gen, nb = SOLVE_CASES[name]
    A = sp.csc_matrix(gen())
    n, ptr, row, val = api.csc_lower_1based(A)
    return A, (n, ptr, row), val, nb


def test_inverse_on_pattern_dev_returns_the_bits_of_the_host_reader():
    import torch
    A, (n, ptr, row), val, nb = _matrix("box11-nb64")
    f = api.Factorization(n, ptr, row, nb=nb, nemin=16)
    f.factor(val).wait()
    f.selected_inverse()
    host = f.inverse_on_pattern()
    out = torch.full((f.nnz + 2,), -7.25, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    f.inverse_on_pattern_dev(out.data_ptr())
    out = out.cpu().numpy()
    assert np.array_equal(out[:f.nnz], host) and (out[f.nnz:] == -7.25).all()
    # three members, the middle one indefinite: its row is NaN in both readers
    vals = np.stack([val, -val, 2.0 * val])
    assert f.factor_batch(vals) == -20 and f.selected_inverse_batch() == -20
    hostb = f.inverse_on_pattern_batch()
    ldout = f.nnz + 3
    outb = torch.full((3, ldout), -7.25, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    f.inverse_on_pattern_batch_dev(outb.data_ptr(), ldout=ldout)
    outb = outb.cpu().numpy()
    assert np.isnan(hostb[1]).all() and np.isfinite(hostb[[0, 2]]).all()
    assert np.array_equal(outb[:, :f.nnz], hostb, equal_nan=True) and (outb[:, f.nnz:] == -7.25).all()
    f.close()


# ---- autograd -----------------------------------------------------------------------------------------
def _chol(name, **kw):
    import spllt_amd
    A, pattern, val, nb = _matrix(name)
    return spllt_amd.SparseCholesky(pattern, nb=nb, nemin=16, **kw)


def test_gradcheck_of_solve_and_logdet():
    """torch.autograd.gradcheck with its default eps, atol, rtol and nondet_tol = 0, on poisson2d(6).  gradcheck
    perturbs its inputs through ``.data``, which by design does not move the version counter the factor cache
    looks at (torch's own check of saved tensors is blind to it in the same way), so the checked function hands
    the handle a clone: every evaluation factorizes, and nondet_tol = 0 then also asks for a deterministic
    factorization.  test_cache_* below cover the cache."""
    import torch
    import spllt_amd
    A = matgen.poisson2d(6)
    n, ptr, row, val = api.csc_lower_1based(A)
    chol = spllt_amd.SparseCholesky(A, nb=16, nemin=4, reproducible=True)
    rng = np.random.default_rng(6)
    tv = torch.tensor(val, device="cuda", requires_grad=True)
    tb = torch.tensor(rng.standard_normal((n, 3)), device="cuda", requires_grad=True)
    assert torch.autograd.gradcheck(lambda v, b: chol.solve(v.clone(), b), (tv, tb), nondet_tol=0.0)
    assert torch.autograd.gradcheck(lambda v: chol.logdet(v.clone()), (tv,), nondet_tol=0.0)
    # a vector right-hand side takes the same path
    t1 = torch.tensor(rng.standard_normal(n), device="cuda", requires_grad=True)
    assert torch.autograd.gradcheck(lambda v, b: chol.solve(v.clone(), b), (tv, t1), nondet_tol=0.0)
    chol.close()


@pytest.mark.parametrize("name", list(SOLVE_CASES))
def test_solve_and_logdet_identities(name):
    import torch
    A, pattern, val, nb = _matrix(name)
    n = pattern[0]
    chol = _chol(name)
    rng = np.random.default_rng(3)
    B = A @ rng.standard_normal((n, 3))
    G = rng.standard_normal((n, 3))
    tv = torch.tensor(val, device="cuda", requires_grad=True)
    tb = torch.tensor(B, device="cuda", requires_grad=True)
    X = chol.solve(tv, tb)
    assert X.shape == (n, 3)
    (X * torch.tensor(G, device="cuda")).sum().backward()
    x, lam = X.detach().cpu().numpy(), tb.grad.cpu().numpy()
    for q in range(3):
        ex, el = bwd_err(A, x[:, q], B[:, q]), bwd_err(A, lam[:, q], G[:, q])
        print(f"{name} column {q}: bwd_err x {ex:.2e} lambda {el:.2e}")
        assert ex <= 1e-14 and el <= 1e-14
    assert torch.equal(tv.grad, chol.pattern_outer(tb.grad, X.detach(), alpha=-1.0))
    # log det and its gradient: the bits of the handle's own readers
    tv.grad = None
    serial = chol.f.factor_serial(0)
    ld = chol.logdet(tv)
    assert chol.f.factor_serial(0) == serial          # (the factor of the solve serves)
    assert ld.dim() == 0 and ld.item() == chol.f.log_det()
    ld.backward()
    prow, pcol = chol.f.pattern_tables()
    assert np.array_equal(tv.grad.cpu().numpy(), np.where(prow == pcol, 1.0, 2.0) * chol.f.inverse_on_pattern())
    chol.close()


def test_batch_identities():
    import torch
    name = "box11-nb64"
    A, pattern, val, nb = _matrix(name)
    n = pattern[0]
    chol = _chol(name)
    scales = np.array([1.0, 2.5, 0.75])
    rng = np.random.default_rng(4)
    B = np.stack([s * (A @ rng.standard_normal((n, 2))) for s in scales])
    G = rng.standard_normal((3, n, 2))
    tv = torch.tensor(scales[:, None] * val[None, :], device="cuda", requires_grad=True)
    tb = torch.tensor(B, device="cuda", requires_grad=True)
    X = chol.solve_batch(tv, tb)
    assert X.shape == (3, n, 2)
    (X * torch.tensor(G, device="cuda")).sum().backward()
    x, lam = X.detach().cpu().numpy(), tb.grad.cpu().numpy()
    for b, s in enumerate(scales):
        for q in range(2):
            ex, el = bwd_err(s * A, x[b, :, q], B[b, :, q]), bwd_err(s * A, lam[b, :, q], G[b, :, q])
            print(f"member {b} column {q}: bwd_err x {ex:.2e} lambda {el:.2e}")
            assert ex <= 1e-14 and el <= 1e-14
        assert torch.equal(tv.grad[b], chol.pattern_outer(tb.grad[b], X[b].detach(), alpha=-1.0)), b
    tv.grad = None
    serial = chol.f.factor_serial(1)
    ld = chol.logdet_batch(tv)
    assert chol.f.factor_serial(1) == serial
    assert ld.shape == (3,) and np.array_equal(ld.detach().cpu().numpy(), chol.f.log_det_batch())
    ld.sum().backward()
    prow, pcol = chol.f.pattern_tables()
    assert np.array_equal(tv.grad.cpu().numpy(), np.where(prow == pcol, 1.0, 2.0)[None, :] * chol.f.inverse_on_pattern_batch())
    # one indefinite member raises in forward and is named
    bad = tv.detach().clone()
    bad[1] = -bad[1]
    with pytest.raises(api.SplltError, match=r"members \[1\]") as ei:
        chol.solve_batch(bad, tb.detach())
    assert ei.value.flag == -20
    with pytest.raises(api.SplltError, match=r"members \[1\]"):
        chol.logdet_batch(bad)
    chol.close()


def _passes(chol, val, B, G):
    """forward + backward of solve and of logdet on fresh tensors: (x, grad_val, grad_B, logdet, its gradient)"""
    import torch
    tv = torch.tensor(val, device="cuda", requires_grad=True)
    tb = torch.tensor(B, device="cuda", requires_grad=True)
    X = chol.solve(tv, tb)
    (X * torch.tensor(G, device="cuda")).sum().backward()
    gv = tv.grad.clone()
    tv.grad = None
    ld = chol.logdet(tv)
    ld.backward()
    return [t.detach().cpu().numpy() for t in (X, gv, tb.grad, ld, tv.grad)]


def test_reproducible_passes_give_identical_bits():
    name = "box11-nb64"
    A, pattern, val, nb = _matrix(name)
    chol = _chol(name, reproducible=True)
    rng = np.random.default_rng(8)
    B, G = rng.standard_normal((pattern[0], 5)), rng.standard_normal((pattern[0], 5))
    first, second = _passes(chol, val, B, G), _passes(chol, val, B, G)
    for a, b in zip(first, second):
        assert np.array_equal(a, b)
    with pytest.raises(NotImplementedError):
        chol.solve_batch(None, None)
    with pytest.raises(NotImplementedError):
        chol.logdet_batch(None)
    chol.close()


def test_cache_serves_one_factor_and_notices_in_place_changes():
    import torch
    name = "box11-nb64"
    A, pattern, val, nb = _matrix(name)
    n = pattern[0]
    chol = _chol(name)
    tv = torch.tensor(val, device="cuda")
    tb = torch.tensor(A @ np.ones((n, 1)), device="cuda")
    s0 = chol.f.factor_serial(0)
    x = chol.solve(tv, tb)
    chol.logdet(tv)
    chol.solve(tv, tb[:, 0])
    assert chol.f.factor_serial(0) == s0 + 1
    assert np.abs(x.cpu().numpy() - 1.0).max() <= 1e-10
    tv.mul_(2.0)                                   # in place: the version counter moves
    x2 = chol.solve(tv, tb)
    assert chol.f.factor_serial(0) == s0 + 2
    assert np.abs(x2.cpu().numpy() - 0.5).max() <= 1e-10
    chol.solve(tv.clone(), tb)                     # another tensor with the same values: factorized again
    assert chol.f.factor_serial(0) == s0 + 3
    chol.close()


def test_backward_after_another_factorization_uses_the_saved_values():
    import torch
    name = "box11-nb64"
    A, pattern, val, nb = _matrix(name)
    n = pattern[0]
    chol = _chol(name, reproducible=True)
    rng = np.random.default_rng(9)
    B = torch.tensor(rng.standard_normal((n, 2)), device="cuda")
    v1 = torch.tensor(val, device="cuda", requires_grad=True)
    v2 = torch.tensor(1.7 * val, device="cuda")
    x = chol.solve(v1, B)
    ld = chol.logdet(v1)
    chol.solve(v2, B)                               # the handle now holds the factor of another matrix
    (x.sum() + ld).backward()
    stale = v1.grad.clone()
    fresh = torch.tensor(val, device="cuda", requires_grad=True)
    (chol.solve(fresh, B).sum() + chol.logdet(fresh)).backward()
    assert torch.equal(stale, fresh.grad)
    chol.close()


def test_errors_are_raised_before_any_library_call():
    import torch
    name = "box11-nb64"
    A, pattern, val, nb = _matrix(name)
    n = pattern[0]
    chol = _chol(name)
    tv = torch.tensor(val, device="cuda")
    tb = torch.ones((n, 2), dtype=torch.float64, device="cuda")
    with pytest.raises(TypeError):
        chol.solve(tv.float(), tb)
    with pytest.raises(TypeError):
        chol.solve(tv, tb.float())
    with pytest.raises(TypeError):
        chol.solve(val, tb)
    with pytest.raises(ValueError):
        chol.solve(tv.cpu(), tb)
    with pytest.raises(ValueError):
        chol.solve(tv, tb.cpu())
    with pytest.raises(ValueError):
        chol.solve(tv[:-1], tb)
    with pytest.raises(ValueError):
        chol.solve(tv, tb[:-1])
    with pytest.raises(ValueError):
        chol.logdet(torch.cat([tv, tv])[::2])      # not contiguous
    with pytest.raises(ValueError):
        chol.solve_batch(tv[None, :], tb)
    with pytest.raises(ValueError):
        chol.pattern_outer(tb, tb[:, :1])
    assert chol.f.factor_serial(0) == 0 and chol.f.factor_serial(1) == 0 and chol.device is None
    # a matrix that is not positive definite raises as Factorization.wait does
    with pytest.raises(api.SplltError) as ei:
        chol.solve(-tv, tb)
    assert ei.value.flag == -20
    with pytest.raises(api.SplltError):
        chol.logdet(-tv)
    assert np.abs(chol.solve(tv, torch.tensor(A @ np.ones(n), device="cuda")).cpu().numpy() - 1.0).max() <= 1e-10
    chol.close()
