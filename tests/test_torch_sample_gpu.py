"""GPU tests of SparseCholesky.sample (torch_ops.py): samples from the cached factor as device tensors, the
gradient to the mean, none to the matrix values."""
import numpy as np
import pytest

from spllt_amd import api, matgen

pytestmark = pytest.mark.gpu


def _setup():
    import torch
    from spllt_amd.torch_ops import SparseCholesky
    A = matgen.nd_like((7, 6, 5), 2)
    n, ptr, row, val = api.csc_lower_1based(A)
    chol = SparseCholesky(A, nb=64, nemin=16)
    v = torch.tensor(val, device="cuda", requires_grad=True)
    f = api.Factorization(n, ptr, row, nb=64, nemin=16)
    f.factor(val).wait()
    return torch, chol, v, f, n


def test_sample_equals_the_library_call_and_differentiates_the_mean_only():
    torch, chol, v, f, n = _setup()
    m = np.random.default_rng(0).standard_normal(n)
    mean = torch.tensor(m, device="cuda", requires_grad=True)
    for kind in ("covariance", "precision"):
        x = chol.sample(v, 37, seed=3, kind=kind, mean=mean)
        assert isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float64 and tuple(x.shape) == (n, 37)
        want = f.sample(37, seed=3, kind=kind, mean=m)
        # (two handles with the default engine: their factors agree to rounding, and so do the samples)
        np.testing.assert_allclose(x.detach().cpu().numpy(), want, rtol=1e-12, atol=1e-12 * np.abs(want).max())
        if kind == "covariance":      # on one factor the product repeats bit for bit
            assert np.array_equal(chol.sample(v, 37, seed=3, kind=kind, mean=mean).detach().cpu().numpy(),
                                  x.detach().cpu().numpy())
        assert x.requires_grad
        mean.grad = None
        x[:, 5].sum().backward()
        assert v.grad is None
        assert np.array_equal(mean.grad.cpu().numpy(), np.ones(n))
    x0 = chol.sample(v, 4, seed=3, kind="covariance")
    assert not x0.requires_grad
    want0 = f.sample(4, seed=3, kind="covariance")
    np.testing.assert_allclose(x0.cpu().numpy(), want0, rtol=1e-12, atol=1e-12 * np.abs(want0).max())
    with pytest.raises(api.SplltError):
        chol.sample(v, 2, kind="variance")
    chol.close()
    f.close()


def test_reproducible_handle_repeats_both_kinds_bit_for_bit():
    torch, _chol, v, f, n = _setup()
    from spllt_amd.torch_ops import SparseCholesky
    _chol.close()
    f.close()
    chol = SparseCholesky(matgen.nd_like((7, 6, 5), 2), nb=64, nemin=16, reproducible=True)
    for kind in ("covariance", "precision"):
        a = chol.sample(v, 9, seed=1, kind=kind).cpu().numpy()
        chol.invalidate()                      # factorize again: flag 4096 gives the same factor bits
        b = chol.sample(v, 9, seed=1, kind=kind).cpu().numpy()
        assert np.array_equal(a, b), kind
    assert chol.f.set_reproducible_solve(False) is False     # the switch is restored after every call
    chol.close()
