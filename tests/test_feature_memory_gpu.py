"""GPU tests of the device memory of the optional features: every allocation a feature makes on first use is
failed once (spllt_hip_debug "alloc_fail_at=k", a simulated return code) and the roll-back is checked by what it
leaves behind: the ledger of device buffers (program("owned")) as it was before the call, every other solve with
the bits it had, and the feature itself with its earlier result on the next call.  The sharing tests run the
sweep of one feature while another one that shares a table or a scratch with it stays prepared.

Families whose own suites assert bit-equality (reproducible solve, products, samplers, constraints) are compared
with np.array_equal where the call works on the same factor bits; the batch products factorize their batches anew
in every call and are compared like the others.  The others add with fp64 atomics or iterate to a tolerance: two runs of the same call on
the same input differ by the order of those sums only, which the project's suites bound by the backward-error
bar; close() below asks for 1e-10 of the largest entry, five orders above fp64 rounding of these
well-conditioned cases and far below any wrong entry."""
import numpy as np
import pytest
import scipy.sparse as sp

from helpers import make_case
from spllt_amd import api, matgen

pytestmark = pytest.mark.gpu

NB, NV = 3, 5          # members of the larger batch, vectors per member
MAX_K = 32


def close(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.abs(a - b).max() <= 1e-10 * max(np.abs(b).max(), 1e-300)


class Case:
    """box11-nb64, factorized, with the right-hand sides every test shares (read-only)"""

    def __init__(self):
        A = matgen.nd_like((11, 10, 9), 2)
        self.f, self.val = make_case(A, nb=64, nemin=16)
        self.f.factor(self.val).wait()
        self.n = A.shape[0]
        rng = np.random.default_rng(7)
        self.B3 = rng.standard_normal((self.n, 3))
        self.X = rng.standard_normal((self.n, NV))
        self.XB = rng.standard_normal((NB, NV, self.n))
        self.vals = np.stack([self.val * (1.0 + 0.05 * b) for b in range(NB)])
        self.C = rng.standard_normal((3, self.n))
        self.mean = rng.standard_normal(self.n)
        cols = rng.integers(0, self.n, size=(NV, 2))
        self.S = sp.csc_matrix((np.ones(2 * NV), (cols.ravel(), np.repeat(np.arange(NV), 2))), shape=(self.n, NV))
        for a in (self.B3, self.X, self.XB, self.vals, self.C, self.mean):
            a.setflags(write=False)
        self.base = self.f.solve_many(self.B3)

    def owned(self):
        return tuple(int(v) for v in self.f.program("owned"))

    def batches(self, feature):
        """a batch of 2, the feature, a batch of 3, the feature again (a larger batch: everything again)"""
        self.f.factor_batch(self.vals[:2])
        feature(2)
        self.f.factor_batch(self.vals)
        return feature(NB)


@pytest.fixture()
def c():
    case = Case()
    yield case
    case.f.lib.spllt_hip_debug(b"alloc_fail_at=0")
    case.f.close()


def sweep(c, call, release, equal, min_failures, width=None, one_take=False):
    """steps 1-3 of the issue for one feature; returns the number of allocations it makes.  one_take: the call is
    one transaction, so a failure leaves the ledger as it was at once; a call of several steps (seed and sweep, two
    batches) may keep what its earlier steps took, and is compared after its release: a buffer that a roll-back
    dropped without returning it stays in the ledger and shows there."""
    f, lib = c.f, c.f.lib
    ref = call()
    release()
    failures = 0
    for k in range(1, MAX_K + 2):
        before = c.owned()
        raised, got = False, None
        assert lib.spllt_hip_debug(b"alloc_fail_at=%d" % k) == 0
        try:
            try:
                got = call()
            except api.SplltError as e:
                raised = True
                assert e.flag == -1, (k, e)
                assert "memory" in f.last_error(), (k, f.last_error())
            armed = lib.spllt_hip_debug(b"alloc_fail_armed")
        finally:
            assert lib.spllt_hip_debug(b"alloc_fail_at=0") == 0
        if armed == 1:                      # the feature makes k - 1 allocations
            assert not raised and equal(got, ref), k
            release()
            break
        failures += 1
        if raised:
            if one_take:
                assert c.owned()[0] == before[0], (k, c.owned(), before)
            release()
            assert c.owned() == before, (k, c.owned(), before)
        else:                               # only a width fallback may absorb a failed allocation
            assert width is not None and width() in (16, 8), k
            assert equal(got, ref), k
        assert close(f.solve_many(c.B3), c.base), k   # (fp64 atomic adds: equal to rounding, not in bits)
        again = call()
        assert equal(again, ref), k
        release()
        assert c.owned() == before, (k, c.owned(), before)
    print(f"allocations {k - 1}, injected failures {failures}")
    assert k <= MAX_K
    assert failures >= max(1, min_failures)
    return k - 1


# ---- the families: (call, release, equality, buffers the comment of engine.hpp lists, width getter) ----------
def fam_repro(c):
    return (lambda: c.f.solve_reproducible(c.X), c.f.release_solve_repro, np.array_equal, 3, None, True)


def fam_fmult(c):
    # (no getter for the width of the single-handle products: a fallback shows as the same bits without a raise)
    return (lambda: c.f.factor_mult(c.X), c.f.release_factor_mult, np.array_equal, 3, lambda: 16, True)


def fam_sample(c):
    # (kind "covariance": mean + P^T L z through the products, bit-reproducible; the mean is taken after them)
    return (lambda: c.f.sample(NV, seed=3, kind="covariance", mean=c.mean), c.f.release_factor_mult, np.array_equal, 1,
            lambda: 16, False)


def fam_sparse(c):
    return (lambda: np.concatenate([c.f.solve_sparse(c.S).ravel(), c.f.gram(c.S).ravel()]), c.f.release_solve_sparse,
            close, 2, None, True)


def fam_refine(c):
    return (lambda: c.f.solve_refined(c.val, c.X)[0], c.f.release_refine, close, 5, None, True)


def fam_constraints(c):
    def call():   # (W = A^-1 C^T through the reproducible solve: the same bits from every set_constraints)
        c.f.set_reproducible_solve(True)
        try:
            c.f.set_constraints(c.C)
            return c.f.constrain(c.X)
        finally:
            c.f.set_reproducible_solve(False)
    return (call, c.f.release_constraints, np.array_equal, 5, None, True)


def fam_selinv(c):
    return (lambda: c.f.selected_inverse().inverse_diag(), c.f.release_inverse, close, 2, None, True)


def fam_fadj(c):
    def call():
        c.f.factor_adjoint_seed(c.X, c.X)
        return c.f.factor_adjoint()
    return (call, c.f.release_factor_adjoint, close, 3, None, False)


def fam_batch(c):
    return (lambda: c.batches(lambda nb: c.f.solve_batch(c.XB[:nb])), c.f.release_batch, close, 6, None, False)


def fam_bmult(c):
    # (every call factorizes the batch again, with fp64 atomic adds: the products have the bits of THEIR factors,
    # which agree to rounding from one factorization to the next)
    return (lambda: c.batches(lambda nb: c.f.factor_mult_batch(c.XB[:nb])), c.f.release_factor_mult_batch,
            close, 3, lambda: 16, False)


def fam_bsm(c):
    seen = []

    def feature(nb):
        x = c.f.solve_many_batch(c.XB[:nb])
        seen.append(c.f.solve_many_batch_info()["rb"])
        return x
    return (lambda: c.batches(feature), c.f.release_solve_many_batch, close, 1, lambda: min(seen[-2:]), False)


def fam_brefine(c):
    seen = []

    def feature(nb):
        y = c.f.matvec_batch(c.vals[:nb], c.XB[:nb])
        x = c.f.solve_refined_batch(c.vals[:nb], c.XB[:nb])[0]
        seen.append(c.f.solve_refined_batch_info()["width"])
        return np.concatenate([np.ravel(y), np.ravel(x)])
    return (lambda: c.batches(feature), c.f.release_refine_batch, close, 4, lambda: min(seen[-2:]), False)


def fam_bselinv(c):
    def feature(nb):
        c.f.selected_inverse_batch()
        return c.f.inverse_diag_batch()
    return (lambda: c.batches(feature), c.f.release_inverse_batch, close, 2, None, False)


def fam_bfadj(c):
    def feature(nb):
        c.f.factor_adjoint_seed_batch(c.XB[:nb], c.XB[:nb])
        return c.f.factor_adjoint_batch()
    return (lambda: c.batches(feature), c.f.release_factor_adjoint_batch, close, 2, None, False)


FAMILIES = {"solve_repro": fam_repro, "factor_mult": fam_fmult, "sample_host_mean": fam_sample,
            "solve_sparse_and_gram": fam_sparse, "solve_refined": fam_refine, "constraints": fam_constraints,
            "selected_inverse": fam_selinv, "factor_adjoint": fam_fadj, "factor_batch_solve_batch": fam_batch,
            "factor_mult_batch": fam_bmult, "solve_many_batch": fam_bsm, "refine_batch_and_matvec_batch": fam_brefine,
            "selected_inverse_batch": fam_bselinv, "factor_adjoint_batch": fam_bfadj}


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_every_allocation_of_a_feature_fails_once(c, family):
    call, release, equal, buffers, width, one_take = FAMILIES[family](c)
    sweep(c, call, release, equal, buffers, width, one_take)


def test_inverse_on_pattern_fails_once(c):
    """the gathered entries are taken beside a valid inverse, which stays"""
    c.f.selected_inverse()
    diag = c.f.inverse_diag()

    def release():   # (the buffer goes with the inverse: take that again)
        c.f.release_inverse()
        c.f.selected_inverse()
    sweep(c, c.f.inverse_on_pattern, release, close, 1)
    assert close(c.f.inverse_diag(), diag)


def test_pattern_outer_fails_once(c):
    """the staging block of the host entry point grows with the call and stays with the handle: the sweep sees it
    on a fresh handle only, so every step takes a new one"""
    fails = 0
    ref = None
    for k in (1, 2):
        case = Case()
        try:
            f = case.f
            if ref is None:
                ref = c.f.pattern_outer(c.X, c.X)
            before = case.owned()
            assert f.lib.spllt_hip_debug(b"alloc_fail_at=%d" % k) == 0
            try:
                with pytest.raises(api.SplltError) as e:
                    f.pattern_outer(c.X, c.X)
                assert e.value.flag == -1 and "memory" in f.last_error()
                assert f.lib.spllt_hip_debug(b"alloc_fail_armed") == 0
            finally:
                f.lib.spllt_hip_debug(b"alloc_fail_at=0")
            fails += 1
            assert case.owned()[0] == before[0] + (k - 1)      # (k = 2: the tables are there and stay)
            assert close(f.solve_many(c.B3), c.base)
            assert np.array_equal(f.pattern_outer(c.X, c.X), ref)
        finally:
            case.f.close()
    assert fails == 2      # the tables of the pattern, the staging block


PAIRS = [("solve_repro", "factor_mult"), ("factor_mult", "factor_mult_batch"),
         ("solve_refined", "refine_batch_and_matvec_batch"), ("selected_inverse", "factor_adjoint"),
         ("selected_inverse_batch", "factor_adjoint_batch")]


@pytest.mark.parametrize("first,second", PAIRS + [(b, a) for a, b in PAIRS])
def test_a_feature_survives_the_failures_of_the_one_it_shares_with(c, first, second):
    call_a, release_a, equal_a, _, _, _ = FAMILIES[first](c)
    call_b, release_b, equal_b, _, width_b, _ = FAMILIES[second](c)
    call_a(), call_b()      # (what stays with the handle for good: the order table, the program tables)
    release_a(), release_b()
    owned0 = c.owned()
    ra = call_a()
    sweep(c, call_b, release_b, equal_b, 1, width_b)
    assert equal_a(call_a(), ra)
    release_a()
    assert c.owned() == owned0
