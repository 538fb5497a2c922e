"""GPU tests of the bit-reproducible batch (include/spllt_hip_batch_repro.h, batch_repro.hip): the deterministic
batch factorization and the reproducible blocked sweep.

Accuracy bars are those of the default batch: the factor against the default batch factor at rtol = atol = 1e-12 and
against the CPU oracle at rel_err <= 1e-12 (TOL_L of tests/test_factor_batch_gpu.py), log det at 1e-12 relative, the
sweep at a scaled backward error of 1e-14 per vector against the member's own A_b and rtol = atol = 1e-12 against
solve_batch (tests/test_solve_many_batch_gpu.py).  Bit identity is compared with tobytes(), with the NaN poison of
both scratches on for the whole module.

Cases: those of tests/test_batch_mult_gpu.py, except that p2d12-nb8 has no block column with two strips (the
backward hazard, tests/test_batch_repro_cpu.py) and is replaced by the next larger one, p2d40-nb16.  No test provokes
a device fault: the "bad" member is a flagged member, which every kernel skips."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import batch_repro_ladder as ladder
import capi_ladder
from batch_repro_emulate import CASES
from helpers import bwd_err, lower_mask, make_case, oracle_factor, rel_err
from spllt_amd import _lib, api

pytestmark = pytest.mark.gpu

NAMES = [c[0] for c in CASES]
NBATCH = [1, 3, 5]
NRHS = [1, 16, 17, 33, 40]
NV = 40


class Case:
    """a handle of its own per case; the members of tests/test_batch_mult_gpu.py"""

    def __init__(self, name, fresh=False):
        _, gen, nb, nemin = next(c for c in CASES if c[0] == name)
        self.name, self.A = name, sp.csc_matrix(gen())
        self.f, self.val = make_case(self.A, nb=nb, nemin=nemin)
        self.n = self.f.n
        self.diag = np.array([self.f.ptr[j] - 1 for j in range(self.n)])
        self.mask = None if fresh else lower_mask(self.f)

    def value(self, b, bad=False):
        """member b: (1 + 0.1 b) val plus 0.05 b on the diagonal; bad: one negative diagonal entry"""
        v = (1 + 0.1 * b) * self.val
        v[self.diag] += 0.05 * b
        if bad:
            v[self.diag[self.n // 2]] *= -1.0
        return v

    def values(self, members, bad=None):
        return np.stack([self.value(b, b == bad) for b in members])

    def member(self, b):
        return ((1 + 0.1 * b) * self.A + 0.05 * b * sp.identity(self.n)).tocsc()

    def rhs(self, members):
        """(len(members), NV, n): B_b = A_b X for one random X, so that the solutions are O(1)"""
        X = np.random.default_rng(2).standard_normal((NV, self.n))
        return np.ascontiguousarray(np.stack([(self.member(b) @ X.T).T for b in members]))


@functools.lru_cache(maxsize=None)
def _case(name):
    return Case(name)


@pytest.fixture(autouse=True)
def _poison_and_clean_switches():
    """every test runs with both scratches full of NaN before every factorization and sweep; the process-wide
    hooks and the handles' switches are as they were afterwards"""
    lib = _lib.load()
    assert lib.spllt_hip_debug(b"batch_repro_poison=1") == 0
    yield
    assert lib.spllt_hip_debug(b"batch_repro_poison=0") == 0
    assert lib.spllt_hip_debug(b"batch_grid_limit=0") == 0
    for c in _CASES_SEEN:
        c.f.set_batch_reproducible(False)


_CASES_SEEN = []


def _on(c):
    if c not in _CASES_SEEN:
        _CASES_SEEN.append(c)
    c.f.set_batch_reproducible(True)
    return c.f


def _state(c, members, place, B, bad=None):
    """factor the batch of `members` with the switch on; (rc, arena, log det, solutions of B for job 0 / 1 / 2) of the
    member at `place`, as bytes"""
    f = _on(c)
    rc = f.factor_batch(c.values(members, bad))
    Bm = np.ascontiguousarray(np.broadcast_to(B, (len(members),) + B.shape))
    sols = tuple(f.solve_batch(Bm, job)[place].tobytes() for job in (0, 1, 2))
    return rc, f.get_factor_batch(place).tobytes(), f.log_det_batch()[place].tobytes(), sols


# ---- accuracy ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbatch", NBATCH)
@pytest.mark.parametrize("name", NAMES)
def test_accuracy(name, nbatch):
    c = _case(name)
    f, members = c.f, list(range(nbatch))
    vals, B = c.values(members), c.rhs(members)
    f.set_batch_reproducible(False)
    assert f.factor_batch(vals) == 0
    assert f.batch_repro_info()["deterministic_factor"] == 0
    arena0 = [f.get_factor_batch(b) for b in members]
    ld0 = f.log_det_batch()
    x0 = {job: f.solve_batch(B, job) for job in (0, 1, 2)}
    _on(c)
    assert f.factor_batch(vals) == 0
    info = f.batch_repro_info()
    assert info["on"] == 1 and info["deterministic_factor"] == 1 and info["factor_launches"] == f.batch_launches() > 0
    assert info["factor_scratch_bytes"] >= nbatch * 8 * f.program("batch_det_scratch_size")
    for b in members:
        got = f.get_factor_batch(b)
        np.testing.assert_allclose(got[c.mask], arena0[b][c.mask], rtol=1e-12, atol=1e-12)
        o, rc = oracle_factor(f, vals[b])
        assert rc == 0
        err = rel_err(got, o.arena(), c.mask)
        print("accuracy", name, "nbatch", nbatch, "member", b, "rel_err vs oracle", err)
        assert err <= 1e-12
    ld = f.log_det_batch()
    assert (np.abs(ld - ld0) <= 1e-12 * np.maximum(1.0, np.abs(ld0))).all(), (ld, ld0)
    for nrhs in NRHS:
        for job in (0, 1, 2):
            Bq = B[:, :nrhs] if nrhs > 1 else B[:, 0]
            got = f.solve_reproducible_batch(Bq, job).reshape(nbatch, nrhs, c.n)
            assert np.isfinite(got).all()
            np.testing.assert_allclose(got, x0[job][:, :nrhs], rtol=1e-12, atol=1e-12)
            if job == 0:
                worst = max(bwd_err(c.member(b), got[b, q], B[b, q]) for b in members for q in range(nrhs))
                print("accuracy", name, "nbatch", nbatch, "nrhs", nrhs, "max scaled backward error", worst)
                assert worst <= 1e-14
        assert f.batch_repro_info()["sweep_rb"] in (16, 32)
    assert f.batch_repro_info()["sweep_scratch_bytes"] > 0


# ---- bit identity -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_a_members_bits_do_not_depend_on_the_batch_the_grid_or_the_run(name, monkeypatch):
    c = _case(name)
    lib = c.f.lib
    T = 4                                   # the member that is followed through the batches
    B = c.rhs([T])[0][:17]
    ref = _state(c, [T], 0, B)              # a batch of 1
    assert ref[0] == 0 and np.isfinite(np.frombuffer(ref[3][0])).all()
    assert _state(c, [T], 0, B) == ref      # the same call again
    assert _state(c, [T, 1, 2], 0, B) == ref               # place 0 of 3
    assert _state(c, [0, 1, 2, 3, T], 4, B) == ref         # place 4 of 5
    for limit in (1, 100):                  # the members split into ranges: one per launch, then a few
        assert lib.spllt_hip_debug(b"batch_grid_limit=%d" % limit) == 0
        assert _state(c, [0, 1, 2, 3, T], 4, B) == ref, limit
        assert _state(c, [T, 1, 2], 0, B) == ref, limit
    assert lib.spllt_hip_debug(b"batch_grid_limit=0") == 0
    # two fresh handles, the second with the other grid mapping (read once per engine)
    for member_fast in ("0", "1"):
        monkeypatch.setenv("SPLLT_BATCH_MEMBER_FAST", member_fast)
        fresh = Case(name, fresh=True)
        try:
            assert _state(fresh, [0, 1, 2, 3, T], 4, B) == ref, member_fast
            assert _state(fresh, [T], 0, B) == ref, member_fast
        finally:
            _CASES_SEEN.remove(fresh)
            fresh.f.close()


@pytest.mark.parametrize("name", NAMES)
def test_a_vectors_bits_do_not_depend_on_its_block_or_the_entry_point(name):
    import torch
    c = _case(name)
    f, members, n = _on(c), [0, 1, 2], c.n
    assert f.factor_batch(c.values(members)) == 0
    B = c.rhs(members)
    for job in (0, 1, 2):
        x = f.solve_reproducible_batch(B, job)                               # 40 per member: blocks of 32 and 16
        assert np.isfinite(x).all()
        for q in (0, 20, 37):                                                # alone: a block of 16
            assert f.solve_reproducible_batch(B[:, q], job).tobytes() == np.ascontiguousarray(x[:, q]).tobytes(), (job, q)
        assert f.solve_reproducible_batch(B[:, :17], job).tobytes() == np.ascontiguousarray(x[:, :17]).tobytes()
        perm = np.random.default_rng(1).permutation(NV)                      # its place in the block
        assert f.solve_reproducible_batch(B[:, perm], job).tobytes() == np.ascontiguousarray(x[:, perm]).tobytes()
        # the switch on: solve_batch and solve_many_batch are the same sweep
        assert f.solve_batch(B, job).tobytes() == x.tobytes()
        assert f.solve_many_batch(B, job).tobytes() == x.tobytes()
        # the device entry points
        for call in (f.solve_reproducible_batch_dev, f.solve_batch_dev, f.solve_many_batch_dev):
            xd = torch.tensor(B, device="cuda")
            torch.cuda.synchronize()
            assert call(xd.data_ptr(), NV, job=job) == 0
            assert xd.cpu().numpy().tobytes() == x.tobytes(), (job, call.__name__)
        # the switch off: the entry point of its own still runs the reproducible sweep on the same factors
        f.set_batch_reproducible(False)
        assert f.batch_repro_info()["on"] == 0 and f.batch_repro_info()["deterministic_factor"] == 1
        assert f.solve_reproducible_batch(B, job).tobytes() == x.tobytes()
        f.set_batch_reproducible(True)
    # blocks of 16 only (what is left when the scratch of 32 does not fit): the same bits
    x = f.solve_reproducible_batch(B, 0)
    f.release_batch_repro()
    f.release_solve_many_batch()
    assert f.batch_repro_info()["sweep_scratch_bytes"] == 0
    assert f.lib.spllt_hip_debug(b"fmult_alloc_fail=1") == 0
    try:
        x16 = f.solve_reproducible_batch(B, 0)
    finally:
        assert f.lib.spllt_hip_debug(b"fmult_alloc_fail=0") == 0
    assert f.batch_repro_info()["sweep_rb"] == 16 and x16.tobytes() == x.tobytes()
    f.release_batch_repro()
    f.release_solve_many_batch()
    assert f.solve_reproducible_batch(B, 0).tobytes() == x.tobytes()


# ---- routing ----------------------------------------------------------------------------------------
def test_every_batch_sweep_is_routed_and_repeats():
    c = _case("box11-nb64")
    f, members, n = _on(c), [0, 1, 2], c.n
    vals = c.values(members)
    B = c.rhs(members)[:, :5]
    Crows = np.random.default_rng(5).standard_normal((3, n))

    def run():
        assert f.factor_batch(vals) == 0
        f.set_constraints_batch(Crows)
        xc, lam = f.solve_constrained_batch(B, multipliers=True)
        s = f.sample_batch(6, seed=11, kind="precision")
        xr, it, err = f.solve_refined_batch(vals, B)
        return xc.tobytes(), lam.tobytes(), s.tobytes(), xr.tobytes(), it.tobytes(), err.tobytes()

    first = run()
    info = f.batch_repro_info()
    assert info["deterministic_factor"] == 1 and info["sweep_rb"] in (16, 32)
    assert all(np.isfinite(np.frombuffer(b)).all() for b in first[:4])
    assert run() == first
    f.set_constraints_batch(None)


@pytest.mark.parametrize("name", NAMES)
def test_the_switch_off_launches_what_the_default_batch_launches(name):
    c = _case(name)
    f, members = c.f, [0, 1, 2]
    f.set_batch_reproducible(False)
    assert f.factor_batch(c.values(members)) == 0
    launches = f.program("batch_launches")
    assert f.batch_launches() == 1 + int((launches[:, 3] > 0).sum())          # the init launch + one per launch
    assert f.batch_repro_info()["deterministic_factor"] == 0
    f.solve_many_batch(c.rhs(members), 0)                                      # 40 per member: two blocks
    per_block = 2 + sum(int((f.program(k)[:, 3] > 0).sum()) for k in ("solve_fwd", "solve_bwd"))
    assert f.solve_many_batch_info()["launches"] == 2 * per_block
    # ... and the deterministic program adds its gather launches
    _on(c)
    assert f.factor_batch(c.values(members)) == 0
    det = f.program("batch_det_launches")
    assert f.batch_launches() == 1 + int((det[:, 3] > 0).sum()) > 1 + int((launches[:, 3] > 0).sum())
    f.solve_many_batch(c.rhs(members), 0)
    assert f.solve_many_batch_info()["launches"] == 2 * per_block              # the reproducible sweep adds no launch


# ---- a flagged member -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_a_flagged_member_is_skipped_and_the_others_keep_their_bits(name):
    c = _case(name)
    f, n = _on(c), c.n
    B = c.rhs([0, 1, 2])[:, :17]
    assert f.factor_batch(c.values([0, 2])) == 0
    want = {job: f.solve_reproducible_batch(B[[0, 2]], job) for job in (0, 1, 2)}
    arenas = [f.get_factor_batch(0).tobytes(), f.get_factor_batch(1).tobytes()]
    ld = f.log_det_batch()
    assert f.factor_batch(c.values([0, 1, 2], bad=1)) == -20
    flags, cols = f.batch_status()
    assert list(flags) == [0, -20, 0]
    assert [f.get_factor_batch(0).tobytes(), f.get_factor_batch(2).tobytes()] == arenas
    got_ld = f.log_det_batch()
    assert np.isnan(got_ld[1]) and got_ld[[0, 2]].tobytes() == ld.tobytes()
    for job in (0, 1, 2):
        x = B.copy()
        rc = f.lib.spllt_hip_solve_repro_batch(f.fkeep, 17, x.ctypes.data, n, job)
        assert rc == -20 and "spllt_hip_solve_repro_batch: " in f.last_error() and "unchanged" in f.last_error()
        assert x[1].tobytes() == B[1].tobytes()
        assert x[[0, 2]].tobytes() == want[job].tobytes()
        got = f.solve_batch(B, job)                                            # (Python: no exception)
        assert got[1].tobytes() == B[1].tobytes() and got[[0, 2]].tobytes() == want[job].tobytes()


# ---- ladder -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", ["analysed", "engine", "factored", "batch", "batch_inverse"])
def test_ladder_on_the_gpu(state):
    cx = capi_ladder.Ctx(_lib.load(), True)
    assert ladder.check_state(cx, state, ladder.golden(True)) == ladder.ROWS


# ---- torch ------------------------------------------------------------------------------------------
def test_torch_batch_reproducible_repeats_forward_and_backward(monkeypatch):
    import torch
    from spllt_amd.torch_ops import SparseCholesky
    c = _case("box11-nb64")
    n, nbatch = c.n, 3
    calls = []
    real = api.Factorization.set_batch_reproducible
    monkeypatch.setattr(api.Factorization, "set_batch_reproducible", lambda self, on: (calls.append(on), real(self, on))[1])
    off = SparseCholesky(c.A, nb=64, nemin=16)
    assert calls == [] and off.batch_reproducible is False                     # off: the setter is never called
    only = SparseCholesky(c.A, nb=64, nemin=16, reproducible=True)
    assert calls == []
    vals0 = torch.tensor(c.values(range(nbatch)), device="cuda")
    B0 = torch.tensor(np.ascontiguousarray(c.rhs(range(nbatch))[:, :5].transpose(0, 2, 1)), device="cuda")
    for op in (lambda: only.solve_batch(vals0, B0), lambda: only.logdet_batch(vals0),
               lambda: only.sample_batch(vals0, 2, seed=1), lambda: only.rsample_batch(vals0, 2, seed=1)):
        with pytest.raises(NotImplementedError, match="batch_reproducible=True"):
            op()
    chol = SparseCholesky(c.A, nb=64, nemin=16, batch_reproducible=True)
    assert calls == [True] and chol.f.batch_repro_info()["on"] == 1

    def run():
        vals = vals0.clone().requires_grad_(True)
        B = B0.clone().requires_grad_(True)
        X = chol.solve_batch(vals, B)
        ld = chol.logdet_batch(vals)
        W = torch.cos(torch.arange(X.numel(), device="cuda", dtype=torch.float64)).reshape(X.shape)
        ((X * W).sum() + (ld * torch.arange(1, nbatch + 1, device="cuda", dtype=torch.float64)).sum()).backward()
        s = chol.sample_batch(vals.detach(), 3, seed=7)
        r = chol.rsample_batch(vals.detach(), 3, seed=7)
        torch.cuda.synchronize()
        return tuple(t.detach().cpu().numpy().tobytes() for t in (X, ld, vals.grad, B.grad, s, r))

    first = run()
    assert all(np.isfinite(np.frombuffer(b)).all() for b in first)
    assert run() == first
    assert chol.f.batch_repro_info()["deterministic_factor"] == 1
