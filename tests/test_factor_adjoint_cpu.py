"""CPU tests of the factor adjoint (spllt_hip_factor_adjoint): the sweep over the selected-inversion program
is interpreted in numpy (tests/factor_adjoint_emulate.py) on an L from an independent LAPACK Cholesky and compared
with the dense formula, with (2 - delta) inv(A) for the seed of log det, and with torch's CPU autograd of the dense
operations for the four seeds of the uses."""
import ctypes as C
import functools

import numpy as np
import pytest

import factor_adjoint_emulate as fe
from helpers import dense_arena, lower_mask, make_case
from selinv_emulate import check_order, expected_z, panel_inverses, selinv_tables
from spllt_amd import api, matgen

# The sweep is backward stable like the substitutions it consists of; on these well-conditioned matrices
# (cond <= 2e3) the dense formula itself is good to a few 1e-16 per entry, the bar of the emulated selected
# inversion against numpy's inverse (tests/test_selinv_batch_cpu.py) leaves room for both.
BAR = 1e-13

IDS = [c[0] for c in fe.CASES]


@functools.lru_cache(maxsize=None)
def _setup(name):
    """the case, its emulator inputs and its dense references: computed once, shared, never modified"""
    _, gen, nb, nemin, pw = fe.CASES[IDS.index(name)]
    A = gen()
    f, val = make_case(A, nb=nb, nemin=nemin, panel_width=pw)
    t = selinv_tables(f)
    L = dense_arena(f, A)
    return dict(A=A, f=f, val=val, t=t, L=L, dinv=panel_inverses(f, L, t), mask=lower_mask(f),
                Ld=fe.dense_from_arena(f, L))


@pytest.mark.parametrize("name", IDS)
def test_emulated_sweep_matches_the_dense_formula(name):
    c = _setup(name)
    f, L, mask = c["f"], c["L"], c["mask"]
    rng = np.random.default_rng(5)
    seeds = {"random": np.where(mask, rng.standard_normal(L.shape), 0.0),
             "rank3": fe.outer_seed(f, rng.standard_normal((f.n, 3)), rng.standard_normal((f.n, 3)), 0.7)}
    for what, seed in seeds.items():
        G = fe.emulate_factor_adjoint(f, L, c["dinv"], seed, c["t"])
        assert np.isfinite(G[mask]).all(), "an entry outside the lower pattern was read"
        err = fe.rel(G, fe.dense_factor_adjoint(f, c["Ld"], seed), mask)
        print(f"{name} {what}: {err:.2e}")
        assert err <= BAR, (what, err)
    # the seed of log det A: (2 - delta_ij) (A^-1)_ij on the WHOLE pattern of L
    G = fe.emulate_factor_adjoint(f, L, c["dinv"], fe.logdet_seed(f, L), c["t"])
    weight = np.full(L.shape, 2.0)
    weight[f.program("selinv_diag")] = 1.0
    err = fe.rel(G, weight * expected_z(f, c["A"]), mask)
    print(f"{name} logdet against (2 - delta) inv(A): {err:.2e}")
    assert err <= BAR, err


def _dense_matrix(val, prow, pcol, porder, n):
    """P A(val) P^T as a torch expression of val (a stored lower entry stands for a_ij and a_ji)"""
    import torch
    A = torch.zeros((n, n), dtype=torch.float64)
    A = A.index_put((prow, pcol), val).index_put((pcol, prow), val)
    return A[porder][:, porder]


@pytest.mark.parametrize("name", ["p2d12-nb4", "fe27-nb64"])
@pytest.mark.parametrize("op", ["L", "Lt", "Linv", "Ltinv"])
def test_the_four_seeds_against_dense_autograd(name, op):
    """loss = sum(gbar * op(L) x) for pivot-order vectors: d loss / d val from the seed of the table, swept by the
    emulator and read at A's entries, against torch's CPU autograd through torch.linalg.cholesky"""
    import torch
    c = _setup(name)
    f, L = c["f"], c["L"]
    n = f.n
    rng = np.random.default_rng(11)
    x, gbar = rng.standard_normal((n, 3)), rng.standard_normal((n, 3))
    prow, pcol = (torch.as_tensor(np.asarray(v, dtype=np.int64)) for v in f.pattern_tables())
    porder = np.empty(n, dtype=np.int64)
    porder[f.sym("order")] = np.arange(n)
    val = torch.tensor(c["val"], dtype=torch.float64, requires_grad=True)
    Lt = torch.linalg.cholesky(_dense_matrix(val, prow, pcol, torch.as_tensor(porder), n))
    xt = torch.as_tensor(x)
    y = {"L": lambda: Lt @ xt, "Lt": lambda: Lt.T @ xt,
         "Linv": lambda: torch.linalg.solve_triangular(Lt, xt, upper=False),
         "Ltinv": lambda: torch.linalg.solve_triangular(Lt.T, xt, upper=True)}[op]()
    (y * torch.as_tensor(gbar)).sum().backward()
    Ld, yn = c["Ld"], y.detach().numpy()
    if op == "L":
        seed = fe.outer_seed(f, gbar, x)
    elif op == "Lt":
        seed = fe.outer_seed(f, x, gbar)
    elif op == "Linv":
        seed = fe.outer_seed(f, np.linalg.solve(Ld.T, gbar), yn, -1.0)
    else:
        seed = fe.outer_seed(f, yn, np.linalg.solve(Ld, gbar), -1.0)
    got = fe.on_pattern(f, fe.emulate_factor_adjoint(f, L, c["dinv"], seed, c["t"]))
    want = val.grad.numpy()
    err = float(np.abs(got - want).max() / np.abs(want).max())
    print(f"{name} {op}: {err:.2e}")
    assert err <= BAR, err


@pytest.mark.parametrize("name", ["p2d16-nb8-pw32", "box11-nb100-pw48"])
def test_adjoint_launches_order_every_gather(name):
    """every entry of G_RR a SYMM launch gathers was made final by an EARLIER launch, and what SCALE and DIAG read
    of their own panel is still the seed; the check catches a sweep whose last gather runs one step too early"""
    c = _setup(name)
    f = c["f"]
    trace = []
    fe.emulate_factor_adjoint(f, c["L"], c["dinv"], fe.logdet_seed(f, c["L"]), c["t"], trace)
    arena = f.sym_info()["arena"]
    access = [(w, r) for w, r, _ in trace]
    assert check_order(access, arena) == []
    assert any(r.size for _, r in access), "expected gathers in this case"
    written = np.zeros(arena, dtype=bool)
    for w, _, own in trace:
        assert not written[own].any(), "a panel was swept twice"
        written[w] = True
    assert (written == c["mask"]).all(), "the sweep writes exactly the lower positions"
    k = max(i for i, (_, r) in enumerate(access) if r.size)
    j = max(i for i in range(k) if access[i][0].size)
    mutated = access[:j] + [access[k]] + access[j:k] + access[k + 1:]
    assert check_order(mutated, arena) != []


def test_the_k_slice_case_has_a_split_unit():
    """the GPU tests rely on fe.KSLICE_CASE for the sum of the K slices: it has a unit with nsplit >= 2 (nR > 256)"""
    u = _setup(fe.KSLICE_CASE)["t"]["units"]
    split = u[u["nsplit"] >= 2]
    assert len(split) and (split["nR"] > 256).all(), (int(u["nsplit"].max()), int(u["nR"].max()))


def test_errors_that_need_no_device():
    f, val = make_case(matgen.poisson2d(8), nb=8, nemin=4)
    lib, n = f.lib, f.n
    x = np.zeros(2 * n + 4)
    p = api._dp(x)
    addr = C.c_void_p(x.ctypes.data)
    seed, seed_dev = lib.spllt_hip_factor_adjoint_seed, lib.spllt_hip_factor_adjoint_seed_dev
    assert seed(f.fkeep, 1, None, p, n, 1.0, 0, 0) == -10 and "null" in f.last_error()
    assert seed(f.fkeep, 1, p, None, n, 1.0, 0, 0) == -10
    assert seed(f.fkeep, -1, p, p, n, 1.0, 0, 0) == -10 and "nvec" in f.last_error()
    assert seed(f.fkeep, 2, p, p, n - 1, 1.0, 0, 0) == -10 and "ld < n" in f.last_error()
    assert seed(f.fkeep, 1, p, p, n, 1.0, 2, 0) == -10 and "accumulate" in f.last_error()
    assert seed(f.fkeep, 1, p, p, n, 1.0, 0, 4) == -10 and "order_flags" in f.last_error()
    assert seed_dev(f.fkeep, 1, None, addr, n, 1.0, 0, 0) == -10
    assert seed_dev(f.fkeep, 1, addr, addr, n - 1, 1.0, 0, 3) == -10
    assert seed(None, 1, p, p, n, 1.0, 0, 0) == -10
    assert lib.spllt_hip_set_factor_adjoint(f.fkeep, None, 10) == -10
    assert lib.spllt_hip_set_factor_adjoint(f.fkeep, p, 0) == -10 and "arena" in f.last_error()
    assert lib.spllt_hip_get_factor_adjoint(f.fkeep, None, 10) == -10
    assert lib.spllt_hip_factor_adjoint(f.fkeep, None) == -10 and "null" in f.last_error()
    assert lib.spllt_hip_factor_adjoint_dev(f.fkeep, None) == -10
    assert not lib.spllt_hip_device_factor_adjoint(f.fkeep)
    assert lib.spllt_hip_release_factor_adjoint(f.fkeep) == 0
    assert lib.spllt_hip_release_factor_adjoint(None) == -10
    with pytest.raises(ValueError):
        f.factor_adjoint_seed(np.zeros((n, 2)), np.zeros((n, 3)))
    f.close()


def test_partitioned_handle_is_unimplemented_without_a_device():
    f, val = make_case(matgen.poisson2d(16), nb=16, nemin=8, prune=True, ncpu=2)
    f.set_partition(0, 2)
    v = np.zeros(f.n)
    for call in (lambda: f.factor_adjoint_seed(v, v), f.factor_adjoint, f.get_factor_adjoint,
                 lambda: f.set_factor_adjoint(np.zeros(f.sym_info()["arena"])),
                 lambda: f.factor_adjoint_seed_dev(v.ctypes.data, v.ctypes.data, 1),
                 lambda: f.factor_adjoint_dev(v.ctypes.data)):
        with pytest.raises(api.SplltError) as ei:
            call()
        assert ei.value.flag == -98 and "partitioned" in f.last_error()
    f.close()
