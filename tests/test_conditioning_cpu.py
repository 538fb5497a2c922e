"""The inputs and the CPU references of tests/test_conditioning_gpu.py, pinned (no GPU needed): the bars of the
GPU tests are ratios to what is computed here, so it is checked here that
  * the longdouble reference is one (eta <= n 2^-63),
  * every input is safely positive definite for a backward-stable factorization (the oracle: rc == 0 and
    eta <= 32 u; the largest value met is 2.6e-16 = 2.3 u),
  * the ALGORITHM of the engine (inverse-multiply TRSM; tests/emulate.py in LAPACK arithmetic for the factor,
    hard_inputs.model_solve for the substitution) is as accurate as the oracle on the benign cases, and crosses
    the reference's own acceptance bar 1e-14 on the Hilbert-1e-10 family.  If a later
    change of the program makes the last assertion false, that is good news: the test is then updated,
  * the interpreter is exactly equivariant under power-of-two scaling (LAPACK arithmetic is, while nothing under-
    or overflows): this checks the generators and that the chosen exponents stay in range.
Run with -s to see the table of DESIGN.md section 20."""
import numpy as np
import pytest

import hard_inputs as hi
from emulate import emulate_program
from helpers import make_case
from spllt_amd import api

U = hi.U


@pytest.mark.parametrize("cid", hi.CASE_IDS)
def test_inputs_and_references(cid):
    A, b, f, val, pw, cls = hi.make(cid)
    r = hi.references(f, A, val, b, pw, key=cid)
    cond = np.linalg.cond(A.toarray())
    print(f"\n{cid}: n={f.n} cond2(A)={cond:.1e} max kappa2(L_pp)={r['kappa']:.1e} eta: longdouble {r['eta_ld']:.1e} "
          f"oracle {r['eta_oracle']:.1e} emulated {r['eta_emul']:.1e} (16-blocked panels {r['eta_emul16']:.1e}) "
          f"max|L_emul-L_oracle|/max|L|={r['fwd_emul']:.1e} omega: oracle {r['omega_oracle'].max():.1e} "
          f"model {r['omega_model'].max():.1e} eta_emul/(u kappa)={r['eta_emul'] / (U * r['kappa']):.1e}")
    assert r["eta_ld"] <= f.n * 2.0 ** -63
    assert r["rc_oracle"] == 0 and r["eta_oracle"] <= 32 * U
    if cls == "benign":
        assert r["eta_emul"] <= 32 * U
        assert r["omega_model"].max() <= 1e-14
    else:
        assert r["eta_emul"] > 1e-14
    f.close()


@pytest.mark.parametrize("cid", ["h200-s10-pw48", "h260-s10-nb256", "bih2d-20-nb100-pw40"])
def test_chain_block_model_is_the_one_panel_algorithm(cid, monkeypatch):
    """SPLLT_CHAIN4=1 (k_chain_block, k_trsm_rows): the interpreter's default (dpotrf of the whole chain block, true
    substitution below it) is backward stable where the kernels' algorithm is not; with
    chain_inverse_multiply=True it reproduces the one-panel-per-step program's error level on hard input."""
    A, b, f0, val, pw, cls = hi.make(cid)
    Ap = hi.permuted(f0, A)
    e0 = hi.eta(Ap, hi.dense_L(f0, emulate_program(f0, val)))
    monkeypatch.setenv("SPLLT_CHAIN4", "1")
    _, _, f, _, _, _ = hi.make(cid)
    kinds = f.program("launches")[:, 0]
    assert (kinds == 8).any() and (kinds == 9).any()
    e_lapack = hi.eta(Ap, hi.dense_L(f, emulate_program(f, val)))
    e_model = hi.eta(Ap, hi.dense_L(f, emulate_program(f, val, chain_inverse_multiply=True)))
    print(f"\n{cid}: eta one panel per step {e0:.1e}, chain blocks: dpotrf + substitution {e_lapack:.1e}, "
          f"inverse-multiply model {e_model:.1e}")
    assert e_lapack <= 32 * U
    assert e0 / 4 <= e_model <= 4 * e0 if cls == "hard" else e_model <= 32 * U
    f.close()
    f0.close()


def test_panel_chol16_is_a_cholesky_and_an_inverse():
    """the 16-blocked panel hook on a well-conditioned block: a factor and its inverse to rounding"""
    rng = np.random.default_rng(3)
    for n in (1, 16, 17, 48, 63, 64):
        B = rng.standard_normal((n, n))
        S = B @ B.T + n * np.eye(n)
        L, W = hi.panel_chol16(S)
        assert hi.eta(S, L) <= 32 * U and hi.inv_resid(L, W) <= 32 * U
        assert np.array_equal(L, np.tril(L)) and np.array_equal(W, np.tril(W))


@pytest.mark.parametrize("opts", range(len(hi.EQUI_OPTS)))
@pytest.mark.parametrize("base", range(len(hi.EQUI_BASES)))
def test_interpreter_is_exactly_equivariant_under_power_of_two_scaling(base, opts):
    name, gen = hi.EQUI_BASES[base]
    A = gen()
    f, val = make_case(A, **hi.EQUI_OPTS[opts])
    L0 = hi.dense_L(f, emulate_program(f, val))
    P = hi.pivot_perm(f)
    for kind in hi.EQUI_KINDS:
        e = hi.equi_scaling(kind, f.n, seed=11 + base)
        As = hi.graded(A, e)
        if kind != "graded":
            assert np.array_equal(As.toarray(), hi.scaled(A, 2 * int(e[0])).toarray())
        n, ptr, row, vs = api.csc_lower_1based(As)
        assert np.array_equal(ptr, f.ptr) and np.array_equal(row, f.row)
        Ls = hi.dense_L(f, emulate_program(f, vs))
        assert np.isfinite(Ls).all()
        assert np.array_equal(np.ldexp(Ls, -e[P][:, None].astype(np.int32)), L0), kind
    f.close()
