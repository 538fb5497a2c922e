"""CPU tests of the low-rank update / downdate of the factors of a batch (include/spllt_hip_updown_batch.h,
batch_updown.hip): the interpreter of tests/updown_batch_emulate.py (the interpreter of updown_emulate.py per
member, driven by the library's plan, with the identity-exit rule) against a dense Cholesky of P (A_b +- W_b W_b^T)
P^T at the project's L-parity bar (1e-12 of max|L|); the exit rule changes no number; off a member's own path nothing
is written; the entry ladder without a device; the Python argument checks; the staging function under the host
sanitizers."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import capi_ladder
import updown_batch_emulate as bem
import updown_batch_ladder as ladder
import updown_emulate as em
from batch_emulate import member_values
from helpers import dense_arena, lower_mask, make_case, rel_err, sym_tables
from spllt_amd import _lib, api, matgen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spllt_hip_updown_batch.h")
BAR = 1e-12
CASES = {
    "p2d12": (lambda: matgen.poisson2d(12), dict(nb=16, nemin=4)),
    "box5": (lambda: matgen.nd_like((5, 5, 4), 1), dict(nb=16)),      # nodes of several block columns
}
NB = 3


@functools.lru_cache(maxsize=None)
def _case(name):
    """A, a handle (analysis only), the tables, the mask, per member (A_b, dense arena of A_b)"""
    gen, kw = CASES[name]
    A = sp.csc_matrix(gen())
    f, _ = make_case(A, **kw)
    members = []
    for b in range(NB):
        Ab, _vb = member_values(A, b, f.ptr, f.row)
        members.append((sp.csc_matrix(Ab), dense_arena(f, Ab)))
    return A, f, sym_tables(f), lower_mask(f), members


def _scaled(W, B):
    """member b's values on the pattern of W: W's own, scaled by 0.5 + 0.25 b"""
    W = bem.canonical(W)
    return np.stack([W.data * (0.5 + 0.25 * b) for b in range(B)])


def test_interface_exists_in_every_layer():
    names = set(re.findall(r"^int\s+(spllt_hip_\w+)\s*\(", open(HEADER).read(), re.M))
    assert len(names) == 5 and names == set(_lib.BATCH_UPDOWN_SYMBOLS) == set(_lib._BATCH_UPDOWN)
    lib = _lib.load()
    for s in names:
        getattr(lib, s)
    assert not names & set(_lib.PROTOTYPES)                    # (PROTOTYPES stays the two older headers)
    for m in ("update_batch", "update_batch_dev", "updown_batch_info", "updown_batch_device_ms", "release_updown_batch"):
        assert callable(getattr(api.Factorization, m))


@pytest.mark.parametrize("k", [1, 3, 9])
@pytest.mark.parametrize("name", list(CASES))
def test_interpreter_matches_a_dense_cholesky_per_member(name, k):
    A, f, t, mask, members = _case(name)
    W = em.edge_columns(A, k, np.random.default_rng(11 * k + len(name)))
    vals = _scaled(W, NB)
    arenas = [L.copy() for _, L in members]
    flags, written = bem.updown_batch(t, f, arenas, W, vals, +1)
    assert flags == [0] * NB
    plan_all = set(f.updown_plan(W).tolist())
    worst_up = worst_back = 0.0
    for b, (Ab, L0) in enumerate(members):
        Wb = bem.member_matrix(W, vals[b])
        worst_up = max(worst_up, rel_err(arenas[b], dense_arena(f, Ab + Wb @ Wb.T), mask))
        assert written[b] <= plan_all
    flags, _ = bem.updown_batch(t, f, arenas, W, vals, -1)
    assert flags == [0] * NB
    for b, (Ab, L0) in enumerate(members):
        worst_back = max(worst_back, rel_err(arenas[b], L0, mask))
    print(name, k, "update", worst_up, "update then downdate", worst_back)
    assert worst_up <= BAR and worst_back <= BAR
    assert len(bem.passes(f, W)) == -(-k // 8)


@pytest.mark.parametrize("name", list(CASES))
def test_the_exit_rule_changes_no_number(name):
    """with and without the identity exit the arenas are equal as numbers (a zero may change its sign where an
    identity rotation is skipped instead of applied)"""
    A, f, t, mask, members = _case(name)
    W = em.edge_columns(A, 9, np.random.default_rng(5))
    for vals in (_scaled(W, NB), bem.leave_one_out(W, [1.0, 0.75, 1.25], NB)):
        a = [L.copy() for _, L in members]
        b = [L.copy() for _, L in members]
        fa, wa = bem.updown_batch(t, f, a, W, vals, +1, exit_rule=True)
        fb, wb = bem.updown_batch(t, f, b, W, vals, +1, exit_rule=False)
        assert fa == fb == [0] * NB
        for m in range(NB):
            assert np.array_equal(a[m], b[m])
            assert wa[m] <= wb[m]


@pytest.mark.parametrize("name", list(CASES))
def test_leave_one_out_writes_a_members_own_path_only(name):
    A, f, t, mask, members = _case(name)
    k = 3
    W = em.edge_columns(A, k, np.random.default_rng(23))
    Wc = bem.canonical(W)
    vals = bem.leave_one_out(W, [1.0, 0.75, 1.25], NB)
    arenas = [L.copy() for _, L in members]
    flags, written = bem.updown_batch(t, f, arenas, W, vals, +1)
    assert flags == [0] * NB
    union = set(f.updown_plan(W).tolist())
    some_smaller = False
    for b, (Ab, L0) in enumerate(members):
        own = set(f.updown_plan(Wc[:, [b % k]]).tolist())
        assert written[b] == own and own <= union
        some_smaller |= own < union
        for c in range(len(t["bcol_off"])):
            if c not in own:
                off, nr, w = int(t["bcol_off"][c]), int(t["bcol_nrow"][c]), int(t["bcol_width"][c])
                assert np.array_equal(arenas[b][off:off + nr * w].view(np.uint64), L0[off:off + nr * w].view(np.uint64)), (b, c)
        Wb = bem.member_matrix(W, vals[b])
        assert rel_err(arenas[b], dense_arena(f, Ab + Wb @ Wb.T), mask) <= BAR
    assert some_smaller, "the case is meant to have a member whose own path is shorter than the union"


def test_interpreter_flags_a_failed_member_and_skips_its_later_passes():
    A, f, t, mask, members = _case("p2d12")
    i = 17
    k = 9                                   # two passes; the failure is in the first
    W = sp.csc_matrix((np.ones(k), (np.full(k, i), np.arange(k))), shape=(f.n, k))
    vals = np.full((NB, k), 0.01)
    vals[1, 0] = np.sqrt(2.0 * members[1][0][i, i])
    arenas = [L.copy() for _, L in members]
    flags, written = bem.updown_batch(t, f, arenas, W, vals, -1)
    assert flags[0] == 0 and flags[2] == 0 and flags[1] == int(t["order"][i]) + 1
    # an already flagged member is not touched at all
    arenas2 = [L.copy() for _, L in members]
    flags2, written2 = bem.updown_batch(t, f, arenas2, W, vals, -1, flags=[0, 5, 0])
    assert flags2[1] == 5 and not written2[1]
    assert np.array_equal(arenas2[1].view(np.uint64), members[1][1].view(np.uint64))


@pytest.mark.parametrize("state", capi_ladder.CPU_STATES)
def test_ladder_without_a_device(state):
    c = capi_ladder.Ctx(_lib.load(), False)
    assert ladder.check_state(c, state, ladder.golden(False)) == ladder.ROWS


def test_python_argument_checks():
    A, f, t, mask, members = _case("p2d12")
    n = f.n
    W = em.edge_columns(A, 3, np.random.default_rng(1))
    nent = bem.canonical(W).nnz
    with pytest.raises(ValueError, match="scipy sparse"):
        f.update_batch(np.ones((n, 1)))
    with pytest.raises(ValueError, match="rows"):
        f.update_batch(sp.csc_matrix((n + 1, 1)))
    with pytest.raises(ValueError, match="shape"):
        f.update_batch(W, vals=np.ones((2, nent + 1)))
    with pytest.raises(ValueError, match="shape"):
        f.update_batch(W, vals=np.ones(nent))
    with pytest.raises(ValueError, match="ldw"):
        f.update_batch_dev(W, 0, nent - 1)
    # on a handle without a batch the library refuses, with the name of the entry point
    with pytest.raises(api.SplltError) as ei:
        f.update_batch(W, vals=np.ones((2, nent)))
    assert ei.value.flag == -10 and "no batch" in str(ei.value)
    assert f.updown_batch_info() == dict(bcols=0, entries=0, launches=0, passes=0, served=0, failed=0)
    assert f.updown_batch_device_ms() == 0.0
    f.release_updown_batch()


def test_partitioned_handle_is_unimplemented():
    g, _ = make_case(matgen.poisson2d(16), nb=16, nemin=8, prune=True, ncpu=2)
    g.set_partition(0, 2)
    W = sp.csc_matrix(([1.0], ([0], [0])), shape=(g.n, 1))
    with pytest.raises(api.SplltError) as ei:
        g.update_batch(W, vals=np.ones((1, 1)))
    assert ei.value.flag == -98
    g.close()


CLANG_CANDIDATES = ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++")


def test_staging_function_under_the_host_sanitizers(tmp_path):
    clang = next((c for c in CLANG_CANDIDATES if os.path.exists(c)), None)
    if clang is None:
        pytest.skip("no ROCm clang++ on this machine")
    exe = str(tmp_path / "updown_stage_test")
    cmd = [clang, "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "spllt_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "updown_stage_test.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and ("asan" in built.stderr or "ubsan" in built.stderr) and "cannot find" in built.stderr:
        pytest.skip("the sanitizer runtime of the ROCm clang is not installed: " + built.stderr.strip().splitlines()[-1])
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    assert "updown_stage_test: ok" in ran.stdout
