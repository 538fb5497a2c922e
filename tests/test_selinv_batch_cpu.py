"""CPU tests of the batched selected inversion (spllt_hip_selected_inverse_batch and friends): the
interface exists in every layer; the batch's selected-inversion program ("batch_selinv_*", panels of 64
columns whatever the handle's panel width) reproduces the dense inverse of members of a batch when
tests/selinv_emulate.py interprets it; its dinv slots are where the batch's chain units write the panel
inverses; its launches order every gather; argument errors that need no device come back as stated."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from batch_emulate import member_matrix
from helpers import dense_arena, lower_mask, make_case, quintuple_hand_amalgamated, quintuple_single_columns, sym_tables
from selinv_emulate import SI_DIAG, check_order, emulate_selinv, expected_z, launch_access, panel_inverses
from spllt_amd import _lib, api, matgen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["spllt_hip_selected_inverse_batch", "spllt_hip_get_inverse_batch", "spllt_hip_device_inverse_batch",
           "spllt_hip_inverse_diag_batch", "spllt_hip_inverse_on_pattern_batch", "spllt_hip_batch_selinv_launches",
           "spllt_hip_release_inverse_batch", "spllt_hip_inverse_on_pattern"]
TABLES = ("units", "tiles", "launches", "rows", "relpos", "diag", "scratch")


def _forest():
    """three disconnected components of different shapes"""
    blocks = [matgen.poisson2d(6), matgen.poisson3d(3), sp.identity(5) * 3.0]
    return sp.block_diag(blocks, format="csc")


# the patterns of tests/test_selinv_cpu.py; every handle has a panel width other than the batch's 64
CASES = [
    ("p2d12-nb4", lambda: matgen.poisson2d(12), 4, 4, 32),
    ("p2d16-nb8", lambda: matgen.poisson2d(16), 8, 4, 16),
    ("p3d6-nb16", lambda: matgen.poisson3d(6), 16, 8, 32),
    ("box6-nb100", lambda: matgen.nd_like((6, 6, 6), 2), 100, 8, 32),          # nodes of several block columns
    ("box7-nb256", lambda: matgen.nd_like((7, 7, 6), 2), 256, 16, 32),         # block columns of several 64-panels
    ("box7-nb256-pw48", lambda: matgen.nd_like((7, 7, 6), 2), 256, 16, 48),
    ("p2d10-single-col", lambda: matgen.poisson2d(10), 8, 1, 32),               # nemin 1: single-column nodes
    ("diag", lambda: sp.diags(np.arange(1.0, 31.0)).tocsc(), 8, 4, 32),
    ("n1", lambda: sp.csc_matrix(np.array([[4.0]])), 8, 4, 32),
    ("forest", _forest, 8, 4, 32),
]


def batch_selinv_tables(f):
    return {k: f.program("batch_selinv_" + k) for k in TABLES}


def _check(f, A, members=(0, 1)):
    t = batch_selinv_tables(f)
    mask = lower_mask(f)
    for b in members:
        Ab = member_matrix(A, b)
        L = dense_arena(f, Ab)
        Z = emulate_selinv(f, L, panel_inverses(f, L, t), t)
        ref = expected_z(f, Ab)
        assert np.isfinite(Z[mask]).all(), "an entry of the pattern was read before it was written, or never written"
        err = float(np.abs(Z[mask] - ref[mask]).max() / np.abs(ref[mask]).max())
        assert err <= 1e-12, (b, err)
    return t


def test_interface_exists_in_every_layer():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "spllt_hip.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.HIP_SYMBOLS, name
        assert re.search(r"\b%s\s*\(" % name, header), name
    assert "batched selected inversion (single GPU)" in header
    for name in ("selected_inverse_batch", "get_inverse_batch", "device_inverse_batch_ptr", "inverse_diag_batch",
                 "inverse_on_pattern_batch", "batch_selinv_launches", "release_inverse_batch", "inverse_on_pattern"):
        assert callable(getattr(api.Factorization, name)), name
    assert lib.spllt_hip_inverse_diag_batch.argtypes[2] is C.c_int64
    assert lib.spllt_hip_debug(b"batch_selinv_fused=0") == 0 and lib.spllt_hip_debug(b"batch_selinv_fused=1") == 0
    assert lib.spllt_hip_debug(b"batch_selinv_fused=2") == -1


@pytest.mark.parametrize("name,gen,nb,nemin,pw", CASES, ids=[c[0] for c in CASES])
def test_batch_selinv_program_reproduces_the_inverse_of_members(name, gen, nb, nemin, pw):
    A = gen()
    f, _ = make_case(A, nb=nb, nemin=nemin, panel_width=pw)
    assert f.program("panel_width") == pw != 64
    t = _check(f, A)
    assert int(t["units"]["pn"].max()) <= 64 and t["scratch"] >= 0
    if name == "box6-nb100":
        assert (np.diff(sym_tables(f)["node_bcol0"]) > 1).any(), "expected nodes wider than one block column"
    if name.startswith("box7-nb256"):
        assert int(sym_tables(f)["bcol_width"].max()) > 64, "expected a block column of several 64-wide panels"
        assert int(t["units"]["pn"].max()) == 64
    if name == "p2d10-single-col":
        assert (np.diff(sym_tables(f)["sptr"]) == 1).any()
    f.close()


@pytest.mark.parametrize("kind", ["single", "amalgamated"])
def test_batch_selinv_program_on_foreign_symbolic(kind):
    A = matgen.poisson2d(11)
    f0, _ = make_case(A, nb=8, nemin=4)
    quint = quintuple_single_columns(f0) if kind == "single" else quintuple_hand_amalgamated(f0)
    n, ptr, row, val = api.csc_lower_1based(A)
    f = api.Factorization(n, ptr, row, nb=8, nemin=4, symbolic=quint, panel_width=32)
    assert f.sym_info()["ordering"] == "symbolic"
    _check(f, A)


def test_batch_tables_do_not_depend_on_the_handles_panel_width_or_engine_flags():
    gen = lambda: matgen.nd_like((7, 7, 6), 2)      # noqa: E731
    ref = None
    for pw, flags in ((32, 0), (64, 0), (48, 4096), (16, 2)):
        f, _ = make_case(gen(), nb=256, nemin=16, panel_width=pw, engine_flags=flags)
        tabs = [np.asarray(f.program("batch_selinv_" + k)).tobytes() for k in TABLES + ("flops",)]
        if ref is None:
            ref = tabs
            own = np.asarray(f.program("selinv_units")).tobytes()
            assert own != tabs[0], "the handle's own program has 32-wide panels"
        else:
            assert tabs == ref, (pw, flags)
        f.close()
    with pytest.raises(KeyError):
        f0, _ = make_case(matgen.poisson2d(8), nb=8, nemin=4)
        f0.program("batch_selinv_panels")


@pytest.mark.parametrize("name,gen,nb,nemin,pw", [CASES[i] for i in (1, 3, 4, 6, 9)], ids=[CASES[i][0] for i in (1, 3, 4, 6, 9)])
def test_dinv_slots_are_where_the_batch_chain_writes_them(name, gen, nb, nemin, pw):
    """k_batch_chain leaves inv(L_pp) of the panel of chain unit q at winv_off + (c0 - cs), row stride
    ce - cs (batch.hip): every unit of the batch's selinv program reads exactly that slot"""
    f, _ = make_case(gen(), nb=nb, nemin=nemin, panel_width=pw)
    slot = {(int(u["off"]), int(u["c0"])): (int(u["dinv_off"]), int(u["dinv_ld"]), int(u["pn"]))
            for u in f.program("batch_selinv_units")}
    launches, chains = f.program("batch_launches"), f.program("batch_chains")
    seen = set()
    for kind, _, first, count in launches[:, :4]:
        if kind != 4:
            continue
        for q in chains[first:first + count]:
            key = (int(q["off"]), int(q["c0"]))
            want = (int(q["winv_off"]) + int(q["c0"]) - int(q["cs"]), int(q["ce"]) - int(q["cs"]), int(q["pn"]))
            assert slot[key] == want, (key, slot[key], want)
            seen.add(key)
    assert seen == set(slot), "every panel of the inversion is a panel the batch factorization inverts"
    # ... and every slot lies inside a member's dinv area
    assert max(o + (pn - 1) * ld + pn for o, ld, pn in slot.values()) <= f.program("batch_dinv_size")
    f.close()


@pytest.mark.parametrize("name,gen,nb,nemin,pw", [CASES[1], CASES[3], CASES[9]], ids=[CASES[i][0] for i in (1, 3, 9)])
def test_batch_selinv_launches_order_every_gather(name, gen, nb, nemin, pw):
    """every Z entry a launch gathers was written by an earlier launch (so a fused step, which gathers and
    writes in one launch, never gathers what its own launch writes)"""
    f, _ = make_case(gen(), nb=nb, nemin=nemin, panel_width=pw)
    t = batch_selinv_tables(f)
    access = launch_access(f, t)
    arena = f.sym_info()["arena"]
    assert check_order(access, arena) == []
    assert any(r.size for _, r in access), "expected gathers in this case"
    # mutation: the last launch that gathers moves in front of the DIAG launch before it
    k = max(i for i, (_, r) in enumerate(access) if r.size)
    j = max(i for i in range(k) if access[i][0].size and t["launches"][i, 0] == SI_DIAG)
    mutated = access[:j] + [access[k]] + access[j:k] + access[k + 1:]
    assert check_order(mutated, arena) != []
    # every step ends with its DIAG launch and the DIAG launches cover the units in order
    launches = t["launches"]
    assert launches[-1, 0] == SI_DIAG
    d = launches[launches[:, 0] == SI_DIAG]
    assert (d[1:, 2] == d[:-1, 2] + d[:-1, 3]).all() and d[0, 2] == 0 and d[-1, 2] + d[-1, 3] == len(t["units"])
    f.close()


def test_argument_errors_on_an_analysed_handle():
    f, val = make_case(matgen.poisson2d(8), nb=8, nemin=4)
    n, nnz, lib = f.n, f.nnz, f.lib
    out = np.zeros(3 * max(nnz, f.sym_info()["arena"]) + 8)
    op = api._dp(out)
    # null handle / null pointer / too small a leading dimension
    assert lib.spllt_hip_selected_inverse_batch(None) == -10
    assert lib.spllt_hip_get_inverse_batch(None, 0, op, 4) == -10
    assert lib.spllt_hip_inverse_diag_batch(None, op, n) == -10
    assert lib.spllt_hip_inverse_on_pattern_batch(None, op, nnz) == -10
    assert lib.spllt_hip_batch_selinv_launches(None) == -10
    assert lib.spllt_hip_release_inverse_batch(None) == -10
    for fn, ld, word in ((lib.spllt_hip_inverse_diag_batch, n, "ldout < n"),
                         (lib.spllt_hip_inverse_on_pattern_batch, nnz, "ldout < nnz")):
        assert fn(f.fkeep, None, ld) == -10 and "null" in f.last_error()
        assert fn(f.fkeep, op, ld - 1) == -10 and word in f.last_error(), f.last_error()
        assert fn(f.fkeep, op, ld) == -10 and "no batch" in f.last_error()
    assert lib.spllt_hip_get_inverse_batch(f.fkeep, 0, None, 4) == -10 and "null" in f.last_error()
    assert lib.spllt_hip_get_inverse_batch(f.fkeep, 0, op, -1) == -10 and "count" in f.last_error()
    assert lib.spllt_hip_get_inverse_batch(f.fkeep, 0, op, 4) == -10 and "no batch" in f.last_error()
    assert lib.spllt_hip_selected_inverse_batch(f.fkeep) == -10 and "no batch" in f.last_error()
    stride = C.c_int64(5)
    assert lib.spllt_hip_device_inverse_batch(f.fkeep, C.byref(stride)) is None and stride.value == 0
    assert lib.spllt_hip_device_inverse_batch(None, C.byref(stride)) is None
    assert lib.spllt_hip_batch_selinv_launches(f.fkeep) == 0
    assert lib.spllt_hip_release_inverse_batch(f.fkeep) == 0
    assert lib.spllt_hip_inverse_on_pattern(f.fkeep, None) == -10
    assert lib.spllt_hip_inverse_on_pattern(f.fkeep, op) == -10       # nothing factorized on this handle
    assert (out == 0.0).all()
    for call in (f.selected_inverse_batch, f.inverse_diag_batch, f.inverse_on_pattern_batch,
                 lambda: f.get_inverse_batch(0), f.inverse_on_pattern):
        with pytest.raises(api.SplltError) as ei:
            call()
        assert ei.value.flag == -10
    assert f.device_inverse_batch_ptr() == (None, 0) and f.batch_selinv_launches() == 0
    f.release_inverse_batch()
    f.close()


def test_partitioned_handle_is_refused_without_a_device():
    f, val = make_case(matgen.poisson2d(16), nb=16, nemin=8, prune=True, ncpu=2)
    f.set_partition(0, 2)
    out = np.zeros(f.nnz + f.n)
    for call in (f.selected_inverse_batch, f.inverse_diag_batch, f.inverse_on_pattern_batch,
                 lambda: f.get_inverse_batch(0)):
        with pytest.raises(api.SplltError) as ei:
            call()
        assert ei.value.flag == -98 and "partitioned" in f.last_error()
    assert f.lib.spllt_hip_inverse_diag_batch(f.fkeep, api._dp(out), f.n) == -98
    f.close()
