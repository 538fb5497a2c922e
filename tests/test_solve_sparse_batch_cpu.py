"""CPU tests of the sparse right-hand-side solves of a batch (include/spllt_hip_solve_sparse_batch.h,
batch_solve_sparse.hip): the header stands alone and its symbols are the library's and the table's; the entry ladder
without a device; the Python wrappers refuse wrong shapes before any library call; the interpreter of
tests/solve_sparse_batch_emulate.py (the BATCH's substitution program restricted to the library's plan, several value
sets at once, from vectors that are NaN outside the touched rows) against dense solves at the bars of
test_solve_sparse_cpu.py; the extracted slot / filter code under the host sanitizers."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.linalg as sl
import scipy.sparse as sp

import capi_ladder
import solve_sparse_batch_ladder as ladder
from batch_emulate import member_values
from helpers import dense_arena, make_case, sym_tables
from solve_sparse_batch_emulate import run_filtered_batch
from spllt_amd import _lib, api, matgen
from test_solve_sparse_cpu import CASES, _columns, _inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spllt_hip_solve_sparse_batch.h")
NB = 3
CLANG_CANDIDATES = ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++")


def test_header_and_tables(tmp_path):
    text = open(HEADER).read()
    names = set(re.findall(r"^int\s+(spllt_hip_\w+)\s*\(", text, re.M))
    assert len(names) == 6 and names == set(_lib.SOLVE_SPARSE_BATCH_SYMBOLS) == set(_lib._SOLVE_SPARSE_BATCH)
    lib = _lib.load()
    for s in names:
        getattr(lib, s)
    older = (_lib.PROTOTYPES, _lib._BATCH_MULT, _lib._BATCH_SOLVE_MANY, _lib._BATCH_ADJOINT, _lib._BATCH_REFINE,
             _lib._CONSTRAIN, _lib._CONSTRAIN_BATCH, _lib._BATCH_REPRO, _lib._BATCH_UPDOWN)
    for table in older:
        assert not names & set(table)
    # every exported symbol of the family is declared
    so = os.path.join(ROOT, "spllt_amd", "libspllt_hip.so")
    nm = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True)
    if nm.returncode == 0:
        exported = set(re.findall(r"\bT (spllt_hip_\w*sparse_batch\w*)", nm.stdout))
        assert exported == names, exported ^ names
    for m in ("solve_sparse_batch", "solve_sparse_batch_dev", "gram_batch", "gram_batch_dev", "inverse_block_batch",
              "solve_sparse_batch_info", "release_solve_sparse_batch"):
        assert callable(getattr(api.Factorization, m))
    assert "WHY A HEADER OF ITS OWN" in text and "folded into" in text
    # the header stands alone: a C and a C++ translation unit that include nothing else
    clang = next((c for c in CLANG_CANDIDATES if os.path.exists(c)), None)
    if clang is not None:
        for lang, ext in (("c", "c"), ("c++", "cpp")):
            src = tmp_path / f"alone.{ext}"
            src.write_text('#include "spllt_hip_solve_sparse_batch.h"\n'
                           "int (*p)(void *, int64_t *) = spllt_hip_solve_sparse_batch_info;\n")
            r = subprocess.run([clang, "-x", lang, "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                                str(src)], capture_output=True, text=True)
            assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("state", capi_ladder.CPU_STATES)
def test_ladder_without_a_device(state):
    c = capi_ladder.Ctx(_lib.load(), False)
    assert ladder.check_state(c, state, ladder.golden(False)) == ladder.ROWS


def test_python_wrappers_refuse_wrong_shapes():
    f, _ = make_case(matgen.poisson2d(8), nb=8, nemin=4)
    n = f.n
    B = sp.csc_matrix(([1.0, 2.0, 3.0], ([1, 4, 6], [0, 0, 1])), shape=(n, 2))
    calls = []
    real = f._call
    f._call = lambda *a, **k: (calls.append(a[0]), real(*a, **k))[1]
    for fn, extra in ((f.solve_sparse_batch, {}), (f.gram_batch, {}),
                      (lambda M, **k: f.solve_sparse_batch_dev(M, 0, n, **k), {}),
                      (lambda M, **k: f.gram_batch_dev(M, 0, 2, **k), {})):
        with pytest.raises(ValueError, match="scipy sparse"):
            fn(np.ones((n, 2)))
        with pytest.raises(ValueError, match="rows"):
            fn(sp.csc_matrix((n + 1, 2)))
        with pytest.raises(ValueError, match="shape"):
            fn(B, vals=np.ones((2, 4)))
        with pytest.raises(ValueError, match="shape"):
            fn(B, vals=np.ones(3))
    with pytest.raises(ValueError, match="job"):
        f.solve_sparse_batch(B, job=3)
    with pytest.raises(ValueError, match="wanted row"):
        f.solve_sparse_batch(B, rows=[0, n])
    with pytest.raises(ValueError, match="one-dimensional"):
        f.solve_sparse_batch(B, rows=[[0, 1]])
    with pytest.raises(ValueError, match="ldx"):
        f.solve_sparse_batch_dev(B, 0, 1, rows=[0, 1])
    with pytest.raises(ValueError, match="ldg"):
        f.gram_batch_dev(B, 0, 1)
    with pytest.raises(ValueError, match="out of range"):
        f.inverse_block_batch([0], [n])
    assert calls == [], calls                                  # nothing reached the library
    # on a handle without a batch the library refuses, with the name of the entry point (-30: no device to ask)
    for fn, name in ((lambda: f.solve_sparse_batch(B, vals=np.ones((2, 3))), "spllt_hip_solve_sparse_batch"),
                     (lambda: f.gram_batch(B), "spllt_hip_gram_sparse_batch"),
                     (lambda: f.inverse_block_batch([0, 1], [2]), "spllt_hip_solve_sparse_batch")):
        with pytest.raises(api.SplltError) as ei:
            fn()
        assert ei.value.flag in (-10, -30)
        if ei.value.flag == -10:
            assert "no batch" in str(ei.value) and name + ":" in str(ei.value)
    assert f.solve_sparse_batch_info() == dict(fwd_bcols=0, bwd_bcols=0, fwd_entries=0, bwd_entries=0, launches=0,
                                               workgroups=0, served=0, flagged=0)
    assert f.program("solve_sparse_batch_host_us") == 0
    f.release_solve_sparse_batch()
    f.close()


def test_partitioned_handle_is_unimplemented():
    g, _ = make_case(matgen.poisson2d(16), nb=16, nemin=8, prune=True, ncpu=2)
    g.set_partition(0, 2)
    B = sp.csc_matrix(([1.0], ([0], [0])), shape=(g.n, 1))
    for fn in (lambda: g.solve_sparse_batch(B), lambda: g.gram_batch(B)):
        with pytest.raises(api.SplltError) as ei:
            fn()
        assert ei.value.flag == -98
    g.close()


@functools.lru_cache(maxsize=None)
def _case(name):
    """A, a handle (analysis only), the tables, variable of a pivot position, per member (dense A_b, its arena, the
    Cholesky factor of P A_b P^T)"""
    gen, kw = CASES[name]
    A = sp.csc_matrix(gen())
    f, _ = make_case(A, **kw)
    t = sym_tables(f)
    var_of = np.empty(f.n, dtype=np.int64)
    var_of[t["order"]] = np.arange(f.n)
    members = []
    for b in range(NB):
        Ab, _vb = member_values(A, b, f.ptr, f.row)
        Ad = Ab.toarray()
        members.append((Ad, dense_arena(f, Ab), sl.cholesky(Ad[np.ix_(var_of, var_of)], lower=True)))
    return A, f, t, var_of, members


def _member_vals(B, nb):
    """member b's values on the pattern of B: B's own scaled by 1 + b / 4, the sign of every third flipped"""
    flip = np.where(np.arange(B.nnz) % 3 == 2, -1.0, 1.0)
    return np.stack([B.data * (1.0 + b / 4.0) * (flip if b % 2 else 1.0) for b in range(nb)])


def test_batch_program_tables_are_exported():
    A, f, t, var_of, members = _case("box5")
    units = f.program("bsolve_units")
    assert len(units) == len(t["bcol_off"]) and (units["pw"] == 64).all() and (units["cb"] == 64).all()
    # the launches of a substitution program do not depend on the panel width: one filter serves both programs
    for name in ("solve_list", "solve_fwd", "solve_bwd"):
        assert np.array_equal(f.program("b" + name), f.program(name)), name
    assert np.array_equal(f.program("bsolve_tiles"), f.program("solve_tiles"))
    with pytest.raises(KeyError):
        f.program("bsolve_nothing")


@pytest.mark.parametrize("job", [0, 1, 2])
@pytest.mark.parametrize("name", list(CASES))
def test_interpreter_reproduces_the_dense_solves(name, job):
    A, f, t, var_of, members = _case(name)
    n, nb = f.n, f.options.nb
    inp = _inputs(name, t, nb)
    order = t["order"]
    cols = [[inp["leaf"]], [inp["other_leaf"], inp["last"]], [], [inp["leaf"] + 1, inp["other_leaf"]]]
    if inp["mid"] is not None:
        cols.append([inp["mid"]])
    B = _columns(n, var_of, cols, seed=1)
    B.sort_indices()
    vals = _member_vals(B, NB)
    arenas = [m[1] for m in members]
    full = []
    for b, (Ad, _arena, Ld) in enumerate(members):
        Bb = sp.csc_matrix((vals[b], B.indices, B.indptr), shape=B.shape).toarray()
        Bp = np.zeros((n, len(cols)))
        Bp[order] = Bb
        full.append((Bp, {0: lambda: np.linalg.solve(Ad, Bb)[var_of],
                          1: lambda: sl.solve_triangular(Ld, Bp, lower=True),
                          2: lambda: sl.solve_triangular(Ld, Bp, lower=True, trans="T")}[job]()))
    for wanted in ([inp["leaf"]], [inp["other_leaf"], inp["last"], inp["other_leaf"]], [inp["last"] - 1, 3],
                   list(range(n))):
        rows = None if len(wanted) == n else var_of[wanted]
        fwd, bwd = f.solve_sparse_plan(B, rows=rows, job=job)
        got, y, touched = run_filtered_batch(f, t, arenas, B, vals, wanted, job, fwd, bwd)
        assert np.isfinite(got).all()
        assert np.isnan(y[:, :, ~touched]).all()         # nothing outside the touched rows was written
        for b, (Ad, _arena, Ld) in enumerate(members):
            Bp, fb = full[b]
            ref = fb[wanted]
            if job == 2:
                # entries of B outside the closure of the wanted rows are not scattered: they cannot reach them
                ref = sl.solve_triangular(Ld, Bp * touched[:, None], lower=True, trans="T")[wanted]
                np.testing.assert_allclose(ref, fb[wanted], rtol=0, atol=1e-13 * np.abs(fb).max())
            err = np.abs(got[b] - ref).max()
            print(name, job, "member", b, len(wanted), "err / max|x|", err / np.abs(fb).max())
            assert err <= 1e-12 * np.abs(fb).max()
            if job != 2:
                assert (got[b][:, 2] == 0.0).all()       # the empty column: exact zeros


@pytest.mark.parametrize("name", list(CASES))
def test_interpreter_gram(name):
    A, f, t, var_of, members = _case(name)
    n, nb = f.n, f.options.nb
    inp = _inputs(name, t, nb)
    cols = [[inp["leaf"]], [inp["other_leaf"], inp["last"]], [], [inp["leaf"] + 1, inp["other_leaf"]], [inp["last"]]]
    B = _columns(n, var_of, cols, seed=3)
    B.sort_indices()
    vals = _member_vals(B, NB)
    fwd, bwd = f.solve_sparse_plan(B, rows=[], job=1)
    assert len(bwd) == 0 and len(fwd) < len(t["bcol_off"])
    _, y, touched = run_filtered_batch(f, t, [m[1] for m in members], B, vals, [], 1, fwd, bwd)
    for b, (Ad, _arena, _Ld) in enumerate(members):
        Y = y[b][:, touched]
        G = Y @ Y.T
        Bb = sp.csc_matrix((vals[b], B.indices, B.indptr), shape=B.shape).toarray()
        ref = Bb.T @ np.linalg.solve(Ad, Bb)
        print(name, "member", b, "touched rows", int(touched.sum()), "err / max|G|", np.abs(G - ref).max() / np.abs(ref).max())
        assert np.abs(G - ref).max() <= 1e-11 * np.abs(ref).max()
        assert (G[2] == 0.0).all() and (G[:, 2] == 0.0).all()


def test_filter_under_the_host_sanitizers(tmp_path):
    clang = next((c for c in CLANG_CANDIDATES if os.path.exists(c)), None)
    if clang is None:
        pytest.skip("no ROCm clang++ on this machine")
    exe = str(tmp_path / "ss_filter_test")
    cmd = [clang, "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "spllt_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "ss_filter_test.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and ("asan" in built.stderr or "ubsan" in built.stderr) and "cannot find" in built.stderr:
        pytest.skip("the sanitizer runtime of the ROCm clang is not installed: " + built.stderr.strip().splitlines()[-1])
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    assert "ss_filter_test: ok" in ran.stdout
