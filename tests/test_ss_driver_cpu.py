"""CPU test of the call sequence of the sparse right-hand-side family (spllt_amd/csrc/ss_driver.hpp, the one
sequence behind solve_sparse / solve_sparse_batch and gram_sparse / gram_sparse_batch):
tests/native/ss_driver_test.cpp runs ss_solve_sequence and ss_gram_sequence on a scripted backend and compares the
recorded steps with traces written out by hand -- the cutting into groups, the order of the steps of a group, the
pair loop of gram with its output offsets, the counters, and the failure paths (a refused take, a failed upload,
copy-out or sync, a launch that overflows a grid).  Built host-only with the address and undefined-behaviour
sanitizers and run as a program of its own (no GPU, no preloaded library)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "ss_driver_test.cpp")
CLANG_CANDIDATES = ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++")


def _clang():
    for c in CLANG_CANDIDATES:
        if os.path.exists(c):
            return c
    return None


def test_ss_sequences(tmp_path):
    clang = _clang()
    if clang is None:
        pytest.skip("no ROCm clang++ on this machine")
    exe = str(tmp_path / "ss_driver_test")
    cmd = [clang, "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           "-I" + os.path.join(ROOT, "spllt_amd", "csrc"), SRC, "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and ("asan" in built.stderr or "ubsan" in built.stderr) and "cannot find" in built.stderr:
        pytest.skip("the sanitizer runtime of the ROCm clang is not installed: " + built.stderr.strip().splitlines()[-1])
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    assert "ss_driver_test: ok" in ran.stdout
