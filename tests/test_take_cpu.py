"""CPU test of the feature-memory helpers of spllt_amd/csrc/engine_detail.hpp (Take, give_back, grow, Shared and
the two allocation hooks): tests/native/take_test.cpp drives them with a counting allocator on malloc / free that
fails at a chosen call, built host-only with the address and undefined-behaviour sanitizers and run as a
program of its own (no GPU, no preloaded library)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "take_test.cpp")
CLANG_CANDIDATES = ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++")


def _clang():
    for c in CLANG_CANDIDATES:
        if os.path.exists(c):
            return c
    return None


def test_take_give_back_grow_and_shared(tmp_path):
    clang = _clang()
    if clang is None:
        pytest.skip("no ROCm clang++ on this machine")
    exe = str(tmp_path / "take_test")
    cmd = [clang, "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           "-I" + os.path.join(ROOT, "spllt_amd", "csrc"), SRC, "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and ("asan" in built.stderr or "ubsan" in built.stderr) and "cannot find" in built.stderr:
        pytest.skip("the sanitizer runtime of the ROCm clang is not installed: " + built.stderr.strip().splitlines()[-1])
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    assert "take_test: ok" in ran.stdout
