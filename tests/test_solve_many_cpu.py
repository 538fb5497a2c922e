"""CPU tests of the blocked many-right-hand-side solve: the interface exists in every layer, and the
argument errors that are decided before any device work come back as the parameter flag on a handle
that has only been analysed."""
import ctypes as C
import os
import re

import numpy as np

from helpers import make_case
from spllt_amd import _lib, api, matgen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_interface_exists_in_every_layer():
    lib = _lib.load()
    for name in ("spllt_hip_solve_many", "spllt_hip_solve_many_dev"):
        assert hasattr(lib, name), name
    header = open(os.path.join(ROOT, "include", "spllt_hip.h")).read()
    assert re.search(r"int\s+spllt_hip_solve_many\(void \*fkeep, int nrhs, double \*x_host, int64_t ldx, int job\);", header)
    assert re.search(r"int\s+spllt_hip_solve_many_dev\(void \*fkeep, int nrhs, double \*x_dev, int64_t ldx, int job,\s*"
                     r"int pivot_order\);", header)
    assert callable(api.Factorization.solve_many) and callable(api.Factorization.solve_many_dev)
    assert lib.spllt_hip_solve_many.argtypes[3] is C.c_int64 and lib.spllt_hip_solve_many_dev.argtypes[3] is C.c_int64


def test_argument_errors_on_an_analysed_handle():
    f, val = make_case(matgen.poisson2d(8), nb=8, nemin=4)
    n = f.n
    x = np.ones(3 * (n + 2))
    call, call_dev = f.lib.spllt_hip_solve_many, f.lib.spllt_hip_solve_many_dev
    cases = [(-1, api._dp(x), n, 0, "nrhs"), (3, api._dp(x), n - 1, 0, "ldx"), (3, api._dp(x), n, 3, "job"),
             (3, api._dp(x), n, -1, "job"), (3, None, n, 0, "null")]
    for nrhs, ptr, ldx, job, word in cases:
        assert call(f.fkeep, nrhs, ptr, ldx, job) == -10
        assert word in f.last_error(), f.last_error()
    # the device entry point takes the same checks (a host address is never touched before them)
    addr = x.ctypes.data
    for nrhs, ptr, ldx, job, word in [(-1, addr, n, 0, "nrhs"), (3, addr, n - 1, 0, "ldx"), (3, addr, n, 7, "job"),
                                      (3, None, n, 0, "null")]:
        assert call_dev(f.fkeep, nrhs, ptr, ldx, job, 0) == -10
        assert word in f.last_error(), f.last_error()
    # good arguments, nothing factorized yet: the flag spllt_hip_solve_dev gives in that state
    assert call(f.fkeep, 3, api._dp(x), n + 2, 0) == -10
    assert "factorized" in f.last_error()
    assert call(f.fkeep, 0, api._dp(x), n, 0) == -10
    assert (x == 1.0).all()
    assert call(None, 3, api._dp(x), n, 0) == -10
    f.close()
