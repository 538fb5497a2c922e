"""The XCD-aware tile order (SPLLT_XCD_ORDER) on the device, on the small case of
test_tile_order_cpu.py: the order of the tiles inside a launch decides where a workgroup runs, never
what it computes."""
import numpy as np
import pytest

from helpers import bwd_err, lower_mask, make_case, oracle_factor, rel_err
from spllt_amd import matgen

pytestmark = pytest.mark.gpu
TOL_L = 1e-12          # tests/test_gpu_parity.py
DETERMINISTIC = 4096   # engine flag: no atomics (buffered inter-node updates, ordered gather)


def _factor(A, monkeypatch, order, flags):
    """the factor of a fresh handle whose program is built under SPLLT_XCD_ORDER = order (None: default)"""
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    if order is None:
        monkeypatch.delenv("SPLLT_XCD_ORDER", raising=False)
    else:
        monkeypatch.setenv("SPLLT_XCD_ORDER", str(order))
    f, val = make_case(A, nb=64, nemin=4, engine_flags=flags)
    f.factor(val).wait()
    tiles = f.program("tiles").copy()     # the engine's own program
    return f, val, f.get_factor(), tiles


def test_deterministic_engine_is_bit_identical_under_both_orders(monkeypatch):
    A = matgen.poisson3d(12)
    f0, _, L0, t0 = _factor(A, monkeypatch, 0, DETERMINISTIC)
    f2, _, L2, t2 = _factor(A, monkeypatch, None, DETERMINISTIC)
    assert not np.array_equal(t0, t2)     # the two engines really ran different tile orders
    assert np.array_equal(L0, L2)
    f0.close()
    f2.close()


def test_default_engine_matches_oracle_under_new_order(monkeypatch):
    A = matgen.poisson3d(12)
    f, val, got, _ = _factor(A, monkeypatch, None, 0)
    o, rc = oracle_factor(f, val, variant="plain", nthreads=4)
    assert rc == 0
    mask = lower_mask(f)
    assert rel_err(got, o.arena(), mask) <= TOL_L
    assert np.all(got[~mask] == 0.0)
    b = A @ np.ones(f.n)
    assert bwd_err(A, f.solve(b), b) <= 1e-14
    f.close()
