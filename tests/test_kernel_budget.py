"""scripts/check_kernel_budget.py (the build's resource budget of k_chain_potrf) on small hand-written
metadata samples: one within the budget, one over it in each of the three ways."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "scripts", "check_kernel_budget.py")
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import check_kernel_budget as ckb  # noqa: E402

SAMPLE = """\
\t.text
_ZN3spx13k_chain_potrfEv:
\ts_endpgm
\t.amdgpu_metadata
---
amdhsa.kernels:
  - .agpr_count:     0
    .args:
      - .address_space:  global
        .offset:         0
        .size:           8
        .value_kind:     global_buffer
    .group_segment_fixed_size: 76800
    .kernarg_segment_size: 72
    .name:           _ZN3spx13k_potrf_panelEv
    .private_segment_fixed_size: 0
    .sgpr_count:     81
    .symbol:         _ZN3spx13k_potrf_panelEv.kd
    .vgpr_count:     180
    .wavefront_size: 64
  - .agpr_count:     %(agpr)d
    .args:
      - .offset:         32
        .size:           40
        .value_kind:     by_value
    .group_segment_fixed_size: %(lds)d
    .kernarg_segment_size: 72
    .name:           _ZN3spx13k_chain_potrfEv
    .private_segment_fixed_size: %(scratch)d
    .sgpr_count:     58
    .symbol:         _ZN3spx13k_chain_potrfEv.kd
    .vgpr_count:     %(vgpr)d
    .wavefront_size: 64
amdhsa.target:   amdgcn-amd-amdhsa--gfx950
amdhsa.version:
  - 1
  - 2
...
\t.end_amdgpu_metadata
"""


def _check(**kw):
    v = dict(vgpr=128, agpr=0, scratch=0, lds=0)
    v.update(kw)
    return ckb.check(SAMPLE % v, "k_chain_potrf", 128, 0, 80 * 1024)


def test_within_budget_passes():
    status, msg = _check()
    assert status == 0 and "128 registers" in msg and "OVER" not in msg
    assert _check(vgpr=120, agpr=16, lds=80 * 1024)[0] == 0


@pytest.mark.parametrize("kw,what", [(dict(vgpr=136), "registers"), (dict(vgpr=180, agpr=16), "registers"),
                                      (dict(scratch=116), "scratch"), (dict(lds=80 * 1024 + 8), "LDS")])
def test_over_budget_fails(kw, what):
    status, msg = _check(**kw)
    assert status == 1 and msg.splitlines()[-1] == "OVER BUDGET: " + what


def test_only_the_named_kernel_is_judged_and_a_missing_one_is_an_error():
    assert ckb.check(SAMPLE % dict(vgpr=128, agpr=0, scratch=0, lds=0), "k_potrf_panel", 128, 0, 80 * 1024)[0] == 1
    assert ckb.check(SAMPLE % dict(vgpr=128, agpr=0, scratch=0, lds=0), "k_nowhere", 128, 0, 80 * 1024)[0] == 2
    assert ckb.check("no metadata here\n", "k_chain_potrf", 128, 0, 80 * 1024)[0] == 2


def test_command_line_exit_status(tmp_path):
    good, bad = tmp_path / "good.s", tmp_path / "bad.s"
    good.write_text(SAMPLE % dict(vgpr=128, agpr=0, scratch=0, lds=0))
    bad.write_text(SAMPLE % dict(vgpr=180, agpr=16, scratch=0, lds=76800))
    assert subprocess.run([sys.executable, SCRIPT, str(good)], capture_output=True).returncode == 0
    r = subprocess.run([sys.executable, SCRIPT, str(bad)], capture_output=True, text=True)
    assert r.returncode == 1 and "OVER BUDGET: registers" in r.stdout
