"""Helpers of the tests of the bit-reproducible batch (TEST-ONLY, never timed): the cases, the adapters that feed the
deterministic batch program to tests/emulate.py and the tables of the batch's reproducible sweep to
tests/solve_repro_emulate.py, and the two hazards the deterministic forms resolve."""
import numpy as np

from spllt_amd import matgen

L_GEMM, L_CHAIN, L_GATHER = 1, 4, 6
MODE_DIRECT, MODE_SCATTER, MODE_TRSM, MODE_BUFFER = 0, 1, 2, 3

# (name, generator, nb, nemin): the cases of the GPU tests.  Those of tests/test_batch_mult_gpu.py, except p2d12-nb8
# (n = 144): none of its block columns has two strips, so the backward sweep has nothing to order there; it is
# replaced by the next larger one of tests/test_solve_repro_cpu.py.
CASES = [
    ("p2d40-nb16", lambda: matgen.poisson2d(40), 16, 16),
    ("box11-nb64", lambda: matgen.nd_like((11, 10, 9), 2), 64, 16),
    ("p3d14-nb384", lambda: matgen.poisson3d(14), 384, 16),
]


class DetProgramView:
    """answers program(name) with the deterministic batch program ("batch_det_" + name) and passes everything else
    through: emulate.emulate_program(DetProgramView(f), val) interprets it"""

    def __init__(self, f):
        self._f = f

    def program(self, name):
        return self._f.program("batch_det_" + name)

    def __getattr__(self, name):
        return getattr(self._f, name)


class BatchSweepView:
    """for solve_repro_emulate.emulate_solve_repro: "rsolve_*" are the batch's tables ("batch_rsolve_*"); the
    substitution program is the handle's, which for a handle with the default panel width IS the batch's (pw = cb =
    64) -- the caller asserts that"""

    def __init__(self, f):
        self._f = f
        assert f.program("panel_width") == 64 and f.program("chain_block") == 64

    def program(self, name):
        return self._f.program("batch_" + name if name.startswith("rsolve_") else name)

    def __getattr__(self, name):
        return getattr(self._f, name)


def check_det_program(f):
    """the deterministic batch program holds only what batch_repro.hip implements; returns (launches, units, tiles)"""
    launches, units, tiles = (f.program("batch_det_" + k) for k in ("launches", "units", "tiles"))
    gtiles, gitems = f.program("batch_det_gather_tiles"), f.program("batch_det_gather_items")
    scratch = f.program("batch_det_scratch_size")
    assert set(launches[:, 0].tolist()) <= {L_CHAIN, L_GEMM, L_GATHER}, sorted(set(launches[:, 0].tolist()))
    assert (units["mode"] != MODE_SCATTER).all()
    for kind, _level, first, count, tile in launches[:, :5]:
        if count == 0:
            continue
        if kind == L_GEMM:
            assert tile in (32, 64), tile
            u = units[tiles[first:first + count]["unit"]]
            assert set(u["mode"].tolist()) <= {MODE_DIRECT, MODE_TRSM, MODE_BUFFER}
            assert (u["atomic"][u["mode"] == MODE_DIRECT] == 0).all()
            buf = u[u["mode"] == MODE_BUFFER]
            assert (buf["d_ld"] == buf["N"]).all() and (buf["d_off"] >= 0).all()
            assert (buf["d_off"] + buf["M"].astype(np.int64) * buf["N"] <= scratch).all()
        elif kind == L_GATHER:
            t = gtiles[first:first + count]
            assert ((t["rows"] >= 1) & (t["rows"] <= 64) & (t["cols"] >= 1) & (t["cols"] <= 64)).all()
            assert (t["first"] >= 0).all() and (t["first"] + t["count"] <= len(gitems)).all()
    if len(gitems):
        assert (gitems["buf_off"] + gitems["i1"].astype(np.int64) * gitems["ld"] <= scratch).all()
    return launches, units, tiles


def entry_hazard(f):
    """True when some destination ENTRY of some gather tile of the deterministic program receives from two distinct
    BUFFER units: two SCATTER units of one launch of the default batch program then add into one entry"""
    units, gtiles, gitems = (f.program("batch_det_" + k) for k in ("units", "gather_tiles", "gather_items"))
    relpos, rlist = f.program("batch_det_relpos"), f.sym("rlist")
    for t in gtiles:
        if t["count"] < 2:
            continue
        seen = {}
        for g in gitems[t["first"]:t["first"] + t["count"]]:
            key = (int(g["buf_off"]), int(g["relrow_off"]), int(g["gcol_off"]))
            rows = relpos[g["relrow_off"] + g["i0"]:g["relrow_off"] + g["i1"]]
            cols = rlist[g["gcol_off"] + g["j0"]:g["gcol_off"] + g["j1"]]
            for i, r in zip(range(g["i0"], g["i1"]), rows):
                for j, cc in zip(range(g["j0"], g["j1"]), cols):
                    if g["lower"] and g["diag_shift"] + i < j:
                        continue
                    if seen.setdefault((int(r), int(cc)), key) != key:
                        return True
    return False
