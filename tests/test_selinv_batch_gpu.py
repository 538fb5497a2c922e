"""GPU tests of the batched selected inversion (spllt_hip_selected_inverse_batch and friends,
batch_selinv.hip): Z_b = (P A_b P^T)^-1 on the pattern of L for every member of a batch, by one program
whose every launch carries all members.  Members: A_b = D_b A D_b (batch_emulate.member_matrix).  Bars,
those of tests/test_selinv_gpu.py: 1e-11 against the dense inverse (relative to max|Z|), 1e-13 against
the numpy interpretation of the same program on the member's own GPU factor, 1e-11 for the two readers.
No test provokes a device fault: a member that is not positive definite is an arithmetic outcome the
kernels report through a flag."""
import ctypes as C
import functools
import time

import numpy as np
import pytest

from batch_emulate import member_values
from helpers import lower_mask, make_case
from selinv_emulate import emulate_selinv, expected_z, panel_inverses
from spllt_amd import _lib, api, matgen

pytestmark = pytest.mark.gpu

# the five patterns of tests/test_factor_batch_gpu.py
CASES = [
    ("p2d40-nb16", lambda: matgen.poisson2d(40), 16, 0),
    ("box11-nb64", lambda: matgen.nd_like((11, 10, 9), 2), 64, 0),
    ("p3d14-nb384", lambda: matgen.poisson3d(14), 384, 0),
    ("fe27-nb768", lambda: matgen.fe27((7, 6, 6), 3), 768, 256),
    ("box12-nb512", lambda: matgen.nd_like((10, 12, 12), 3), 512, 256),
]
NAMES = [c[0] for c in CASES]
NBATCH = [1, 3, 16]
TOL_DENSE, TOL_EMU = 1e-11, 1e-13
TABLES = ("units", "tiles", "launches", "rows", "relpos", "diag", "scratch")


def _rel(a, b, mask):
    return float(np.abs(a[mask] - b[mask]).max() / np.abs(b[mask]).max())


class Case:
    def __init__(self, name, **kw):
        _, gen, nb, min_width = next(c for c in CASES if c[0] == name)
        self.name = name
        self.A = gen()
        self.f, self.val = make_case(self.A, nb=nb, nemin=16, **kw)
        assert int(self.f.sym("bcol_width").max()) > min_width, "the case degenerated: no wide block column"
        self.mask = lower_mask(self.f)
        self.tables = {k: self.f.program("batch_selinv_" + k) for k in TABLES}
        self._members, self._ref, self._inv = {}, {}, {}

    def member(self, b):
        """(A_b, val_b)"""
        if b not in self._members:
            self._members[b] = member_values(self.A, b, self.f.ptr, self.f.row)
        return self._members[b]

    def values(self, nbatch):
        return np.stack([self.member(b)[1] for b in range(nbatch)])

    def expected(self, b):
        """inv(P A_b P^T) on the arena"""
        if b not in self._ref:
            self._ref[b] = expected_z(self.f, self.member(b)[0])
        return self._ref[b]

    def dense_inverse(self, b):
        if b not in self._inv:
            self._inv[b] = np.linalg.inv(self.member(b)[0].toarray())
        return self._inv[b]

    def pattern(self):
        """0-based (row, column) of the entries of the analysed CSC-lower pattern, in the order of val"""
        ptr, row = np.asarray(self.f.ptr) - 1, np.asarray(self.f.row) - 1
        return row, np.repeat(np.arange(self.f.n), np.diff(ptr))

    def emulated(self, b):
        """the batch's selinv program interpreted in numpy on member b's own GPU factor"""
        L = self.f.get_factor_batch(b)
        return emulate_selinv(self.f, L, panel_inverses(self.f, L, self.tables), self.tables)


@functools.lru_cache(maxsize=None)
def _case(name):
    return Case(name)


def _assert_member(c, b, Z, diag, onpat, what="", emulate=True):
    e_dense = _rel(Z, c.expected(b), c.mask)
    e_emu = _rel(Z, c.emulated(b), c.mask) if emulate else 0.0
    Ainv = c.dense_inverse(b)
    e_diag = float(np.abs(diag - np.diag(Ainv)).max() / np.abs(np.diag(Ainv)).max())
    r, cc = c.pattern()
    e_pat = float(np.abs(onpat - Ainv[r, cc]).max() / np.abs(Ainv).max())
    print(c.name, what, "member", b, "Z vs dense %.2e, vs emulation %.2e, diag %.2e, on pattern %.2e"
          % (e_dense, e_emu, e_diag, e_pat))
    assert np.isfinite(Z[c.mask]).all()
    assert e_dense <= TOL_DENSE, (b, e_dense)
    assert e_emu <= TOL_EMU, (b, e_emu)
    assert e_diag <= TOL_DENSE, (b, e_diag)
    assert e_pat <= TOL_DENSE, (b, e_pat)


def _fused(f, on):
    assert f.lib.spllt_hip_debug(b"batch_selinv_fused=1" if on else b"batch_selinv_fused=0") == 0


@pytest.fixture(autouse=True)
def _default_hooks():
    yield
    lib = _lib.load()
    lib.spllt_hip_debug(b"batch_selinv_fused=1")
    lib.spllt_hip_debug(b"batch_grid_limit=0")


# ---- parity per member ------------------------------------------------------------------------------
@pytest.mark.parametrize("nbatch", NBATCH)
@pytest.mark.parametrize("name", NAMES)
def test_every_member_matches_the_dense_inverse_and_the_emulation(name, nbatch):
    c = _case(name)
    f = c.f
    assert f.factor_batch(c.values(nbatch)) == 0, f.last_error()
    assert f.selected_inverse_batch() == 0, f.last_error()
    diag, onpat = f.inverse_diag_batch(), f.inverse_on_pattern_batch()
    assert diag.shape == (nbatch, f.n) and onpat.shape == (nbatch, f.nnz)
    for b in range(nbatch):
        _assert_member(c, b, f.get_inverse_batch(b), diag[b], onpat[b], "nbatch %d" % nbatch)
    ptr, stride = f.device_inverse_batch_ptr()
    assert ptr and stride >= f.sym_info()["arena"] and stride % 32 == 0
    assert stride == f.device_factor_batch_ptr()[1]


@pytest.mark.parametrize("name", NAMES)
def test_the_unfused_form_meets_the_bars_too(name):
    c = _case(name)
    f = c.f
    assert f.factor_batch(c.values(3)) == 0
    _fused(f, False)
    assert f.selected_inverse_batch() == 0
    diag, onpat = f.inverse_diag_batch(), f.inverse_on_pattern_batch()
    for b in range(3):
        _assert_member(c, b, f.get_inverse_batch(b), diag[b], onpat[b], "unfused")


def test_the_leading_dimensions_of_the_readers():
    """ldout > n / nnz: the padding and two extra rows behind the last member stay bit-identical"""
    c = _case("box11-nb64")
    f, n, nnz = c.f, c.f.n, c.f.nnz
    assert f.factor_batch(c.values(3)) == 0 and f.selected_inverse_batch() == 0
    d0, p0 = f.inverse_diag_batch(), f.inverse_on_pattern_batch()
    for fn, w, want in ((f.lib.spllt_hip_inverse_diag_batch, n, d0), (f.lib.spllt_hip_inverse_on_pattern_batch, nnz, p0)):
        out = np.full((5, w + 7), -7.25e77)
        assert fn(f.fkeep, api._dp(out), w + 7) == 0, f.last_error()
        assert np.array_equal(out[:3, :w], want)
        assert (out[:3, w:] == -7.25e77).all() and (out[3:] == -7.25e77).all()


# ---- reproducibility, fused against unfused ------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_two_inversions_are_bit_identical_and_the_two_forms_agree(name):
    c = _case(name)
    f, nbatch = c.f, 3
    assert f.factor_batch(c.values(nbatch)) == 0
    Z = {}
    for on in (True, False):
        _fused(f, on)
        assert f.selected_inverse_batch() == 0
        first = [f.get_inverse_batch(b).copy() for b in range(nbatch)]
        assert f.selected_inverse_batch() == 0
        for b in range(nbatch):
            assert np.array_equal(first[b][c.mask], f.get_inverse_batch(b)[c.mask]), (on, b)
        Z[on] = first
    for b in range(nbatch):
        e = _rel(Z[True][b], Z[False][b], c.mask)
        print(name, "member", b, "fused vs unfused %.2e" % e)
        assert e <= 1e-13, (b, e)


def test_fusing_saves_launches_and_the_count_does_not_depend_on_the_batch_size():
    c = _case("p2d40-nb16")
    f = c.f
    launches = c.tables["launches"]
    counts = {}
    for nbatch in (1, 16):
        assert f.factor_batch(c.values(nbatch)) == 0
        for on in (True, False):
            _fused(f, on)
            assert f.selected_inverse_batch() == 0
            counts[(nbatch, on)] = f.batch_selinv_launches()
    print("p2d40-nb16 launches: fused", counts[(16, True)], "unfused", counts[(16, False)])
    assert counts[(1, True)] == counts[(16, True)] and counts[(1, False)] == counts[(16, False)]
    assert counts[(16, False)] == int((launches[:, 3] > 0).sum())
    assert counts[(16, True)] < counts[(16, False)]
    assert counts[(16, True)] >= int((launches[:, 0] == 2).sum())         # at least one launch per step


# ---- one bad member -----------------------------------------------------------------------------------
@pytest.mark.parametrize("on", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("name", ["p2d40-nb16", "box11-nb64"])
def test_one_bad_member_is_skipped_and_the_others_are_inverted(name, on):
    c = _case(name)
    f, n, nbatch, k = c.f, c.f.n, 5, 2
    j = n // 2
    vals = c.values(nbatch).copy()
    vals[k, f.ptr[j] - 1] *= -1.0              # the diagonal entry of variable j
    assert f.factor_batch(vals) == -20
    _fused(f, on)
    rc = f.lib.spllt_hip_selected_inverse_batch(f.fkeep)
    assert rc == -20 and "skipped" in f.last_error()
    assert f.selected_inverse_batch() == -20               # (Python: no exception)
    diag, onpat = f.inverse_diag_batch(), f.inverse_on_pattern_batch()
    assert np.isnan(diag[k]).all() and np.isnan(onpat[k]).all()
    with pytest.raises(api.SplltError) as ei:
        f.get_inverse_batch(k)
    assert ei.value.flag == -20 and "member %d" % k in f.last_error()
    for b in range(nbatch):
        if b != k:
            _assert_member(c, b, f.get_inverse_batch(b), diag[b], onpat[b], "bad member %d" % k)
    # the handle is still good
    assert f.factor_batch(c.values(nbatch)) == 0 and f.selected_inverse_batch() == 0
    assert np.isfinite(f.inverse_diag_batch()).all()


# ---- launches split by member range ---------------------------------------------------------------------
@pytest.mark.parametrize("on", [True, False], ids=["fused", "unfused"])
def test_a_launch_too_large_for_one_grid_is_split_by_member_range(on):
    c = _case("box11-nb64")
    f, nbatch = c.f, 16
    assert f.factor_batch(c.values(nbatch)) == 0
    _fused(f, on)
    assert f.selected_inverse_batch() == 0
    whole = f.batch_selinv_launches()
    Z0 = [f.get_inverse_batch(b).copy() for b in range(nbatch)]
    d0, p0 = f.inverse_diag_batch(), f.inverse_on_pattern_batch()
    biggest = int(c.tables["launches"][:, 3].max())
    try:
        assert f.lib.spllt_hip_debug(("batch_grid_limit=%d" % (5 * biggest)).encode()) == 0   # at most 5 members per launch
        assert f.selected_inverse_batch() == 0
        split = f.batch_selinv_launches()
        Zs = [f.get_inverse_batch(b).copy() for b in range(nbatch)]
        ds, ps = f.inverse_diag_batch(), f.inverse_on_pattern_batch()
    finally:
        assert f.lib.spllt_hip_debug(b"batch_grid_limit=0") == 0
    print("launches", whole, "->", split)
    assert split > whole
    for a, b in zip(Zs, Z0):
        assert np.array_equal(a[c.mask], b[c.mask])
    assert np.array_equal(ds, d0) and np.array_equal(ps, p0)
    assert f.selected_inverse_batch() == 0 and f.batch_selinv_launches() == whole


@pytest.mark.parametrize("fast", ["0", "1"])
def test_both_grid_mappings(fast, monkeypatch):
    monkeypatch.setenv("SPLLT_BATCH_MEMBER_FAST", fast)
    c = Case("box11-nb64")                      # (the mapping is read when a handle prepares its first batch)
    f = c.f
    for on in (True, False):
        assert f.factor_batch(c.values(3)) == 0
        _fused(f, on)
        assert f.selected_inverse_batch() == 0
        diag, onpat = f.inverse_diag_batch(), f.inverse_on_pattern_batch()
        for b in range(3):
            _assert_member(c, b, f.get_inverse_batch(b), diag[b], onpat[b], "member_fast " + fast)
    f.close()


# ---- staleness, independence, storage -------------------------------------------------------------------
def test_a_new_batch_makes_the_inverse_stale():
    c = _case("p2d40-nb16")
    f = c.f
    assert f.factor_batch(c.values(3)) == 0 and f.selected_inverse_batch() == 0
    f.get_inverse_batch(0)
    assert f.factor_batch(c.values(3)) == 0
    for read in (lambda: f.get_inverse_batch(0), f.inverse_diag_batch, f.inverse_on_pattern_batch):
        with pytest.raises(api.SplltError) as ei:
            read()
        assert ei.value.flag == -10 and "selected_inverse_batch" in f.last_error()
    assert f.device_inverse_batch_ptr() == (None, 0)
    assert f.selected_inverse_batch() == 0
    assert _rel(f.get_inverse_batch(1), c.expected(1), c.mask) <= TOL_DENSE
    # an empty batch is a no-op that leaves the inverse valid
    v = c.values(1)
    assert f.lib.spllt_hip_factor_batch(f.akeep, f.fkeep, 0, f.nnz, C.c_void_p(v.ctypes.data), f.nnz) == 0
    assert _rel(f.get_inverse_batch(1), c.expected(1), c.mask) <= TOL_DENSE


def test_the_single_inverse_and_the_batch_inverse_do_not_disturb_each_other():
    c = _case("box11-nb64")
    f = c.f
    A7, v7 = c.member(7)
    f.factor(v7).wait()
    f.selected_inverse()
    Z0, d0 = f.get_inverse().copy(), f.inverse_diag().copy()
    assert f.factor_batch(c.values(3)) == 0 and f.selected_inverse_batch() == 0
    assert np.array_equal(f.get_inverse(), Z0) and np.array_equal(f.inverse_diag(), d0)   # still valid, untouched
    before = [f.get_inverse_batch(b).copy() for b in range(3)]
    f.factor(c.member(9)[1]).wait()             # the single factor again: its Z is stale, the batch's is not
    with pytest.raises(api.SplltError):
        f.get_inverse()
    f.selected_inverse()
    for b in range(3):
        assert np.array_equal(f.get_inverse_batch(b), before[b])
    assert _rel(f.get_inverse(), c.expected(9), c.mask) <= TOL_DENSE
    assert _rel(before[2], c.expected(2), c.mask) <= TOL_DENSE


def test_storage_grows_and_is_released():
    c = _case("p2d40-nb16")
    f = c.f
    rng = np.random.default_rng(11)
    for nbatch in (4, 2, 24):
        assert f.factor_batch(c.values(nbatch)) == 0 and f.selected_inverse_batch() == 0
        assert f.inverse_diag_batch().shape == (nbatch, f.n)
        for b in (0, nbatch - 1):
            assert _rel(f.get_inverse_batch(b), c.expected(b), c.mask) <= TOL_DENSE
        with pytest.raises(api.SplltError) as ei:
            f.get_inverse_batch(nbatch)
        assert ei.value.flag == -10 and "member" in f.last_error()
    f.release_inverse_batch()
    assert f.device_inverse_batch_ptr() == (None, 0) and f.batch_selinv_launches() == 0
    with pytest.raises(api.SplltError) as ei:
        f.inverse_diag_batch()
    assert ei.value.flag == -10 and "selected_inverse_batch" in f.last_error()
    f.release_inverse_batch()                               # twice is fine
    # the batch factor and its solve are still there
    x = rng.standard_normal((24, f.n))
    B = np.stack([c.member(b)[0] @ x[b] for b in range(24)])
    np.testing.assert_allclose(f.solve_batch(B), x, rtol=0, atol=1e-9)
    assert f.selected_inverse_batch() == 0
    assert _rel(f.get_inverse_batch(23), c.expected(23), c.mask) <= TOL_DENSE
    f.release_batch()                                       # ... which takes the inverse with it
    assert f.device_inverse_batch_ptr() == (None, 0)
    with pytest.raises(api.SplltError) as ei:
        f.selected_inverse_batch()
    assert ei.value.flag == -10 and "no batch" in f.last_error()
    assert f.factor_batch(c.values(2)) == 0 and f.selected_inverse_batch() == 0
    assert _rel(f.get_inverse_batch(1), c.expected(1), c.mask) <= TOL_DENSE


def test_partitioned_handle_returns_unimplemented():
    import torch
    A = matgen.poisson2d(32)
    f, val = make_case(A, nb=16, nemin=8, prune=True, ncpu=2)
    xb = torch.zeros(max(1, f.set_partition(0, 2)), dtype=torch.float64, device="cuda")
    f.set_exchange_buffer(xb.data_ptr())
    for call in (f.selected_inverse_batch, f.inverse_diag_batch, f.inverse_on_pattern_batch,
                 lambda: f.get_inverse_batch(0)):
        with pytest.raises(api.SplltError) as ei:
            call()
        assert ei.value.flag == -98 and "partitioned" in f.last_error()
    f.close()


# ---- the single-handle twin of the pattern reader ---------------------------------------------------------
@pytest.mark.parametrize("name", ["p2d40-nb16", "fe27-nb768"])
def test_inverse_on_pattern_matches_inverse_entries(name):
    c = _case(name)
    f = c.f
    A3, v3 = c.member(3)
    f.factor(v3).wait()
    f.selected_inverse()
    r, cc = c.pattern()
    got = f.inverse_on_pattern()
    assert got.shape == (f.nnz,)
    assert np.array_equal(got, f.inverse_entries(r, cc))
    Ainv = c.dense_inverse(3)
    assert np.abs(got - Ainv[r, cc]).max() <= TOL_DENSE * np.abs(Ainv).max()
    f.factor(v3).wait()                          # stale again
    with pytest.raises(api.SplltError) as ei:
        f.inverse_on_pattern()
    assert ei.value.flag == -10 and "selected_inverse" in f.last_error()


# ---- timing guard -------------------------------------------------------------------------------------
def test_a_batched_inversion_is_not_slower_than_its_members_one_after_the_other():
    """p2d40-nb16, 16 members: one batched inversion against 16 single-handle selected_inverse calls on
    the same pattern in the same process (the unchanged single-handle path).  Median of 5 after 2
    warm-ups each, alternating, a host clock around calls that end in a synchronise."""
    import torch
    c = _case("p2d40-nb16")
    f, nbatch = c.f, 16
    f.factor(c.member(0)[1]).wait()
    assert f.factor_batch(c.values(nbatch)) == 0
    t_seq, t_batch = [], []
    for it in range(7):
        for which in ("seq", "batch"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if which == "seq":
                for b in range(nbatch):
                    f.selected_inverse()
            else:
                assert f.selected_inverse_batch() == 0
            dt = time.perf_counter() - t0
            if it >= 2:
                (t_seq if which == "seq" else t_batch).append(dt)
    # both hold member 0's inverse, each within 1e-11 of the dense one
    assert _rel(f.get_inverse_batch(0), f.get_inverse(), c.mask) <= 2 * TOL_DENSE
    seq, bat = float(np.median(t_seq)), float(np.median(t_batch))
    print("16 sequential inversions %.3f ms, one batched inversion of 16 %.3f ms, ratio %.2f, launches %d"
          % (seq * 1e3, bat * 1e3, seq / bat, f.batch_selinv_launches()))
    assert bat <= seq, (seq, bat)
