"""PyTorch front end: differentiable sparse SPD solve, log-determinant, factor products and sampling on the GPU.

``SparseCholesky`` owns one analysed pattern (an ``api.Factorization``) and offers ``solve``, ``logdet``, their
batched twins, ``factor_apply`` (L, L^T, L^-1, L^-T times a block of vectors) and ``rsample`` (reparameterised
Gaussian draws) as ``torch.autograd.Function``s over device tensors.  Nothing is computed here: the factorization,
the solves, the selected inverse, the sampled outer product and the adjoint of the factor of the backward passes
are the library's HIP kernels, called on the tensors' own memory (DESIGN.md sections 17 and 19).

Convention: ``val[k]`` is the k-th stored value of the CSC lower triangle and stands for BOTH a_ij and a_ji, so

    d loss / d val[k] = -(lam_i x_j + [i != j] lam_j x_i)      for x = A^-1 b,  lam = A^-1 xbar
    d logdet / d val[k] = (2 - delta_ij) (A^-1)_ij

The factor itself is differentiated by one sweep (spllt_hip_factor_adjoint): with all vectors in pivot order

    y = L x: Lbar = ybar x^T        y = L^-1 x: Lbar = -(L^-T ybar) y^T
    y = L^T x: Lbar = x ybar^T      y = L^-T x: Lbar = -y (L^-1 ybar)^T

restricted to the pattern of L, any number of columns in ONE sweep (the map Lbar -> d loss / d val is linear).

The factors of a batch are differentiated the same way, all members in one sweep (spllt_hip_factor_adjoint_batch):
``factor_apply_batch`` and ``rsample_batch``.

Out of scope: CPU tensors, float32, partitioned handles, sparse right-hand sides, second derivatives; ``sample`` and
``sample_batch`` stay without a gradient to the matrix values (``rsample`` and ``rsample_batch`` have it).
"""
import weakref

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from .api import Factorization, SplltError, csc_lower_1based

__all__ = ["SparseCholesky"]

_NOT_POSDEF = -20
# what a batch operation says under reproducible=True alone (the single handle's switch does not reach the batch)
_NO_DET_BATCH = (": the batch has no deterministic form under reproducible=True; pass batch_reproducible=True for the "
                 "bit-reproducible batch")


class SparseCholesky:
    """A sparse SPD matrix pattern with differentiable operations on its values.

    A_or_pattern: a scipy sparse symmetric matrix (its lower triangle gives the pattern and the order of ``val``) or
    the triple (n, ptr, row) of a 1-based CSC lower triangle.  reproducible=True: the deterministic engine (flag
    4096) and the reproducible solve -- forward and backward of ``solve`` and ``logdet`` are then bit-reproducible
    across calls; it does not reach the batch, whose operations then raise NotImplementedError unless
    batch_reproducible=True is given too.  batch_reproducible=True: Factorization.set_batch_reproducible for the
    handle -- the deterministic batch factorization and the reproducible blocked sweep under every batch operation:
    ``solve_batch``, ``logdet_batch``, ``sample_batch`` (both kinds), ``solve_constrained_batch``,
    ``factor_apply_batch`` and ``rsample_batch`` and the backward passes of the differentiable ones repeat bit for
    bit, whatever the batch size and a member's place in it.  batch_blocked=True: the
    forward and the backward of ``solve_batch`` and the precision kind of ``sample_batch`` run through the blocked
    matrix-core batch solve (Factorization.solve_many_batch_dev) instead of solve_batch_dev -- the same numbers to
    rounding, the path for many right-hand sides per member; off by default.

    One factorization serves every operation on the same values: the object remembers the tensor it factorized last
    (a weak reference and its ``_version``) and the library's factor serial, and factorizes again only when one of
    them differs.  A write that bypasses the version counter (``val.data``, a raw pointer) is not seen, exactly as
    autograd's own check of saved tensors does not see it: pass a fresh tensor or call ``invalidate()`` then.
    """

    def __init__(self, A_or_pattern, nb=256, reproducible=False, batch_blocked=False, batch_reproducible=False,
                 **analyse_kw):
        if isinstance(A_or_pattern, (tuple, list)):
            n, ptr, row = A_or_pattern
        else:
            n, ptr, row, _ = csc_lower_1based(A_or_pattern)
        self.reproducible = bool(reproducible)
        self.batch_blocked = bool(batch_blocked)
        flags = int(analyse_kw.pop("engine_flags", 0)) | (4096 if self.reproducible else 0)
        self.f = Factorization(n, ptr, row, nb=nb, engine_flags=flags, **analyse_kw)
        self.n, self.nnz = self.f.n, self.f.nnz
        self.batch_reproducible = bool(batch_reproducible)
        if self.batch_reproducible:   # (off: the handle never hears of the switch)
            self.f.set_batch_reproducible(True)
        self.device = None           # the device of the first tensor; the engine is created there
        self._stream = None
        self._weight = None           # 2 - delta_ij per entry of val
        self._C = None                # set_constraints: (the rows, whether the handle has them)
        self._C_on_batch = False      # ... and whether the handle's batch has them
        self.invalidate()

    # ---- checks: before any library call ----------------------------------------------------------
    def _tensor(self, t, name, shape, device=None):
        """device: where the tensor has to be when the handle has no device yet (that of the call's first tensor)"""
        device = self.device if self.device is not None else device
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name}: expected a torch.Tensor, got {type(t).__name__}")
        if t.dtype != torch.float64:
            raise TypeError(f"{name}: expected float64, got {t.dtype}")
        if t.device.type != "cuda":
            raise ValueError(f"{name}: expected a tensor on the GPU, got one on {t.device}")
        if device is not None and t.device != device:
            raise ValueError(f"{name}: expected a tensor on {device} like the handle's other tensors, got one on {t.device}")
        if len(shape) != t.dim() or any(s is not None and s != d for s, d in zip(shape, t.shape)):
            want = "(" + ", ".join("*" if s is None else str(s) for s in shape) + ")"
            raise ValueError(f"{name}: expected shape {want}, got {tuple(t.shape)}")
        return t

    def _values(self, t, name, shape):
        """the values are read in place by the factorization: they have to be contiguous"""
        self._tensor(t, name, shape)
        if not t.is_contiguous():
            raise ValueError(f"{name}: expected a contiguous tensor (the factorization reads it in place)")
        return t

    def _rhs(self, B, name, device=None):
        if isinstance(B, torch.Tensor) and B.dim() == 1:
            return self._tensor(B, name, (self.n,), device)
        return self._tensor(B, name, (self.n, None), device)

    def _enter(self, t):
        """the handle's device fixed by the first tensor; no library call under stream capture"""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("SparseCholesky: the library synchronizes with the host, it cannot run under stream capture")
        if self.device is None:
            self.device = t.device

    def _sync(self):
        """the engine stream waits for the work torch has enqueued on its current stream"""
        with torch.cuda.device(self.device):
            if self._stream is None:
                self._stream = torch.cuda.ExternalStream(self.f.engine_stream(), device=self.device)
            self._stream.wait_stream(torch.cuda.current_stream(self.device))

    # ---- the factor cache ---------------------------------------------------------------------------
    def invalidate(self):
        """forget which tensors the current factors came from: the next operation factorizes again"""
        self._fac = (None, -1, -1)    # (weak reference, _version, factor serial) of the single factor
        self._bat = (None, -1, -1)    # ... of the batch
        self._z_serial = (-1, -1)     # factor serials whose selected inverse is on the device

    @staticmethod
    def _current(slot, t, serial):
        ref, version, ser = slot
        return ref is not None and ref() is t and version == t._version and ser == serial

    def _ensure_factor(self, val):
        """the factor of val on the device; returns its serial"""
        serial = self.f.factor_serial(0)
        if self._current(self._fac, val, serial):
            return serial
        self._fac = (None, -1, -1)
        self._sync()
        with torch.cuda.device(self.device):
            self.f.factor_dev(val.data_ptr())
            self.f.wait()             # raises SplltError on a matrix that is not positive definite
        serial = self.f.factor_serial(0)
        self._fac = (weakref.ref(val), val._version, serial)
        return serial

    def _ensure_batch(self, vals):
        serial = self.f.factor_serial(1)
        if self._current(self._bat, vals, serial):
            return serial
        self._bat = (None, -1, -1)
        self._sync()
        with torch.cuda.device(self.device):
            rc = self.f.factor_batch_dev(vals.data_ptr(), vals.shape[0], ldval=self.nnz)
        if rc == _NOT_POSDEF:
            flags, cols = self.f.batch_status()
            bad = [int(b) for b in np.nonzero(flags)[0]]
            raise SplltError("spllt_hip_factor_batch_dev", rc,
                             f"members {bad} are not positive definite (pivot columns {[int(cols[b]) for b in bad]})")
        serial = self.f.factor_serial(1)
        self._bat = (weakref.ref(vals), vals._version, serial)
        return serial

    def _weights(self):
        if self._weight is None:
            row, col = self.f.pattern_tables()
            self._weight = torch.as_tensor(np.where(row == col, 1.0, 2.0), dtype=torch.float64, device=self.device)
        return self._weight

    # ---- library calls on tensors ---------------------------------------------------------------------
    def _solve_inplace(self, work):
        """work: (nrhs, n) contiguous, overwritten with the solutions"""
        self._sync()
        with torch.cuda.device(self.device):
            if self.reproducible:
                self.f.solve_reproducible_dev(work.data_ptr(), work.shape[0], ldx=self.n)
            else:
                self.f.solve_many_dev(work.data_ptr(), work.shape[0], ldx=self.n)
        return work

    def _solve_batch_inplace(self, work):
        """work: (nbatch, nrhs, n) contiguous, overwritten"""
        self._sync()
        with torch.cuda.device(self.device):
            if self.batch_blocked:
                self.f.solve_many_batch_dev(work.data_ptr(), work.shape[1], ldx=self.n)
            else:
                self.f.solve_batch_dev(work.data_ptr(), work.shape[1], ldx=self.n)
        return work

    def _outer(self, ut, vt, alpha):
        """ut, vt: (nvec, n) contiguous -> (nnz,)"""
        out = torch.empty(self.nnz, dtype=torch.float64, device=self.device)
        self._sync()
        with torch.cuda.device(self.device):
            self.f.pattern_outer_dev(ut.data_ptr(), vt.data_ptr(), ut.shape[0], out.data_ptr(), alpha=alpha)
        return out

    def _outer_batch(self, ut, vt, alpha):
        """ut, vt: (nbatch, nvec, n) contiguous -> (nbatch, nnz)"""
        out = torch.empty((ut.shape[0], self.nnz), dtype=torch.float64, device=self.device)
        self._sync()
        with torch.cuda.device(self.device):
            self.f.pattern_outer_batch_dev(ut.data_ptr(), vt.data_ptr(), ut.shape[0], ut.shape[1], out.data_ptr(),
                                           alpha=alpha)
        return out

    def _inverse_on_pattern(self, serial):
        out = torch.empty(self.nnz, dtype=torch.float64, device=self.device)
        self._sync()
        with torch.cuda.device(self.device):
            if self._z_serial[0] != serial:
                self.f.selected_inverse()
                self._z_serial = (serial, self._z_serial[1])
            self.f.inverse_on_pattern_dev(out.data_ptr())
        return out

    def _inverse_on_pattern_batch(self, nbatch, serial):
        out = torch.empty((nbatch, self.nnz), dtype=torch.float64, device=self.device)
        self._sync()
        with torch.cuda.device(self.device):
            if self._z_serial[1] != serial:
                self.f.selected_inverse_batch()
                self._z_serial = (self._z_serial[0], serial)
            self.f.inverse_on_pattern_batch_dev(out.data_ptr(), ldout=self.nnz)
        return out

    # ---- the public operations ----------------------------------------------------------------------
    def solve(self, val, B):
        """x = A(val)^-1 B.  val: (nnz,), B: (n,) or (n, nrhs); differentiable in both"""
        self._values(val, "val", (self.nnz,))
        self._rhs(B, "B", val.device)
        self._enter(val)
        return _Solve.apply(self, val, B)

    def logdet(self, val):
        """log det A(val), a 0-dim tensor; differentiable in val"""
        self._values(val, "val", (self.nnz,))
        self._enter(val)
        return _LogDet.apply(self, val)

    def solve_batch(self, vals, B):
        """X_b = A(vals[b])^-1 B[b].  vals: (nbatch, nnz), B: (nbatch, n, nrhs); differentiable in both"""
        if self.reproducible and not self.batch_reproducible:
            raise NotImplementedError("solve_batch" + _NO_DET_BATCH)
        self._values(vals, "vals", (None, self.nnz))
        self._tensor(B, "B", (vals.shape[0], self.n, None), vals.device)
        self._enter(vals)
        return _SolveBatch.apply(self, vals, B)

    def logdet_batch(self, vals):
        """log det A(vals[b]), shape (nbatch,); differentiable in vals"""
        if self.reproducible and not self.batch_reproducible:
            raise NotImplementedError("logdet_batch" + _NO_DET_BATCH)
        self._values(vals, "vals", (None, self.nnz))
        self._enter(vals)
        return _LogDetBatch.apply(self, vals)

    def pattern_outer(self, U, V, alpha=1.0):
        """out[k] = alpha sum_q (U[i, q] V[j, q] + [i != j] U[j, q] V[i, q]) at the k-th entry (i, j) of the pattern.
        U, V: (n, nvec) or (n,); not differentiable"""
        self._rhs(U, "U")
        self._tensor(V, "V", tuple(U.shape), U.device)
        self._enter(U)
        with torch.no_grad():
            ut = U.reshape(self.n, -1).t().contiguous()
            vt = V.reshape(self.n, -1).t().contiguous()
            return self._outer(ut, vt, float(alpha))

    def set_constraints(self, C):
        """Hard linear constraints C x = e for ``solve_constrained`` and ``sample(..., constrained=True)``, and for
        their batch forms ``solve_constrained_batch`` and ``sample_batch(..., constrained=True)``.  C: a
        float64 device tensor (k, n), k <= 64, or None to clear them.  The rows are copied to the handle with the
        next constrained operation (which has the factor they need); a later factorization is picked up by the
        library.  WITHOUT GRADIENTS: nothing that passes through the constraints carries a gradient, neither to
        val, nor to C, nor to B, mean or e."""
        self._C_on_batch = False
        if C is None:
            self._C = None
            if self.device is not None:
                with torch.cuda.device(self.device):
                    self.f.release_constraints()
                    self.f.release_constraints_batch()
            return self
        self._tensor(C, "C", (None, self.n))
        if not 1 <= C.shape[0] <= 64:
            raise ValueError(f"C: expected 1 to 64 rows, got {C.shape[0]}")
        self._C = (C.detach().contiguous().clone(), False)    # (rows, already on the handle)
        return self

    def _ensure_constraints(self):
        """the stored rows on the handle (the current factor is on the device); returns k"""
        if self._C is None:
            raise RuntimeError("SparseCholesky: no constraints (call set_constraints first)")
        rows, on_handle = self._C
        if not on_handle:
            self._sync()
            with torch.cuda.device(self.device):
                before = self.f.set_reproducible_solve(self.reproducible)
                try:
                    self.f.set_constraints_dev(rows.data_ptr(), rows.shape[0], ldc=self.n)
                finally:
                    self.f.set_reproducible_solve(before)
            self._C = (rows, True)
        return rows.shape[0]

    def _ensure_constraints_batch(self):
        """the stored rows on the handle's batch (the current batch is on the device); returns k"""
        if self._C is None:
            raise RuntimeError("SparseCholesky: no constraints (call set_constraints first)")
        rows = self._C[0]
        if not self._C_on_batch:
            self._sync()
            with torch.cuda.device(self.device):
                if self.f.set_constraints_batch_dev(rows.data_ptr(), rows.shape[0], ldc=self.n) < 0:
                    raise SplltError("spllt_hip_set_constraints_batch_dev", _NOT_POSDEF, self.f.last_error())
            self._C_on_batch = True
        return rows.shape[0]

    def solve_constrained_batch(self, vals, B, e=None):
        """x*_b = argmin 1/2 x^T A(vals[b]) x - B[b]^T x subject to C x = e, for every column of B[b] and every member
        in the same launches: the blocked batch solve, then the correction, in one library call.  vals: (nbatch,
        nnz), B: (nbatch, n, nrhs); e: None (zeros) or (k,).  Returns (x*, lambda) of shapes (nbatch, n, nrhs) and
        (nbatch, k, nrhs).  WITHOUT GRADIENTS (see set_constraints)."""
        if self.reproducible and not self.batch_reproducible:
            raise NotImplementedError("solve_constrained_batch" + _NO_DET_BATCH)
        self._values(vals, "vals", (None, self.nnz))
        self._tensor(B, "B", (vals.shape[0], self.n, None), vals.device)
        self._enter(vals)
        with torch.no_grad():
            self._ensure_batch(vals)
            k = self._ensure_constraints_batch()
            if e is not None:
                e = self._tensor(e, "e", (k,)).contiguous()
            work = B.detach().transpose(1, 2).contiguous().clone()
            lam = torch.empty((work.shape[0], work.shape[1], k), dtype=torch.float64, device=self.device)
            self._sync()
            with torch.cuda.device(self.device):
                self.f.constrain_batch_dev(work.data_ptr(), work.shape[1], ldx=self.n,
                                           e_dev_ptr=None if e is None else e.data_ptr(), lde=0,
                                           lambda_dev_ptr=lam.data_ptr(), ldl=k, entry="solve_constrained")
        return work.transpose(1, 2), lam.transpose(1, 2)

    def solve_constrained(self, val, B, e=None):
        """x* = argmin 1/2 x^T A(val) x - B^T x subject to C x = e, for every column of B: the blocked solve, then
        the correction, on device tensors in one library call.  B: (n,) or (n, nrhs); e: None (zeros) or (k,).
        Returns (x*, lambda), lambda (k,) or (k, nrhs) the Lagrange multipliers.  WITHOUT GRADIENTS (see
        set_constraints)."""
        self._values(val, "val", (self.nnz,))
        self._rhs(B, "B", val.device)
        self._enter(val)
        with torch.no_grad():
            self._ensure_factor(val)
            k = self._ensure_constraints()
            if e is not None:
                e = self._tensor(e, "e", (k,)).contiguous()
            work = B.detach().reshape(self.n, -1).t().contiguous().clone()
            lam = torch.empty((work.shape[0], k), dtype=torch.float64, device=self.device)
            self._sync()
            with torch.cuda.device(self.device):
                self.f.constrain_dev(work.data_ptr(), work.shape[0], ldx=self.n, e_dev_ptr=None if e is None else e.data_ptr(),
                                     lde=0, lambda_dev_ptr=lam.data_ptr(), ldl=k, entry="solve_constrained")
        x, lam = work.t(), lam.t()
        return (x[:, 0], lam[:, 0]) if B.dim() == 1 else (x, lam)

    def sample(self, val, nsamp, seed=0, kind="precision", mean=None, constrained=False, e=None):
        """nsamp draws of N(mean, A(val)^-1) (kind "precision") or N(mean, A(val)) ("covariance") from the cached
        factor of val: a float64 device tensor (n, nsamp); sample q is a function of (seed, q) alone
        (Factorization.sample).  The result carries NO gradient to val -- pathwise derivatives through L are out of
        scope -- but it does carry the gradient to mean (the identity).  reproducible=True: the precision kind
        goes through the reproducible solve and repeats bit for bit, like the covariance kind always does.
        constrained=True (kind "precision" only): draws of N(mean, A(val)^-1) | C x = e for the rows of
        set_constraints, e None (zeros) or (k,); WITHOUT GRADIENTS, to mean as well."""
        self._values(val, "val", (self.nnz,))
        if mean is not None:
            self._tensor(mean, "mean", (self.n,), val.device)
        self._enter(val)
        if constrained:
            if kind != "precision":
                raise ValueError("sample: constrained=True needs kind='precision'")
            with torch.no_grad():
                self._ensure_factor(val)
                k = self._ensure_constraints()
                if e is not None:
                    e = self._tensor(e, "e", (k,)).contiguous()
                m = None if mean is None else mean.detach().contiguous()
                work = torch.empty((int(nsamp), self.n), dtype=torch.float64, device=self.device)
                self._sync()
                with torch.cuda.device(self.device):
                    before = self.f.set_reproducible_solve(self.reproducible)
                    try:
                        self.f.sample_constrained_dev(work.data_ptr(), int(nsamp), ldx=self.n, seed=seed,
                                                      mean_dev_ptr=None if m is None else m.data_ptr(),
                                                      e_dev_ptr=None if e is None else e.data_ptr())
                    finally:
                        self.f.set_reproducible_solve(before)
            return work.t()
        if e is not None:
            raise ValueError("sample: e needs constrained=True")
        with torch.no_grad():
            self._ensure_factor(val)
            work = torch.empty((int(nsamp), self.n), dtype=torch.float64, device=self.device)
            self._sync()
            with torch.cuda.device(self.device):
                before = self.f.set_reproducible_solve(self.reproducible)
                try:
                    self.f.sample_dev(work.data_ptr(), int(nsamp), ldx=self.n, seed=seed, kind=kind)
                finally:
                    self.f.set_reproducible_solve(before)
        x = work.t()
        return x if mean is None else x + mean[:, None]

    def sample_batch(self, vals, nsamp, seed=0, kind="precision", mean=None, common_noise=False, constrained=False,
                     e=None):
        """nsamp draws per member of N(mean_b, A(vals[b])^-1) (kind "precision") or N(mean_b, A(vals[b]))
        ("covariance") from the cached factors of the batch (those of solve_batch / logdet_batch): a float64 device
        tensor (nbatch, n, nsamp).  vals: (nbatch, nnz); mean: (n,) for all members or (nbatch, n).  Member b draws
        from a noise stream of its own, common_noise=True gives every member the same noise (Factorization.sample_batch).
        The result carries NO gradient, neither to vals nor to mean, like the draws of ``sample`` with respect to val:
        it is computed under no_grad, mean added on the device (``rsample_batch`` draws the same bits with the
        pathwise gradient).  reproducible=True raises NotImplementedError, like the other batch operations.
        constrained=True (kind "precision" only): draws of N(mean_b, A(vals[b])^-1) | C x = e for the rows of
        set_constraints, e None (zeros) or (k,)."""
        if self.reproducible and not self.batch_reproducible:
            raise NotImplementedError("sample_batch" + _NO_DET_BATCH)
        if constrained and kind != "precision":
            raise ValueError("sample_batch: constrained=True needs kind='precision'")
        if e is not None and not constrained:
            raise ValueError("sample_batch: e needs constrained=True")
        self._values(vals, "vals", (None, self.nnz))
        ldmean = 0
        if mean is not None:
            if isinstance(mean, torch.Tensor) and mean.dim() == 2:
                self._tensor(mean, "mean", (vals.shape[0], self.n), vals.device)
                ldmean = self.n
            else:
                self._tensor(mean, "mean", (self.n,), vals.device)
        self._enter(vals)
        with torch.no_grad():
            self._ensure_batch(vals)
            work = torch.empty((vals.shape[0], int(nsamp), self.n), dtype=torch.float64, device=self.device)
            m = None if mean is None else mean.detach().contiguous()
            if constrained:
                k = self._ensure_constraints_batch()
                if e is not None:
                    e = self._tensor(e, "e", (k,)).contiguous()
            self._sync()
            with torch.cuda.device(self.device):
                before = self.f.set_batch_blocked_solve(self.batch_blocked)
                try:
                    if constrained:
                        self.f.sample_constrained_batch_dev(work.data_ptr(), int(nsamp), ldx=self.n, seed=seed,
                                                            mean_dev_ptr=None if m is None else m.data_ptr(),
                                                            ldmean=ldmean, e_dev_ptr=None if e is None else e.data_ptr(),
                                                            common_noise=common_noise)
                    else:
                        self.f.sample_batch_dev(work.data_ptr(), int(nsamp), ldx=self.n, seed=seed, kind=kind,
                                                mean_dev_ptr=None if m is None else m.data_ptr(), ldmean=ldmean,
                                                common_noise=common_noise)
                finally:
                    self.f.set_batch_blocked_solve(before)
        return work.transpose(1, 2)

    # ---- operations with the factor in the graph ------------------------------------------------------
    def _factor_op_inplace(self, work, op):
        """work: (nvec, n) contiguous, overwritten with op(L) applied to every vector (user layout)"""
        self._sync()
        with torch.cuda.device(self.device):
            job = 1 if op in ("L", "Linv") else 2
            if op in ("L", "Lt"):
                self.f.factor_mult_dev(work.data_ptr(), work.shape[0], ldx=self.n, job=job)
            elif self.reproducible:
                self.f.solve_reproducible_dev(work.data_ptr(), work.shape[0], ldx=self.n, job=job)
            else:
                self.f.solve_many_dev(work.data_ptr(), work.shape[0], ldx=self.n, job=job)
        return work

    def _factor_adjoint(self, a, b, alpha, b_pivot_order=False):
        """a, b: (nvec, n) contiguous -> d/dval of the seed alpha sum_q a_q b_q^T, (nnz,): seed passes of 32 vectors,
        one sweep, the reader"""
        nvec, step = a.shape[0], 32
        if nvec == 0:
            return torch.zeros(self.nnz, dtype=torch.float64, device=self.device)
        out = torch.empty(self.nnz, dtype=torch.float64, device=self.device)
        self._sync()
        with torch.cuda.device(self.device):
            for q in range(0, nvec, step):
                self.f.factor_adjoint_seed_dev(a[q:].data_ptr(), b[q:].data_ptr(), min(step, nvec - q), ld=self.n,
                                               alpha=alpha, accumulate=q > 0, b_pivot_order=b_pivot_order)
            self.f.factor_adjoint_dev(out.data_ptr())
        return out

    _FACTOR_OPS = ("L", "Lt", "Linv", "Ltinv")

    def factor_apply(self, val, X, op):
        """Y = op(L) X for the Cholesky factor P A(val) P^T = L L^T; op: "L", "Lt", "Linv", "Ltinv".  X: (n,) or
        (n, nvec), a pivot-order vector laid out in user positions as Factorization.factor_mult (job 1, 2) and
        solve_many (job 1, 2) take and leave it.  Differentiable in val and X; the backward pass is one library call
        for the gradient of X, then the seed, ONE sweep of the factor's adjoint and its reader for val."""
        if op not in self._FACTOR_OPS:
            raise ValueError(f"op: expected one of {self._FACTOR_OPS}, got {op!r}")
        self._values(val, "val", (self.nnz,))
        self._rhs(X, "X", val.device)
        self._enter(val)
        return _FactorApply.apply(self, val, X, op)

    def rsample(self, val, nsamp, seed=0, kind="precision", mean=None):
        """``sample`` with the pathwise gradient: the same bits forward, differentiable in val and mean.  The noise is
        not kept: the backward pass draws it again (covariance) or does not need it (precision)."""
        self._values(val, "val", (self.nnz,))
        if mean is not None:
            self._tensor(mean, "mean", (self.n,), val.device)
        if kind not in ("precision", "covariance"):
            raise ValueError(f"kind: expected 'precision' or 'covariance', got {kind!r}")
        self._enter(val)
        x = _RSample.apply(self, val, int(nsamp), int(seed), kind)
        return x if mean is None else x + mean[:, None]

    # ---- the same with the factors of a batch in the graph ---------------------------------------------
    def _factor_op_batch_inplace(self, work, op):
        """work: (nbatch, nvec, n) contiguous, overwritten with op(L_b) applied to every vector of member b"""
        self._sync()
        with torch.cuda.device(self.device):
            job = 1 if op in ("L", "Linv") else 2
            if op in ("L", "Lt"):
                self.f.factor_mult_batch_dev(work.data_ptr(), work.shape[1], ldx=self.n, job=job)
            elif self.batch_blocked:
                self.f.solve_many_batch_dev(work.data_ptr(), work.shape[1], ldx=self.n, job=job)
            else:
                self.f.solve_batch_dev(work.data_ptr(), work.shape[1], ldx=self.n, job=job)
        return work

    def _factor_adjoint_batch(self, a, b, alpha, b_pivot_order=False):
        """a, b: (nbatch, nvec, n) contiguous -> d/dvals of the seeds alpha sum_q a_bq b_bq^T, (nbatch, nnz): seed
        passes of 32 vectors per member, ONE sweep for all members, the reader"""
        nbatch, nvec, step = a.shape[0], a.shape[1], 32
        if nvec == 0:
            return torch.zeros((nbatch, self.nnz), dtype=torch.float64, device=self.device)
        out = torch.empty((nbatch, self.nnz), dtype=torch.float64, device=self.device)
        keep = []                     # (the passes' copies live until the library has read them)
        self._sync()
        with torch.cuda.device(self.device):
            for q in range(0, nvec, step):
                aq, bq = a, b
                if nvec > step:
                    aq, bq = a[:, q:q + step].contiguous(), b[:, q:q + step].contiguous()
                    keep.append((aq, bq))
                    self._sync()
                self.f.factor_adjoint_seed_batch_dev(aq.data_ptr(), bq.data_ptr(), aq.shape[1], ld=self.n, alpha=alpha,
                                                     accumulate=q > 0, b_pivot_order=b_pivot_order)
            self.f.factor_adjoint_batch_dev(out.data_ptr(), ldout=self.nnz)
        return out

    def factor_apply_batch(self, vals, X, op):
        """Y_b = op(L_b) X[b] for the Cholesky factors P A(vals[b]) P^T = L_b L_b^T; op: "L", "Lt", "Linv",
        "Ltinv".  vals: (nbatch, nnz), X: (nbatch, n, nvec), the vectors in the layout of ``factor_apply``.
        Differentiable in vals and X; the backward pass is one library call for the gradient of X, then seed passes
        of 32 vectors per member, ONE sweep of the batch's factor adjoint and its reader for vals."""
        if self.reproducible and not self.batch_reproducible:
            raise NotImplementedError("factor_apply_batch" + _NO_DET_BATCH)
        if op not in self._FACTOR_OPS:
            raise ValueError(f"op: expected one of {self._FACTOR_OPS}, got {op!r}")
        self._values(vals, "vals", (None, self.nnz))
        self._tensor(X, "X", (vals.shape[0], self.n, None), vals.device)
        self._enter(vals)
        return _FactorApplyBatch.apply(self, vals, X, op)

    def rsample_batch(self, vals, nsamp, seed=0, kind="precision", mean=None, common_noise=False):
        """``sample_batch`` with the pathwise gradient: the same bits forward, differentiable in vals and mean
        ((n,) or (nbatch, n); added outside the Function, its gradient is autograd's).  The noise is not kept: the
        backward pass draws it again (covariance) or does not need it (precision)."""
        if self.reproducible and not self.batch_reproducible:
            raise NotImplementedError("rsample_batch" + _NO_DET_BATCH)
        self._values(vals, "vals", (None, self.nnz))
        if mean is not None:
            if isinstance(mean, torch.Tensor) and mean.dim() == 2:
                self._tensor(mean, "mean", (vals.shape[0], self.n), vals.device)
            else:
                self._tensor(mean, "mean", (self.n,), vals.device)
        if kind not in ("precision", "covariance"):
            raise ValueError(f"kind: expected 'precision' or 'covariance', got {kind!r}")
        self._enter(vals)
        x = _RSampleBatch.apply(self, vals, int(nsamp), int(seed), kind, bool(common_noise))
        if mean is None:
            return x
        return x + (mean[:, :, None] if mean.dim() == 2 else mean[None, :, None])

    def close(self):
        self.f.close()


def _to_vectors(B):
    """(n,) or (n, nrhs) -> a fresh contiguous (nrhs, n) work tensor: the library wants every vector contiguous"""
    return B.detach().reshape(B.shape[0], -1).t().clone(memory_format=torch.contiguous_format)


class _Solve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, chol, val, B):
        ctx.chol = chol
        ctx.serial = chol._ensure_factor(val)
        work = chol._solve_inplace(_to_vectors(B))
        ctx.vector = B.dim() == 1
        ctx.save_for_backward(val, work)
        return work.view(-1) if ctx.vector else work.t()

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        chol = ctx.chol
        val, xt = ctx.saved_tensors
        if chol.f.factor_serial(0) != ctx.serial:       # another matrix was factorized in between
            chol._ensure_factor(val)
        lam = chol._solve_inplace(_to_vectors(grad))
        gval = chol._outer(lam, xt, -1.0) if ctx.needs_input_grad[1] else None
        return None, gval, (lam.view(-1) if ctx.vector else lam.t())


class _FactorApply(torch.autograd.Function):
    """Y = op(L) X; the table of the module docstring"""
    _ADJOINT = {"L": "Lt", "Lt": "L", "Linv": "Ltinv", "Ltinv": "Linv"}

    @staticmethod
    def forward(ctx, chol, val, X, op):
        ctx.chol, ctx.op = chol, op
        ctx.serial = chol._ensure_factor(val)
        work = chol._factor_op_inplace(_to_vectors(X), op)
        ctx.vector = X.dim() == 1
        # the products need their input, the solves their output
        ctx.save_for_backward(val, _to_vectors(X) if op in ("L", "Lt") else work)
        return work.view(-1) if ctx.vector else work.t()

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        chol, op = ctx.chol, ctx.op
        val, kept = ctx.saved_tensors
        if chol.f.factor_serial(0) != ctx.serial:       # another matrix was factorized in between
            chol._ensure_factor(val)
        gt = _to_vectors(grad)
        xbar = chol._factor_op_inplace(gt.clone(), _FactorApply._ADJOINT[op])
        gval = None
        if ctx.needs_input_grad[1]:
            if op == "L":
                gval = chol._factor_adjoint(gt, kept, 1.0)
            elif op == "Lt":
                gval = chol._factor_adjoint(kept, gt, 1.0)
            elif op == "Linv":
                gval = chol._factor_adjoint(xbar, kept, -1.0)
            else:
                gval = chol._factor_adjoint(kept, xbar, -1.0)
        return None, gval, (xbar.view(-1) if ctx.vector else xbar.t()), None


class _RSample(torch.autograd.Function):
    """x = P^T L^-T z (precision) or P^T L z (covariance), z the white noise of (seed, sample); the mean is added
    outside (its gradient is autograd's)"""

    @staticmethod
    def forward(ctx, chol, val, nsamp, seed, kind):
        ctx.chol, ctx.nsamp, ctx.seed, ctx.kind = chol, nsamp, seed, kind
        ctx.serial = chol._ensure_factor(val)
        work = torch.empty((nsamp, chol.n), dtype=torch.float64, device=chol.device)
        chol._sync()
        with torch.cuda.device(chol.device):
            before = chol.f.set_reproducible_solve(chol.reproducible)
            try:
                chol.f.sample_dev(work.data_ptr(), nsamp, ldx=chol.n, seed=seed, kind=kind)
            finally:
                chol.f.set_reproducible_solve(before)
        if kind == "precision":
            ctx.save_for_backward(val, work)
        else:
            ctx.save_for_backward(val)
        return work.t()

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        chol = ctx.chol
        val = ctx.saved_tensors[0]
        if not ctx.needs_input_grad[1]:
            return None, None, None, None, None
        if chol.f.factor_serial(0) != ctx.serial:
            chol._ensure_factor(val)
        gt = _to_vectors(grad)
        if ctx.kind == "precision":      # y = L^-T z: Lbar = -y (L^-1 ybar)^T
            u = chol._factor_op_inplace(gt, "Linv")
            gval = chol._factor_adjoint(ctx.saved_tensors[1], u, -1.0)
        else:                            # y = L z: Lbar = ybar z^T, z in pivot order as white_noise_dev writes it
            z = torch.empty((max(ctx.nsamp, 1), chol.n), dtype=torch.float64, device=chol.device)
            chol._sync()
            with torch.cuda.device(chol.device):
                chol.f.white_noise_dev(z.data_ptr(), ctx.nsamp, ldz=chol.n, seed=ctx.seed)
            gval = chol._factor_adjoint(gt, z[:ctx.nsamp], 1.0, b_pivot_order=True)
        return None, gval, None, None, None


def _to_batch_vectors(B):
    """(nbatch, n, nvec) -> a fresh contiguous (nbatch, nvec, n) work tensor"""
    return B.detach().transpose(1, 2).clone(memory_format=torch.contiguous_format)


class _FactorApplyBatch(torch.autograd.Function):
    """Y_b = op(L_b) X_b; the table of the module docstring per member"""

    @staticmethod
    def forward(ctx, chol, vals, X, op):
        ctx.chol, ctx.op = chol, op
        ctx.serial = chol._ensure_batch(vals)
        work = chol._factor_op_batch_inplace(_to_batch_vectors(X), op)
        # the products need their input, the solves their output
        ctx.save_for_backward(vals, _to_batch_vectors(X) if op in ("L", "Lt") else work)
        return work.transpose(1, 2)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        chol, op = ctx.chol, ctx.op
        vals, kept = ctx.saved_tensors
        if chol.f.factor_serial(1) != ctx.serial:       # another batch was factorized in between
            chol._ensure_batch(vals)
        gt = _to_batch_vectors(grad)
        xbar = chol._factor_op_batch_inplace(gt.clone(), _FactorApply._ADJOINT[op])
        gvals = None
        if ctx.needs_input_grad[1]:
            if op == "L":
                gvals = chol._factor_adjoint_batch(gt, kept, 1.0)
            elif op == "Lt":
                gvals = chol._factor_adjoint_batch(kept, gt, 1.0)
            elif op == "Linv":
                gvals = chol._factor_adjoint_batch(xbar, kept, -1.0)
            else:
                gvals = chol._factor_adjoint_batch(kept, xbar, -1.0)
        return None, gvals, xbar.transpose(1, 2), None


class _RSampleBatch(torch.autograd.Function):
    """x_b = P^T L_b^-T z_b (precision) or P^T L_b z_b (covariance), z_b the white noise of (seed, member's stream,
    sample); the mean is added outside (its gradient is autograd's)"""

    @staticmethod
    def forward(ctx, chol, vals, nsamp, seed, kind, common_noise):
        ctx.chol, ctx.nsamp, ctx.seed, ctx.kind, ctx.common = chol, nsamp, seed, kind, common_noise
        ctx.serial = chol._ensure_batch(vals)
        work = torch.empty((vals.shape[0], nsamp, chol.n), dtype=torch.float64, device=chol.device)
        chol._sync()
        with torch.cuda.device(chol.device):
            before = chol.f.set_batch_blocked_solve(chol.batch_blocked)
            try:
                chol.f.sample_batch_dev(work.data_ptr(), nsamp, ldx=chol.n, seed=seed, kind=kind, common_noise=common_noise)
            finally:
                chol.f.set_batch_blocked_solve(before)
        if kind == "precision":
            ctx.save_for_backward(vals, work)
        else:
            ctx.save_for_backward(vals)
        return work.transpose(1, 2)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        chol = ctx.chol
        vals = ctx.saved_tensors[0]
        if not ctx.needs_input_grad[1]:
            return None, None, None, None, None, None
        if chol.f.factor_serial(1) != ctx.serial:
            chol._ensure_batch(vals)
        gt = _to_batch_vectors(grad)
        if ctx.kind == "precision":      # y = L^-T z: Lbar = -y (L^-1 ybar)^T
            u = chol._factor_op_batch_inplace(gt, "Linv")
            gvals = chol._factor_adjoint_batch(ctx.saved_tensors[1], u, -1.0)
        else:                            # y = L z: Lbar = ybar z^T, z in pivot order as white_noise_batch_dev writes it
            z = torch.empty((vals.shape[0], max(ctx.nsamp, 1), chol.n), dtype=torch.float64, device=chol.device)
            chol._sync()
            with torch.cuda.device(chol.device):
                chol.f.white_noise_batch_dev(z.data_ptr(), ctx.nsamp, ldz=chol.n, seed=ctx.seed, common_noise=ctx.common)
            gvals = chol._factor_adjoint_batch(gt, z if ctx.nsamp > 0 else z[:, :0], 1.0, b_pivot_order=True)
        return None, gvals, None, None, None, None


class _LogDet(torch.autograd.Function):
    @staticmethod
    def forward(ctx, chol, val):
        ctx.chol = chol
        ctx.serial = chol._ensure_factor(val)
        chol._sync()
        with torch.cuda.device(chol.device):
            ld = chol.f.log_det()
        ctx.save_for_backward(val)
        return torch.tensor(ld, dtype=torch.float64, device=chol.device)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        chol = ctx.chol
        (val,) = ctx.saved_tensors
        serial = ctx.serial
        if chol.f.factor_serial(0) != serial:
            serial = chol._ensure_factor(val)
        return None, chol._weights() * chol._inverse_on_pattern(serial) * grad


class _SolveBatch(torch.autograd.Function):
    @staticmethod
    def forward(ctx, chol, vals, B):
        ctx.chol = chol
        ctx.serial = chol._ensure_batch(vals)
        work = chol._solve_batch_inplace(B.detach().transpose(1, 2).clone(memory_format=torch.contiguous_format))
        ctx.save_for_backward(vals, work)
        return work.transpose(1, 2)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        chol = ctx.chol
        vals, xt = ctx.saved_tensors
        if chol.f.factor_serial(1) != ctx.serial:
            chol._ensure_batch(vals)
        lam = chol._solve_batch_inplace(grad.transpose(1, 2).clone(memory_format=torch.contiguous_format))
        gvals = chol._outer_batch(lam, xt, -1.0) if ctx.needs_input_grad[1] else None
        return None, gvals, lam.transpose(1, 2)


class _LogDetBatch(torch.autograd.Function):
    @staticmethod
    def forward(ctx, chol, vals):
        ctx.chol = chol
        ctx.serial = chol._ensure_batch(vals)
        chol._sync()
        with torch.cuda.device(chol.device):
            ld = chol.f.log_det_batch()
        ctx.save_for_backward(vals)
        return torch.as_tensor(ld, dtype=torch.float64, device=chol.device)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        chol = ctx.chol
        (vals,) = ctx.saved_tensors
        serial = ctx.serial
        if chol.f.factor_serial(1) != serial:
            serial = chol._ensure_batch(vals)
        return None, chol._weights() * chol._inverse_on_pattern_batch(vals.shape[0], serial) * grad[:, None]
