// The iteration of the refined solves, once: iterative refinement and factor-preconditioned CG on the work vectors
// of one group (single handle) or one pass (the members of a batch).  Host only: the driver names the six work
// arrays and the selector arrays of refine.hpp and hands every operation to a backend, which knows where they are
// and how they are launched (engine_solve.cpp: Engine::RefineBackend, Engine::RefineBatchBackend;
// tests/native/refine_driver_test.cpp: a scripted one that records the sequence).
//
// A pair is one vector of one member (single handle: one vector).  be.readback(out) fills out[g] = best confirmed
// error and out[be.stride() + g] = state of pair g (0 iterating, 1 converged, 2 failed).
//
//   int  pairs() / stride() / vslots() / sslots()      slots: the partials of a vector kernel / of a product
//   bool fits()                                        false once a launch overflowed a grid (batch)
//   int  permute_in()                                  the caller's vectors -> B
//   void dot(a, b, sel, want, residual_like)           partials a.b
//   void finalize(stage, nslots, flag)                 second stage of a reduction and its scalar step
//   void copy(dst, src, sel, want, zero_others)
//   int  apply_factor(v)                               v = M^-1 v, all columns
//   void spmv(x, b, y, sel, want, partials)            y = A x (b = RFV_NONE) or y = b - A x
//   void axpy(alpha, x, p, r, q, sel, want, partials)  x += alpha p (alpha false: 1); r -= alpha q unless RFV_NONE
//   void pupdate(p, z, sel, want)                      p = z + beta p
//   int  readback(out)
//   int  permute_out(src)                              src -> the caller's vectors
//   int  finish()                                      the stream idle; the code of the group / pass
//
// A vector takes part in a kernel when sel is RFSEL_ALL or its entry of the selector array equals want.
#pragma once
#include <cstddef>
#include <vector>

#include "refine.hpp"

namespace spx {

enum RfVec { RFV_NONE = -1, RFV_B = 0, RFV_X, RFV_R, RFV_P, RFV_Q, RFV_XB };   // (the storage order of the work arrays)
enum RfSel { RFSEL_ALL = 0, RFSEL_ST, RFSEL_DECL, RFSEL_IMPROVE };

// method 0: refinement, 1: PCG.  its[g] = applications of M^-1 to pair g after the first; out: the last readback.
// Returns the first non-zero code of permute_in, apply_factor, readback or permute_out (nothing further is
// enqueued), else that of finish().
template <class Backend>
int refine_iterate(Backend& be, int method, int max_iter, std::vector<int>& its, std::vector<double>& out) {
  const size_t np = (size_t)be.pairs(), stride = (size_t)be.stride();
  const int vslots = be.vslots(), sslots = be.sslots();
  its.assign(np, 0);
  out.assign(2 * stride, 0.0);
  int rc = 0;
  if ((rc = be.permute_in())) return rc;
  be.dot(RFV_B, RFV_B, RFSEL_ALL, 0, true);
  be.finalize(RFS_BNORM, vslots, 0);
  // x = M^-1 b, r = b - A x, the error of the first iterate
  be.copy(RFV_X, RFV_B, RFSEL_ALL, 0, false);
  if (!be.fits()) return be.finish();   // (no sweep on vectors that were not written)
  if ((rc = be.apply_factor(RFV_X))) return rc;
  auto true_residual = [&](RfSel sel, int want, int flag) {
    be.spmv(RFV_X, RFV_B, RFV_R, sel, want, true);
    be.finalize(RFS_TRUE, sslots, flag);
    be.copy(RFV_XB, RFV_X, RFSEL_IMPROVE, 1, false);   // the best confirmed iterate
  };
  true_residual(RFSEL_ST, 0, 0);
  if ((rc = be.readback(out))) return rc;
  auto active = [&]() {
    for (size_t g = 0; g < np; ++g)
      if (out[stride + g] == 0.0) return true;
    return false;
  };
  for (int it = 0; it < max_iter && be.fits() && active();) {
    ++it;
    for (size_t g = 0; g < np; ++g)
      if (out[stride + g] == 0.0) its[g] = it;
    if (method == 0) {
      // x += M^-1 r ; r = b - A x
      be.copy(RFV_P, RFV_R, RFSEL_ST, 0, true);   // (frozen vectors: a zero column for the sweep)
      if ((rc = be.apply_factor(RFV_P))) return rc;
      be.axpy(false, RFV_X, RFV_P, RFV_NONE, RFV_NONE, RFSEL_ST, 0, false);
      true_residual(RFSEL_ST, 0, 0);
    } else {
      // z = M^-1 r (in q) ; beta = r.z / (r.z)_old, 0 after a restart ; p = z + beta p
      be.copy(RFV_Q, RFV_R, RFSEL_ST, 0, true);   // (frozen vectors: a zero column for the sweep)
      if ((rc = be.apply_factor(RFV_Q))) return rc;
      be.dot(RFV_R, RFV_Q, RFSEL_ST, 0, false);
      be.finalize(RFS_BETA, vslots, 0);
      be.pupdate(RFV_P, RFV_Q, RFSEL_ST, 0);
      // q = A p with the partials of p.q ; alpha = r.z / p.q ; x += alpha p, r -= alpha q
      be.spmv(RFV_P, RFV_NONE, RFV_Q, RFSEL_ST, 0, true);
      be.finalize(RFS_ALPHA, sslots, 0);
      be.axpy(true, RFV_X, RFV_P, RFV_R, RFV_Q, RFSEL_ST, 0, true);
      be.finalize(RFS_REC, vslots, 0);
      // what the recurrence declares converged is confirmed with a true residual (no work if nothing is declared)
      true_residual(RFSEL_DECL, 1, 1);
    }
    if ((rc = be.readback(out))) return rc;
  }
  if (method == 1 && be.fits() && active()) {
    // out of iterations: the error reported is that of a true residual
    be.finalize(RFS_FINAL, 0, 0);
    true_residual(RFSEL_DECL, 1, 1);
    if ((rc = be.readback(out))) return rc;
  }
  if ((rc = be.permute_out(RFV_XB))) return rc;
  return be.finish();
}

}  // namespace spx
