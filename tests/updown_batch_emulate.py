"""numpy interpreter of the low-rank update / downdate of the factors of a batch (spllt_hip_updown_batch,
batch_updown.hip): the interpreter of updown_emulate.py per member, pass by pass (8 columns) and block column by
block column in the order of the library's plan of the pass, with the two exits of the generate kernel:

  1. a member that is flagged (not positive definite before the call, or after an earlier pass of it) is skipped;
  2. a block column whose own columns hold only zeros in the member's work array is skipped: every rotation would
     be c = 1, t = 0.  Its arena entries are neither read nor written.

One pattern for all members, each member its own values."""
import numpy as np
import scipy.sparse as sp

import updown_emulate as em

VEC = 8


def canonical(W):
    """W as the library sees it: CSC, rows ascending within a column, stored zeros kept"""
    W = sp.csc_matrix(W, dtype=np.float64, copy=True)
    W.sum_duplicates()
    W.sort_indices()
    return W


def passes(f, W):
    """[(columns of the pass, the library's plan for them)]: the non-empty columns of W in groups of 8"""
    W = canonical(W)
    cols = [v for v in range(W.shape[1]) if W.indptr[v + 1] > W.indptr[v]]
    out = []
    for c0 in range(0, len(cols), VEC):
        cs = cols[c0:c0 + VEC]
        out.append((cs, f.updown_plan(_pattern_ones(W[:, cs]))))
    return out


def _pattern_ones(W):
    W = W.copy()
    W.data[:] = 1.0          # (the plan follows from the pattern; a stored zero still belongs to it)
    return W


def member_columns(t, W, vals_b):
    """member b's W_b (n x k, pivot order, dense) from the shared pattern and its values in W's CSC order"""
    W = canonical(W)
    Wb = sp.csc_matrix((np.asarray(vals_b, dtype=np.float64), W.indices, W.indptr), shape=W.shape)
    return em.pivot_columns(t, Wb)


def member_matrix(W, vals_b):
    W = canonical(W)
    return sp.csc_matrix((np.asarray(vals_b, dtype=np.float64), W.indices, W.indptr), shape=W.shape)


def updown_batch(t, f, arenas, W, vals, sign, flags=None, exit_rule=True):
    """arenas: one array per member, modified in place; vals: (B, nnz(W)); flags: per member None / 0 (clear) or the
    1-based pivot position it failed at before the call.  Returns (flags after the call, per member the set of
    block columns the sweep wrote)."""
    B = len(arenas)
    flags = [0] * B if flags is None else [int(x) for x in flags]
    plan_passes = passes(f, W)
    written = [set() for _ in range(B)]
    for m in range(B):
        Wp_all = member_columns(t, W, vals[m])
        for cs, plan in plan_passes:
            if flags[m]:
                break                                        # exit 1
            Wp = np.ascontiguousarray(Wp_all[:, cs])
            bad = -1
            for b in plan:
                s = int(t["bcol_node"][b])
                w, r0 = int(t["bcol_width"][b]), int(t["bcol_r0"][b])
                own = t["rlist"][t["rptr"][s] + r0:t["rptr"][s] + r0 + w]
                if exit_rule and not np.any(Wp[own] != 0.0):
                    continue                                 # exit 2
                with np.errstate(over="ignore", invalid="ignore"):
                    got = em._sweep(t, arenas[m], [b], Wp, sign, Wp.shape[1], -1)
                written[m].add(int(b))
                if got >= 0 and bad < 0:
                    bad = got
            if bad >= 0:
                flags[m] = bad + 1
    return flags, written


def leave_one_out(W, scale, B):
    """values for B members on the pattern of W: member b non-zero in column b mod k only"""
    W = canonical(W)
    k = W.shape[1]
    col_of = np.repeat(np.arange(k), np.diff(W.indptr))
    vals = np.zeros((B, W.nnz))
    for b in range(B):
        sel = col_of == b % k
        vals[b, sel] = W.data[sel] * scale[b]
    return vals
