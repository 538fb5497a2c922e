"""numpy interpreter of the low-rank update / downdate (spllt_hip_updown, updown.hip): the recurrence of
DESIGN.md section 14 applied to a dense arena through the exported symbolic tables, block column by block
column in the order of a plan.

Per column j of a block column and per vector q (q fastest):
    d = L_jj;  r = sqrt(d*d + sign*w_j*w_j);  c = r/d;  t = w_j/d;  L_jj = r
    rows i > j of the block column:  L_ij = (L_ij + sign*t*w_i)/c;  w_i = c*w_i - t*L_ij
The rows "below" include the later columns of the same node: a block column is self-contained, w is addressed
through the block column's row list."""
import numpy as np


def pivot_columns(t, W):
    """W (n x k, user variable order, dense or scipy sparse) as a dense array in pivot order"""
    W = np.asarray(W.todense()) if hasattr(W, "todense") else np.asarray(W, dtype=np.float64)
    W = W.reshape(W.shape[0], -1)
    Wp = np.zeros(W.shape)
    Wp[t["order"]] = W
    return Wp


def updown(t, arena, plan, Wp, sign):
    """arena (modified in place): the factor; plan: block columns, ascending; Wp: n x k in pivot order, modified
    in place (what the sweep leaves in it; the library zeroes its own work array instead).  Returns the smallest
    pivot position at which d*d + sign*w_j*w_j <= 0 (the sweep goes on with r = d there), or -1."""
    bad = -1
    k = Wp.shape[1]
    with np.errstate(over="ignore", invalid="ignore"):     # (after a failed pivot the numbers mean nothing)
        return _sweep(t, arena, plan, Wp, sign, k, bad)


def _sweep(t, arena, plan, Wp, sign, k, bad):
    for b in plan:
        s = int(t["bcol_node"][b])
        w, nr, off, r0 = (int(t["bcol_width"][b]), int(t["bcol_nrow"][b]), int(t["bcol_off"][b]), int(t["bcol_r0"][b]))
        rows = t["rlist"][t["rptr"][s] + r0:t["rptr"][s] + r0 + nr]
        blk = arena[off:off + nr * w].reshape(nr, w)          # a view
        for j in range(w):
            below = rows[j + 1:]
            for q in range(k):
                d = blk[j, j]
                wj = Wp[rows[j], q]
                r2 = d * d + sign * wj * wj
                if not r2 > 0.0:
                    if bad < 0:
                        bad = int(rows[j])
                    r2 = d * d
                r = np.sqrt(r2)
                c, tt = r / d, wj / d
                blk[j, j] = r
                blk[j + 1:, j] = (blk[j + 1:, j] + sign * tt * Wp[below, q]) / c
                Wp[below, q] = c * Wp[below, q] - tt * blk[j + 1:, j]
    return bad


def tree_path_plan(t, nb, firsts):
    """the union, over the first pivot positions `firsts`, of: the block column holding j and the later block
    columns of its node, and every block column of every ancestor node; sorted"""
    sptr, sparent, bcol_node = t["sptr"], t["sparent"], t["bcol_node"]
    nn = len(sparent)
    node_of = np.repeat(np.arange(nn), np.diff(sptr))
    first_bcol = {}
    for b, s in enumerate(bcol_node):
        first_bcol.setdefault(int(s), b)
    out = set()
    for j in firsts:
        s = int(node_of[j])
        b0 = first_bcol[s] + (int(j) - int(sptr[s])) // nb
        out |= {b for b in range(b0, len(bcol_node)) if bcol_node[b] == s}
        a = int(sparent[s])
        while a < nn:
            out |= {b for b in range(len(bcol_node)) if bcol_node[b] == a}
            a = int(sparent[a])
    return np.array(sorted(out), dtype=np.int32)


def edge_columns(A, k, rng):
    """n x k sparse W whose columns have clique patterns of A: alternately a e_i + b e_j on a random off-diagonal
    entry (i, j) of A and a single a e_i"""
    import scipy.sparse as sp
    C = sp.tril(sp.coo_matrix(A), -1)
    rows, cols, vals = [], [], []
    for q in range(k):
        if q % 2 == 0:
            e = int(rng.integers(len(C.row)))
            rows += [int(C.row[e]), int(C.col[e])]
            cols += [q, q]
            vals += [float(rng.uniform(0.5, 1.5)), -float(rng.uniform(0.5, 1.5))]
        else:
            rows.append(int(rng.integers(A.shape[0])))
            cols.append(q)
            vals.append(float(rng.uniform(0.5, 1.5)))
    return sp.csc_matrix((vals, (rows, cols)), shape=(A.shape[0], k))


def fill_column(t, A):
    """one column a e_i + b e_j whose pair of pivot positions lies in the structure of L (row list of the
    supernode of the smaller one) but is NOT an entry of A: a fill position; None when L has no fill"""
    import scipy.sparse as sp
    A = sp.csr_matrix(A)
    inv = np.empty(len(t["order"]), dtype=np.int64)
    inv[t["order"]] = np.arange(len(t["order"]))
    for s in range(len(t["sparent"])):
        rows = t["rlist"][t["rptr"][s]:t["rptr"][s + 1]]
        j = int(t["sptr"][s])
        for p in rows[::-1]:
            if p > j and A[inv[j], inv[p]] == 0:
                return sp.csc_matrix(([0.75, -1.25], ([int(inv[j]), int(inv[p])], [0, 0])), shape=(A.shape[0], 1))
    return None
