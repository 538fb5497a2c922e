"""Numpy side of the sparse right-hand-side solve: the brute-force reach of a set of pivot positions in the
structure of L, the touched rows of a plan, and an interpreter of the exported substitution program restricted
to given sets of block columns.  Reads the symbolic tables and the "solve_*" program only; the plan under test
comes from the library and is passed in."""
import numpy as np
import scipy.linalg as sl

SR = 64  # kSolveStripRows


def bcol_of(t, nb, p):
    """the block column that holds pivot position p"""
    s = int(np.searchsorted(t["sptr"], p, side="right")) - 1
    return int(t["node_bcol0"][s]) + (p - int(t["sptr"][s])) // nb


def bcol_rows(t, b):
    """pivot positions of the rows of block column b (its own columns first)"""
    s, r0, nr = int(t["bcol_node"][b]), int(t["bcol_r0"][b]), int(t["bcol_nrow"][b])
    return t["rlist"][int(t["rptr"][s]) + r0:int(t["rptr"][s]) + r0 + nr]


def brute_reach(t, nb, positions):
    """Block columns a substitution started at `positions` can reach: the closure of "block column b writes the
    rows of its row list" -- a graph search over the row lists, with no use of the tree."""
    seen, stack = set(), [bcol_of(t, nb, int(p)) for p in positions]
    while stack:
        b = stack.pop()
        if b in seen:
            continue
        seen.add(b)
        for r in bcol_rows(t, b):
            c = bcol_of(t, nb, int(r))
            if c not in seen:
                stack.append(c)
    return np.array(sorted(seen), dtype=np.int64)


def touched_rows(t, fwd, bwd, wanted):
    """boolean mask over the pivot positions: own columns of the block columns of either set + wanted positions"""
    n = int(t["sptr"][-1])
    m = np.zeros(n, dtype=bool)
    for b in list(fwd) + list(bwd):
        w = int(t["bcol_width"][b])
        m[bcol_rows(t, int(b))[:w]] = True
    m[np.asarray(wanted, dtype=np.int64)] = True
    return m


def emulate_solve_sparse(f, arena, y, fwd, bwd, job=0):
    """The launches of "solve_fwd" / "solve_bwd" with the entries whose block column is in fwd / bwd; y: (nrhs, n)
    in pivot order, modified in place.  Returns the number of launches that survive."""
    units, lst, tiles = f.program("solve_units"), f.program("solve_list"), f.program("solve_tiles")
    rlist = f.sym("rlist")
    fwd, bwd = set(int(b) for b in fwd), set(int(b) for b in bwd)
    kept = 0

    def blk(u):
        w, nr, off = int(u["w"]), int(u["nrow"]), int(u["off"])
        return arena[off:off + nr * w].reshape(nr, w), rlist[int(u["idx_off"]):int(u["idx_off"]) + nr], w

    def run(launches, keep):
        nonlocal kept
        for kind, _lev, first, count in launches:
            some = False
            if kind in (0, 3):       # DIAG forward / backward
                for b in lst[first:first + count]:
                    if int(b) not in keep:
                        continue
                    some = True
                    B, idx, w = blk(units[int(b)])
                    y[:, idx[:w]] = sl.solve_triangular(np.tril(B[:w]), y[:, idx[:w]].T, lower=True,
                                                        trans="N" if kind == 0 else "T").T
            else:                    # STRIP forward (1) / backward (2)
                for tl in tiles[first:first + count]:
                    if int(tl["unit"]) not in keep:
                        continue
                    some = True
                    B, idx, w = blk(units[int(tl["unit"])])
                    r0 = w + int(tl["ti"]) * SR
                    r1 = min(r0 + SR, B.shape[0])
                    if kind == 1:
                        y[:, idx[r0:r1]] -= y[:, idx[:w]] @ B[r0:r1].T
                    else:
                        y[:, idx[:w]] -= y[:, idx[r0:r1]] @ B[r0:r1]
            kept += 1 if some else 0

    if job in (0, 1):
        run(f.program("solve_fwd"), fwd)
    if job in (0, 2):
        run(f.program("solve_bwd"), bwd)
    return kept
