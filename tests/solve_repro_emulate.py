"""Numpy interpreter of the reproducible substitution: the launches of "solve_fwd" / "solve_bwd" with the
strip products stored in a scratch vector and subtracted by the diagonal launches in the order of the
"rsolve_*" tables (include/spllt_hip.h).  Reads nothing but those tables, the substitution program and rlist."""
import numpy as np
import scipy.linalg as sl

SR = 64  # kSolveStripRows


def tables(f):
    return {k: f.program("rsolve_" + k) for k in ("fslot", "bfirst", "gptr", "gsrc", "bslot", "frows", "bsize")}


def emulate_solve_repro(f, arena, y, job=0):
    """y: (nrhs, n) in pivot order, modified in place.  The scratch starts full of NaN before every sweep: a
    slot that is read without having been written in that sweep poisons the result."""
    units, lst, tiles = f.program("solve_units"), f.program("solve_list"), f.program("solve_tiles")
    fwd, bwd = f.program("solve_fwd"), f.program("solve_bwd")
    rlist = f.sym("rlist")
    t = tables(f)
    scratch = np.empty((y.shape[0], max(t["frows"], t["bsize"], 1)))

    def blk(u):
        w, nr, off = int(u["w"]), int(u["nrow"]), int(u["off"])
        return arena[off:off + nr * w].reshape(nr, w), rlist[int(u["idx_off"]):int(u["idx_off"]) + nr], w

    def run(launches):
        scratch[:] = np.nan
        for kind, _lev, first, count in launches:
            if kind in (0, 3):       # DIAG forward / backward: gather in table order, then the tile solve
                for b in lst[first:first + count]:
                    b = int(b)
                    B, idx, w = blk(units[b])
                    rhs = y[:, idx[:w]].copy()
                    if kind == 0:
                        for j, p in enumerate(idx[:w]):
                            for k in range(int(t["gptr"][p]), int(t["gptr"][p + 1])):
                                rhs[:, j] -= scratch[:, int(t["gsrc"][k])]
                    else:
                        ns = (B.shape[0] - w + SR - 1) // SR
                        for s in range(ns):
                            o = int(t["bfirst"][b]) + s * w
                            rhs -= scratch[:, o:o + w]
                    y[:, idx[:w]] = sl.solve_triangular(np.tril(B[:w]), rhs.T, lower=True,
                                                        trans="N" if kind == 0 else "T").T
            else:                    # STRIP forward (1) / backward (2): the product is stored
                for i in range(first, first + count):
                    b, ti = int(tiles[i]["unit"]), int(tiles[i]["ti"])
                    B, idx, w = blk(units[b])
                    r0 = w + ti * SR
                    r1 = min(r0 + SR, B.shape[0])
                    if kind == 1:
                        o = int(t["fslot"][b]) + r0 - w
                        scratch[:, o:o + r1 - r0] = y[:, idx[:w]] @ B[r0:r1].T
                    else:
                        o = int(t["bslot"][i])
                        scratch[:, o:o + w] = y[:, idx[r0:r1]] @ B[r0:r1]

    if job in (0, 1):
        run(fwd)
    if job in (0, 2):
        run(bwd)
    return y
