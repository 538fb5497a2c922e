"""Numpy side of the sparse right-hand-side solves of a batch: an interpreter of the BATCH's substitution program
(the "bsolve_*" tables of spllt_hip_program_get: panel width and chain block 64 whatever the handle's), restricted
to given sets of block columns, on the vectors of several members at once -- every surviving entry of a launch is
applied to all members before the next one, as a launch that carries all members does.  Reads the symbolic tables and
the program only; the plan under test comes from the library and is passed in."""
import numpy as np
import scipy.linalg as sl

from solve_sparse_emulate import SR, touched_rows


def emulate_solve_sparse_batch(f, arenas, y, fwd, bwd, job=0):
    """arenas: one dense arena per member; y: (members, nrhs, n) in pivot order, modified in place.  Returns the
    number of launches that survive the filter (the same for every number of members)."""
    units, lst, tiles = f.program("bsolve_units"), f.program("bsolve_list"), f.program("bsolve_tiles")
    assert (units["pw"] == 64).all() and (units["cb"] == 64).all()
    rlist = f.sym("rlist")
    fwd, bwd = set(int(b) for b in fwd), set(int(b) for b in bwd)
    kept = 0

    def blk(u, arena):
        w, nr, off = int(u["w"]), int(u["nrow"]), int(u["off"])
        return arena[off:off + nr * w].reshape(nr, w)

    def run(launches, keep):
        nonlocal kept
        for kind, _lev, first, count in launches:
            some = False
            if kind in (0, 3):       # DIAG forward / backward
                for b in lst[first:first + count]:
                    if int(b) not in keep:
                        continue
                    some = True
                    u = units[int(b)]
                    w = int(u["w"])
                    idx = rlist[int(u["idx_off"]):int(u["idx_off"]) + w]
                    for m, arena in enumerate(arenas):
                        y[m][:, idx] = sl.solve_triangular(np.tril(blk(u, arena)[:w]), y[m][:, idx].T, lower=True,
                                                           trans="N" if kind == 0 else "T").T
            else:                    # STRIP forward (1) / backward (2)
                for tl in tiles[first:first + count]:
                    if int(tl["unit"]) not in keep:
                        continue
                    some = True
                    u = units[int(tl["unit"])]
                    w, nr = int(u["w"]), int(u["nrow"])
                    idx = rlist[int(u["idx_off"]):int(u["idx_off"]) + nr]
                    r0 = w + int(tl["ti"]) * SR
                    r1 = min(r0 + SR, nr)
                    for m, arena in enumerate(arenas):
                        B = blk(u, arena)
                        if kind == 1:
                            y[m][:, idx[r0:r1]] -= y[m][:, idx[:w]] @ B[r0:r1].T
                        else:
                            y[m][:, idx[:w]] -= y[m][:, idx[r0:r1]] @ B[r0:r1]
            kept += 1 if some else 0

    if job in (0, 1):
        run(f.program("bsolve_fwd"), fwd)
    if job in (0, 2):
        run(f.program("bsolve_bwd"), bwd)
    return kept


def run_filtered_batch(f, t, arenas, B, vals, wanted, job, fwd, bwd):
    """The interpreter from vectors that are NaN outside the touched rows.  B: scipy CSC in canonical order (the
    pattern); vals: (members, nnz(B)).  Returns (values at the wanted positions (members, nwanted, k), the vectors,
    the touched mask)."""
    n, k = B.shape
    order = t["order"]
    touched = touched_rows(t, fwd, bwd, wanted)
    y = np.full((len(arenas), k, n), np.nan)
    y[:, :, touched] = 0.0
    for c in range(k):
        for e in range(B.indptr[c], B.indptr[c + 1]):
            p = int(order[B.indices[e]])
            if touched[p]:
                y[:, c, p] = vals[:, e]
    emulate_solve_sparse_batch(f, arenas, y, fwd, bwd, job)
    return y[:, :, wanted].transpose(0, 2, 1), y, touched
