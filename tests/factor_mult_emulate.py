"""Numpy interpreter of the factor products (factor_mult.hip): both directions with every sum in the order of
the "rsolve_*" tables (include/spllt_hip.h).  Reads nothing but those tables, "solve_units" / "solve_tiles",
rlist and the arena; of a diagonal tile only the lower triangle (np.where, not a product with a mask: what
sits in the strict upper part, NaN included, cannot reach the result)."""
import numpy as np

SR = 64  # kSolveStripRows


def tables(f):
    return {k: f.program("rsolve_" + k) for k in ("fslot", "bfirst", "gptr", "gsrc", "bslot", "frows", "bsize")}


def emulate_factor_mult(f, arena, X, transpose):
    """X: (n, k) in pivot order.  Returns L X (transpose: L^T X).  The scratch starts full of NaN: a slot that is
    read without having been written poisons the result."""
    units, tiles = f.program("solve_units"), f.program("solve_tiles")
    rlist = f.sym("rlist")
    t = tables(f)
    scratch = np.full((max(t["frows"], t["bsize"], 1), X.shape[1]), np.nan)
    Y = np.full_like(X, np.nan)

    def blk(b):
        u = units[b]
        w, nr, off = int(u["w"]), int(u["nrow"]), int(u["off"])
        return arena[off:off + nr * w].reshape(nr, w), rlist[int(u["idx_off"]):int(u["idx_off"]) + nr], w

    for i, tl in enumerate(tiles):                     # launch 1: every (block column, strip) tile stores
        b, ti = int(tl["unit"]), int(tl["ti"])
        B, idx, w = blk(b)
        r0 = w + ti * SR
        r1 = min(r0 + SR, B.shape[0])
        if transpose:
            o = int(t["bslot"][i])
            scratch[o:o + w] = B[r0:r1].T @ X[idx[r0:r1]]
        else:
            o = int(t["fslot"][b]) + r0 - w
            scratch[o:o + r1 - r0] = B[r0:r1] @ X[idx[:w]]
    low = {}
    for b in range(len(units)):                        # launch 2: the diagonal tile, then the stored products
        B, idx, w = blk(b)
        if w not in low:
            low[w] = np.tril(np.ones((w, w), dtype=bool))
        D = np.where(low[w], B[:w], 0.0)
        if transpose:
            y = D.T @ X[idx[:w]]
            ns = (B.shape[0] - w + SR - 1) // SR
            for s in range(ns):                        # ascending strip
                o = int(t["bfirst"][b]) + s * w
                y = y + scratch[o:o + w]
        else:
            y = D @ X[idx[:w]]
            for j, p in enumerate(idx[:w]):
                for k in range(int(t["gptr"][p]), int(t["gptr"][p + 1])):   # table order
                    y[j] = y[j] + scratch[int(t["gsrc"][k])]
        Y[idx[:w]] = y
    return Y


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on uint32 arrays (counter words c0..c3, key words k0, k1), ten rounds."""
    M0, M1, W0, W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), 0x9E3779B9, 0xBB67AE85
    c = [np.asarray(v, dtype=np.uint32) for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(k0), int(k1)
    lo32 = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0 = M0 * c[0].astype(np.uint64)
        p1 = M1 * c[2].astype(np.uint64)
        h0, l0 = (p0 >> np.uint64(32)).astype(np.uint32), (p0 & lo32).astype(np.uint32)
        h1, l1 = (p1 >> np.uint64(32)).astype(np.uint32), (p1 & lo32).astype(np.uint32)
        c = [h1 ^ c[1] ^ np.uint32(k0), l1, h0 ^ c[3] ^ np.uint32(k1), l0]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def white_noise_reference(n, nsamp, seed, first_sample=0):
    """(n, nsamp) standard normals in pivot order: the definition in include/spllt_hip.h, in numpy"""
    p = np.arange(n, dtype=np.uint32)[:, None]
    s = (np.arange(nsamp, dtype=np.uint64) + np.uint64(first_sample))[None, :]
    w = philox4x32_10(p, np.uint32(0), (s & np.uint64(0xFFFFFFFF)).astype(np.uint32),
                      (s >> np.uint64(32)).astype(np.uint32), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    a = ((w[1].astype(np.uint64) << np.uint64(32)) | w[0].astype(np.uint64)) >> np.uint64(11)
    b = ((w[3].astype(np.uint64) << np.uint64(32)) | w[2].astype(np.uint64)) >> np.uint64(11)
    u1 = (a + np.uint64(1)).astype(np.float64) * 2.0 ** -53
    u2 = b.astype(np.float64) * 2.0 ** -53
    return np.sqrt(-2.0 * np.log(u1)) * np.cos((2.0 * np.pi) * u2)
