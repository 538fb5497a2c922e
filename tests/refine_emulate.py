"""numpy restatement of the refined solves (spllt_hip_solve_refined): the same loop,
stopping rule, definition of `iterations`, confirmation step and best-iterate rule, for ONE vector and any
preconditioner callback apply_M.

    x = M^-1 b ; r = b - A x ; e = |r|_2 / (|b|_2 + max|a_ij| |x|_2)
    method 0 (refinement):  while e > tol and it < max_iter:  x += M^-1 r ; r = b - A x ; it += 1
    method 1 (PCG):         z = M^-1 r ; p = z ; the standard recurrences; a vector that the recurrence
                            residual declares converged is confirmed with a true residual and goes on from
                            it, with a fresh direction, if the confirmation fails

iterations = applications of M^-1 after the first.  The error returned is always that of a true residual,
the x returned the iterate with the smallest such error."""
import numpy as np


def apply_tables(rowptr, col, src, val, xp):
    """y_p = sum_k val[src[k]] * x[col[k]] for vectors in pivot order (xp: n or n x nvec)"""
    prod = val[src][:, None] * xp.reshape(len(rowptr) - 1, -1)[col]
    nz = np.flatnonzero(np.diff(rowptr) > 0)
    y = np.zeros((len(rowptr) - 1, prod.shape[1]))
    y[nz] = np.add.reduceat(prod, rowptr[:-1][nz], axis=0)
    return y.reshape(xp.shape)


def backward_error(r, b, x, amax):
    rr = float(r @ r)
    if rr == 0.0:
        return 0.0
    return float(np.sqrt(rr) / (np.linalg.norm(b) + amax * np.linalg.norm(x)))


def refine(A, b, apply_M, method, tol, max_iter):
    """Returns (x, iterations, error, converged).  A: anything with A @ v and abs(A).max(); method 0 / 1."""
    amax = float(abs(A).max())
    b = np.asarray(b, dtype=np.float64)
    x = apply_M(b.copy())
    r = b - A @ x
    e = backward_error(r, b, x, amax)
    best_x, best_e = x.copy(), e

    def keep(xc, ec):
        nonlocal best_x, best_e
        if ec < best_e:
            best_x, best_e = xc.copy(), ec

    it = 0
    if not np.isfinite(e):
        return best_x, it, best_e, False
    if e <= tol:
        return best_x, it, best_e, True
    if method == 0:
        while it < max_iter:
            it += 1
            x = x + apply_M(r.copy())
            r = b - A @ x
            e = backward_error(r, b, x, amax)
            keep(x, e)
            if not np.isfinite(e):
                return best_x, it, best_e, False
            if e <= tol:
                return best_x, it, best_e, True
        return best_x, it, best_e, False
    restart, rz, p = True, 0.0, None
    while it < max_iter:
        it += 1
        z = apply_M(r.copy())
        rz_new = float(r @ z)
        beta = 0.0 if restart else rz_new / rz
        if not (np.isfinite(beta) and np.isfinite(rz_new)):
            return best_x, it, best_e, False
        p = z if beta == 0.0 else z + beta * p
        rz, restart = rz_new, False
        q = A @ p
        alpha = rz / float(p @ q)
        if not np.isfinite(alpha):
            return best_x, it, best_e, False
        x = x + alpha * p
        r = r - alpha * q
        e_rec = backward_error(r, b, x, amax)
        if not np.isfinite(e_rec):
            return best_x, it, best_e, False
        if e_rec <= tol:              # declared: confirm with a true residual
            r = b - A @ x
            e = backward_error(r, b, x, amax)
            keep(x, e)
            if not np.isfinite(e):
                return best_x, it, best_e, False
            if e <= tol:
                return best_x, it, best_e, True
            restart = True
    r = b - A @ x                     # out of iterations: report a true residual (which may pass)
    e = backward_error(r, b, x, amax)
    keep(x, e)
    return best_x, it, best_e, bool(np.isfinite(e) and e <= tol)
