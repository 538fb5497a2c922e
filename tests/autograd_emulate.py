"""Dense numpy emulator of the two adjoints of spllt_amd.torch_ops, with the convention of the library: val[k], the
k-th stored value of the CSC lower triangle at (row[k], col[k]) = (i, j), i >= j, stands for BOTH a_ij and a_ji.

    x = A^-1 B,  loss = sum(G * x):   lam = A^-1 G,   d loss / d B = lam,
                                      d loss / d val[k] = -sum_q (lam[i, q] x[j, q] + [i != j] lam[j, q] x[i, q])
    log det A:                        d / d val[k] = (2 - [i == j]) (A^-1)[i, j]

Everything is dense and in numpy: the mathematics pinned independently of the GPU.
"""
import numpy as np


def dense_from_values(n, row, col, val):
    """the symmetric matrix of the stored lower-triangle values (row, col 0-based)"""
    A = np.zeros((n, n), dtype=val.dtype)
    A[row, col] = val
    A[col, row] = val
    return A


def pattern_outer(row, col, U, V, alpha=1.0, dtype=np.float64):
    """alpha sum_q (U[i, q] V[j, q] + [i != j] U[j, q] V[i, q]) per entry; dtype: the precision of the sum"""
    U = np.asarray(U, dtype=dtype).reshape(len(U), -1)
    V = np.asarray(V, dtype=dtype).reshape(len(V), -1)
    s = (U[row] * V[col]).sum(axis=1, dtype=dtype)
    t = (U[col] * V[row]).sum(axis=1, dtype=dtype)
    return dtype(alpha) * (s + np.where(row != col, t, dtype(0)))


def pattern_outer_magnitude(row, col, U, V, alpha=1.0):
    """|alpha| sum_q (|u_i v_j| + [i != j] |u_j v_i|) in long double: what the rounding bound of the chain scales with"""
    return np.asarray(pattern_outer(row, col, np.abs(np.asarray(U, dtype=np.longdouble)),
                                    np.abs(np.asarray(V, dtype=np.longdouble)), abs(alpha), dtype=np.longdouble))


def solve_grads(n, row, col, val, B, G):
    """(x, d loss / d val, d loss / d B) for loss = sum(G * A^-1 B)"""
    A = dense_from_values(n, row, col, val)
    X = np.linalg.solve(A, B)
    lam = np.linalg.solve(A, G)
    return X, pattern_outer(row, col, lam, X, alpha=-1.0), lam


def logdet_grad(n, row, col, val):
    """(log det A, d log det A / d val)"""
    A = dense_from_values(n, row, col, val)
    sign, ld = np.linalg.slogdet(A)
    assert sign > 0
    Z = np.linalg.inv(A)
    return ld, np.where(row == col, 1.0, 2.0) * Z[row, col]
