"""References of the impedance scan tests: the dense NumPy restatement (Y(h) from admittance.line_model, numpy.linalg.inv) and the tree
recurrence of csrc/hpf_zscan.hpp in numpy.clongdouble (radial networks).  Test infrastructure only."""
import numpy as np

EPS = 2.0 ** -52


def dense_Y(model, h, yx=None, dtype=np.complex128):
    """Y(h) [n][n] of one real order h; yx [n]: the y_extra row of the point"""
    n = int(model["n"])
    Y = np.zeros((n, n), dtype=dtype)
    R, X = np.asarray(model["R"], dtype=dtype), np.asarray(model["X"], dtype=dtype)
    y = 1 / (R + 1j * X * h) if len(R) else R
    for e, (a, b) in enumerate(zip(model["fr"], model["to"])):
        Y[a, b] -= y[e]
        Y[b, a] -= y[e]
        Y[a, a] += y[e]
        Y[b, b] += y[e]
    d = np.asarray(model["gsh"], dtype=dtype) + 1j * h * np.asarray(model["bsh"], dtype=dtype)
    xsh = np.asarray(model["xsh"], dtype=float)
    if h != 1:
        nz = xsh != 0
        d[nz] += 1 / (1j * xsh[nz].astype(dtype) * h)
    if yx is not None:
        d = d + np.asarray(yx, dtype=dtype)
    Y[np.arange(n), np.arange(n)] += d
    return Y


def dense_scan(model, h, y_extra=None):
    """-> Zfull [F][n][n] = Y(h)^-1, kappa [F] = the 2-norm condition number of Y(h), Y [F][n][n]"""
    Ys = np.stack([dense_Y(model, x, None if y_extra is None else y_extra[f]) for f, x in enumerate(h)])
    return np.linalg.inv(Ys), np.linalg.cond(Ys, 2), Ys


def bfs_tree(model):
    """BFS spanning tree from bus 0, neighbours in ascending branch index -> parent, parent branch, BFS order (radial: every branch is in it)"""
    n = int(model["n"])
    adj = [[] for _ in range(n)]
    for e, (a, b) in enumerate(zip(model["fr"], model["to"])):
        adj[a].append((e, int(b)))
        adj[b].append((e, int(a)))
    parent, pbranch, order = [-2] * n, [-1] * n, [0]
    parent[0] = -1
    for i in order:
        for e, j in adj[i]:
            if parent[j] == -2:
                parent[j], pbranch[j] = i, e
                order.append(j)
    assert len(order) == n
    return parent, pbranch, order


def tree_scan_longdouble(model, h, y_extra=None):
    """The up / down recurrence in clongdouble for a RADIAL model -> Z [F][n] clongdouble"""
    n = int(model["n"])
    assert int(model["nb"]) == n - 1
    parent, pbranch, order = bfs_tree(model)
    L = np.clongdouble
    hh = np.asarray(h, dtype=np.longdouble)
    R, X = np.asarray(model["R"], dtype=np.longdouble), np.asarray(model["X"], dtype=np.longdouble)
    y = [1 / (R[e] + L(1j) * X[e] * hh) for e in range(n - 1)]                     # [nb][F]
    xsh = np.asarray(model["xsh"], dtype=np.longdouble)
    S = []
    for i in range(n):
        d = np.asarray(model["gsh"], dtype=np.longdouble)[i] + L(1j) * hh * np.asarray(model["bsh"], dtype=np.longdouble)[i]
        if xsh[i] != 0:
            d = d + np.where(hh != 1, 1 / (L(1j) * xsh[i] * hh), 0)
        if y_extra is not None:
            d = d + np.asarray(y_extra)[:, i].astype(L)
        S.append(d)
    for i in range(1, n):
        S[i] = S[i] + y[pbranch[i]]
        S[parent[i]] = S[parent[i]] + y[pbranch[i]]
    w, t, Z = [None] * n, [None] * n, [None] * n
    for i in reversed(order):
        w[i] = 1 / S[i]
        if parent[i] >= 0:
            t[i] = y[pbranch[i]] * w[i]
            S[parent[i]] = S[parent[i]] - y[pbranch[i]] * t[i]
    for i in order:
        Z[i] = w[i] if parent[i] < 0 else w[i] + t[i] * (t[i] * Z[parent[i]])
    return np.stack(Z, axis=1)
