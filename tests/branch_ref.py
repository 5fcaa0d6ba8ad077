"""NumPy restatement of the branch flows and the branch statistics (include/hpf.h, hpf_branch_*): the yardstick of the branch tests -- never the
library's own output.  Test infrastructure only.

Input: the shared admittance pattern (rowptr, col, Yval [Hn][nnz]) and voltages in the ABI's stacked order (k = q*n + i).  A branch is one stored
pair (i, j), i < j, numbered in CSR order; y = -Y at its position.  All arithmetic is real and unfused (NumPy rounds every real product and sum on
its own), every sum over q runs sequentially over ascending q, so on the host the header's functions give the same doubles."""
import numpy as np

TILE = 32
QUANT = ("irms", "loss", "lossh")
EXACT = ("counts", "irms_max", "irms_arg", "irms_over", "loss_max", "loss_arg", "lossh_max", "lossh_arg")
SUMS = ("irms_sum", "irms_sumsq", "loss_sum", "loss_sumsq", "lossh_sum", "lossh_sumsq")


def branches(rowptr, col):
    """-> from, to, ypos [nb]: stored pairs (i, j), i < j, row-major, columns ascending"""
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    ypos = np.nonzero(np.asarray(col) > rows)[0]
    return rows[ypos].astype(np.int32), np.asarray(col)[ypos].astype(np.int32), ypos.astype(np.int32)


def series(Yval, ypos):
    """y [Hn][nb] = -Y[q][pos(i, j)]"""
    return -np.asarray(Yval)[:, ypos]


def rect(Vm, Va, n, Hn):
    """U [S][Hn][n] = Vm exp(j Va), componentwise products (HG:403)"""
    Vm = np.asarray(Vm, dtype=np.float64).reshape(-1, Hn, n)
    Va = np.asarray(Va, dtype=np.float64).reshape(-1, Hn, n)
    return Vm * np.cos(Va) + 1j * (Vm * np.sin(Va))


def loss_h_of(loss_q):
    """loss_q [S][Hn][nb] -> [S][Hn]: tiles of 32 consecutive branches, ascending e inside a tile from 0.0, then the tile sums ascending from 0.0"""
    S, Hn, nb = loss_q.shape
    out = np.zeros((S, Hn))
    for t0 in range(0, nb, TILE):
        a = np.zeros((S, Hn))
        for e in range(t0, min(t0 + TILE, nb)):
            a = a + loss_q[:, :, e]
        out = out + a
    return out


def flows(fr, to, y, U):
    """fr, to [nb]; y [Hn][nb]; U [S][Hn][n] -> dict of I [S][Hn][nb] complex, i2, loss_q [S][Hn][nb], irms, thd_i, loss, loss_harm [S][nb],
    loss_h [S][Hn], and d = U_i - U_j"""
    U = np.asarray(U)
    dr = U.real[:, :, fr] - U.real[:, :, to]
    di = U.imag[:, :, fr] - U.imag[:, :, to]
    yr, yi = y.real[None], y.imag[None]
    Ir = yr * dr - yi * di
    Ii = yr * di + yi * dr
    i2 = Ir * Ir + Ii * Ii
    loss_q = yr * (dr * dr + di * di)
    Hn = U.shape[1]
    i2_all, i2_harm = np.zeros_like(i2[:, 0]), np.zeros_like(i2[:, 0])
    l_all, l_harm = np.zeros_like(i2[:, 0]), np.zeros_like(i2[:, 0])
    for q in range(Hn):
        i2_all = i2_all + i2[:, q]
        l_all = l_all + loss_q[:, q]
        if q >= 1:
            i2_harm = i2_harm + i2[:, q]
            l_harm = l_harm + loss_q[:, q]
    with np.errstate(all="ignore"):
        thd_i = np.sqrt(i2_harm) / np.sqrt(i2[:, 0])
    return {"I": Ir + 1j * Ii, "i2": i2, "loss_q": loss_q, "irms": np.sqrt(i2_all), "thd_i": thd_i, "loss": l_all, "loss_harm": l_harm,
            "loss_h": loss_h_of(loss_q), "d": dr + 1j * di}


def _four(x, ids, limit=None):
    shape = x.shape[1:]
    if x.shape[0] == 0:
        return np.zeros(shape), np.full(shape, -1, np.int32), np.zeros(shape), np.zeros(shape), np.zeros(shape, np.uint32)
    mx = x.max(axis=0)
    arg = np.where(x == mx, ids[:, None], np.iinfo(np.int64).max).min(axis=0).astype(np.int32)
    over = np.zeros(shape, np.uint32) if limit is None else (x > limit).sum(axis=0).astype(np.uint32)
    return mx, arg, x.sum(axis=0), (x * x).sum(axis=0), over


def accumulate(fl, ids, flags, thd_ok, rating=None, deferred=None):
    """The statistics of the scenarios whose flows are fl (dict of flows()): a scenario is added when flags bit 0 is set and thd_ok (a finite THD
    at every bus); the ones listed in `deferred` count as deferred and are left out, every other one as skipped."""
    ids = np.asarray(ids, dtype=np.int64)
    flags = np.asarray(flags, dtype=np.int64)
    S = len(ids)
    dfr = np.zeros(S, bool) if deferred is None else np.asarray(deferred, bool)
    ok = ((flags & 1) != 0) & np.asarray(thd_ok, bool) & ~dfr
    nb = fl["irms"].shape[1]
    lim = np.full(nb, np.inf) if rating is None else np.asarray(rating, dtype=np.float64)
    out = {"counts": np.array([ok.sum(), (~ok & ~dfr).sum(), dfr.sum()], dtype=np.int64)}
    for pre, key in zip(QUANT, ("irms", "loss", "loss_harm")):
        mx, arg, s, s2, over = _four(fl[key][ok], ids[ok], lim if pre == "irms" else None)
        out.update({pre + "_max": mx, pre + "_arg": arg, pre + "_sum": s, pre + "_sumsq": s2})
        if pre == "irms":
            out["irms_over"] = over
        out[pre] = fl[key][ok]
    out["added_mask"] = ok
    return out


def thd_ok(Vm, n, Hn):
    """every bus has a finite THD_F (the rule of the accumulators: hpf_stat.thd_max finite)"""
    V = np.asarray(Vm, dtype=np.float64).reshape(-1, Hn, n)
    with np.errstate(all="ignore"):
        hs = np.zeros_like(V[:, 0])
        for q in range(1, Hn):
            hs = hs + V[:, q] * V[:, q]
        return np.isfinite(np.sqrt(hs) / np.abs(V[:, 0])).all(axis=1)


def sum_bound(samples_abs_sum, added):
    """recursive sum of `added` non-negative terms: |computed - exact| <= added * 2^-52 * sum (either order, either side)"""
    return added * 2.0 ** -52 * samples_abs_sum
