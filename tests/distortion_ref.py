"""NumPy restatement of the distortion accumulator (include/hpf.h, hpf_distortion_*): the yardstick of the distortion tests -- never the
library's own output.  Test infrastructure only.

Input: raw signed magnitudes Vm [S][Hn*n] in the ABI's stacked order (k = q*n + i, what solve_scenarios(..., want_voltages=True) returns), the
scenario ids [S], the result flags [S] (hpf_stat.flags).  A scenario is added when flags bit 0 is set and every bus has a finite THD; every
other one counts as skipped (scenarios listed in `deferred` count as deferred instead and are left out)."""
import numpy as np

FIELDS_X = ("x_max", "x_arg", "x_sum", "x_sumsq", "x_over")
FIELDS_THD = ("thd_max", "thd_arg", "thd_sum", "thd_sumsq", "thd_over", "thd_hist")
EXACT = ("counts", "x_max", "x_arg", "x_over", "thd_max", "thd_arg", "thd_over", "thd_hist")
SUMS = ("x_sum", "x_sumsq", "thd_sum", "thd_sumsq")


def samples(Vm, n, Hn):
    """-> x [S][Hn][n] (|V_1| at q = 0, |V_h| / |V_1| above), thd [S][n]: sequential sum over ascending q, one sqrt, one division."""
    V = np.asarray(Vm, dtype=np.float64).reshape(-1, Hn, n)
    with np.errstate(all="ignore"):
        v0 = np.abs(V[:, 0, :])
        x = np.abs(V) / v0[:, None, :]
        x[:, 0, :] = v0
        hs = np.zeros_like(v0)
        for q in range(1, Hn):
            hs = hs + V[:, q, :] * V[:, q, :]
        thd = np.sqrt(hs) / v0
    return x, thd


def bins_of(thd, hist_max, bins):
    inv_w = float(bins) / float(hist_max)
    with np.errstate(all="ignore"):
        b = np.minimum((np.where(thd >= hist_max, 0.0, thd) * inv_w).astype(np.int64), bins)
    return np.where(thd >= hist_max, bins, b)


def _five(x, ids, limit):
    """x [A][...], ids [A], limit broadcastable to x[0] -> max, arg, sum, sumsq, over"""
    shape = x.shape[1:]
    if x.shape[0] == 0:
        return (np.zeros(shape), np.full(shape, -1, np.int32), np.zeros(shape), np.zeros(shape), np.zeros(shape, np.uint32))
    mx = x.max(axis=0)
    idb = ids.reshape((-1,) + (1,) * len(shape))
    arg = np.where(x == mx, idb, np.iinfo(np.int64).max).min(axis=0).astype(np.int32)
    return mx, arg, x.sum(axis=0), (x * x).sum(axis=0), (x > limit).sum(axis=0).astype(np.uint32)


def accumulate(Vm, ids, flags, n, Hn, limit=None, thd_limit=np.inf, hist_max=1.0, bins=64, deferred=None):
    ids = np.asarray(ids, dtype=np.int64)
    flags = np.asarray(flags, dtype=np.int64)
    x, thd = samples(Vm, n, Hn)
    S = x.shape[0]
    dfr = np.zeros(S, bool) if deferred is None else np.asarray(deferred, bool)
    ok = ((flags & 1) != 0) & np.isfinite(thd).all(axis=1) & ~dfr
    lim = np.full(Hn, np.inf) if limit is None else np.asarray(limit, dtype=np.float64)
    out = {"counts": np.array([ok.sum(), (~ok & ~dfr).sum(), dfr.sum()], dtype=np.int64)}
    out.update(zip(FIELDS_X, _five(x[ok], ids[ok], lim[:, None])))
    out.update(zip(FIELDS_THD[:5], _five(thd[ok], ids[ok], float(thd_limit))))
    hist = np.zeros((n, bins + 1), dtype=np.uint32)
    b = bins_of(thd[ok], hist_max, bins)
    for row in b:
        hist[np.arange(n), row] += 1
    out["thd_hist"] = hist
    out["x"], out["thd"], out["added_mask"] = x[ok], thd[ok], ok
    return out


def sum_bound(samples_abs_sum, added):
    """recursive sum of `added` non-negative terms: |computed - exact| <= added * 2^-52 * sum (either order, either side)"""
    return added * 2.0 ** -52 * samples_abs_sum
