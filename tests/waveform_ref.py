"""NumPy restatement of the voltage waveforms and the waveform statistics (include/hpf.h, hpf_waveform*): the yardstick of the waveform tests --
never the library's own output.  Test infrastructure only.

Voltages come in the ABI's stacked order (k = q*n + i) or as U [S][n][Hn] (the device layout).  All arithmetic is real and unfused (NumPy rounds
every real product, difference and sum on its own), every sum over q runs sequentially over ascending q from 0.0, the table positions are integers
(j = (order k) & (T - 1)), so with the same table the header's functions give the same doubles."""
import ctypes as C

import numpy as np

QUANT = ("peak", "crest")
EXACT = ("counts", "peak_max", "peak_arg", "peak_over", "crest_max", "crest_arg", "crest_over")
SUMS = ("peak_sum", "peak_sumsq", "crest_sum", "crest_sumsq")
SQRT2 = 1.4142135623730951


def lib_table(T):
    """(ct, st) [T] through hpf_waveform_table: the library's own table (host libm; no device)"""
    from harmonic_power_flow_amd import _lib
    ct, st = np.empty(T), np.empty(T)
    rc = _lib.load().hpf_waveform_table(int(T), ct.ctypes.data_as(_lib.c_dbl_p), st.ctypes.data_as(_lib.c_dbl_p))
    assert rc == 0, rc
    return ct, st


def own_table(T):
    """the same table from numpy's cos / sin (may differ from libm's in the last bit: for the bound tests), quadrant points exact"""
    w = 6.283185307179586 / float(T)
    j = np.arange(T, dtype=np.float64)
    ct, st = np.cos(j * w), np.sin(j * w)
    for q, (c, s) in zip((0, T // 4, T // 2, 3 * T // 4), ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))):
        ct[q], st[q] = c, s
    return ct, st


def rect(Vm, Va, n, Hn):
    """U [S][n][Hn] = Vm exp(j Va) from the stacked order, componentwise products"""
    Vm = np.asarray(Vm, dtype=np.float64).reshape(-1, Hn, n).transpose(0, 2, 1)
    Va = np.asarray(Va, dtype=np.float64).reshape(-1, Hn, n).transpose(0, 2, 1)
    return np.ascontiguousarray(Vm * np.cos(Va) + 1j * (Vm * np.sin(Va)))


def samples(U, orders, T, ct, st):
    """U [..., Hn] -> v [..., T]"""
    U = np.asarray(U, dtype=np.complex128)
    k = np.arange(T, dtype=np.int64)
    v = np.zeros(U.shape[:-1] + (T,))
    for q, h in enumerate(orders):
        j = (int(h) * k) & (T - 1)
        v = v + (U.real[..., q, None] * ct[j] - U.imag[..., q, None] * st[j])
    return v


def sumsq(U):
    U = np.asarray(U, dtype=np.complex128)
    s = np.zeros(U.shape[:-1])
    for q in range(U.shape[-1]):
        s = s + (U.real[..., q] * U.real[..., q] + U.imag[..., q] * U.imag[..., q])
    return s


def rms(U):
    return np.sqrt(0.5 * sumsq(U))


def waveform(U, orders, T, ct, st):
    """-> dict of v [..., T], peak, kpeak, crest, slack, rms, sum_abs (= sum_q |U_q|) [...]"""
    U = np.asarray(U, dtype=np.complex128)
    v = samples(U, orders, T, ct, st)
    a = np.abs(v)
    kpeak = np.argmax(a, axis=-1)                                 # (the first maximum: the smallest k; a NaN first of all)
    peak = np.take_along_axis(a, kpeak[..., None], axis=-1)[..., 0]
    s = sumsq(U)
    w = 3.141592653589793 / float(T)
    acc, sum_abs = np.zeros(U.shape[:-1]), np.zeros(U.shape[:-1])
    for q, h in enumerate(orders):
        mag = np.sqrt(U.real[..., q] * U.real[..., q] + U.imag[..., q] * U.imag[..., q])
        acc = acc + (float(h) * float(h)) * mag
        sum_abs = sum_abs + mag
    with np.errstate(all="ignore"):
        crest = SQRT2 * (peak / np.sqrt(s))
    return {"v": v, "peak": peak, "kpeak": kpeak.astype(np.int32), "crest": crest, "slack": (0.5 * (w * w)) * acc, "rms": np.sqrt(0.5 * s),
            "sum_abs": sum_abs}


def _five(x, ids, limit):
    shape = x.shape[1:]
    if x.shape[0] == 0:
        return np.zeros(shape), np.full(shape, -1, np.int32), np.zeros(shape), np.zeros(shape), np.zeros(shape, np.uint32)
    mx = x.max(axis=0)
    arg = np.where(x == mx, ids[:, None], np.iinfo(np.int64).max).min(axis=0).astype(np.int32)
    return mx, arg, x.sum(axis=0), (x * x).sum(axis=0), (x > limit).sum(axis=0).astype(np.uint32)


def accumulate(peak, crest, ids, flags, thd_ok, peak_limit=None, crest_limit=np.inf, deferred=None):
    """The statistics of the scenarios with peak, crest [S][n]: a scenario is added when flags bit 0 is set and thd_ok (a finite THD at every bus);
    the ones listed in `deferred` count as deferred and are left out, every other one as skipped."""
    ids = np.asarray(ids, dtype=np.int64)
    flags = np.asarray(flags, dtype=np.int64)
    S, n = peak.shape
    dfr = np.zeros(S, bool) if deferred is None else np.asarray(deferred, bool)
    ok = ((flags & 1) != 0) & np.asarray(thd_ok, bool) & ~dfr
    lim = np.full(n, np.inf) if peak_limit is None else np.asarray(peak_limit, dtype=np.float64)
    out = {"counts": np.array([ok.sum(), (~ok & ~dfr).sum(), dfr.sum()], dtype=np.int64), "added_mask": ok}
    for pre, x, l in (("peak", peak, lim), ("crest", crest, crest_limit)):
        mx, arg, s, s2, over = _five(x[ok], ids[ok], l)
        out.update({pre + "_max": mx, pre + "_arg": arg, pre + "_sum": s, pre + "_sumsq": s2, pre + "_over": over})
    return out
