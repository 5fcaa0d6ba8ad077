"""Loader of the host emulation of the voltage waveforms and the waveform statistics (tests/cpu_emul/waveform_emul.cpp: the functions of
csrc/hpf_waveform.hpp in the kernels' order).  Test infrastructure only."""
import ctypes as C
import os
import subprocess

import numpy as np

from distortion_emul import list_args

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpu_emul", "waveform_emul.cpp")
LIB = os.path.join(HERE, "cpu_emul", "libhpf_waveform_emul.so")
CSRC = os.path.join(os.path.dirname(HERE), "harmonic-power-flow_amd", "csrc")
HDRS = [os.path.join(CSRC, f) for f in ("hpf_waveform.hpp", "hpf_distortion.hpp", "hpf_accum.hpp", "hpf_assembly.hpp")]

NAMES = ("counts", "peak_max", "peak_arg", "peak_sum", "peak_sumsq", "peak_over", "crest_max", "crest_arg", "crest_sum", "crest_sumsq",
         "crest_over")
DTYPES = (np.int64, np.float64, np.int32, np.float64, np.float64, np.uint32, np.float64, np.int32, np.float64, np.float64, np.uint32)
_F = ("peak_max", "peak_sum", "peak_sumsq", "crest_max", "crest_sum", "crest_sumsq")
_A = ("peak_arg", "crest_arg")
_O = ("peak_over", "crest_over")


def load():
    if (not os.path.exists(LIB)) or os.path.getmtime(LIB) < max(os.path.getmtime(p) for p in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", CSRC, SRC, "-o", LIB])
    lib = C.CDLL(LIB)
    lib.emul_wave_rms.restype = C.c_double
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def table(T):
    """(ct, st) [T] of wave_table; None for a T the header refuses"""
    ct, st = np.empty(max(T, 1)), np.empty(max(T, 1))
    return (ct, st) if load().emul_wave_table(C.c_int(T), _p(ct), _p(st)) == 0 else None


def waveform(U, orders, T, ct, st, sel=()):
    """The emulated k_wave_peaks: U [S][n][Hn] complex -> dict in the ABI's shapes (v [S][len(sel)][T])"""
    lib = load()
    U = np.ascontiguousarray(U, dtype=np.complex128)
    S, n, Hn = U.shape
    orders = np.ascontiguousarray(orders, dtype=np.int32)
    sel = np.ascontiguousarray(sel, dtype=np.int32)
    ct, st = np.ascontiguousarray(ct, dtype=np.float64), np.ascontiguousarray(st, dtype=np.float64)
    assert len(orders) == Hn and len(ct) == len(st) == T
    out = {"v": np.zeros((S, len(sel), T)), "peak": np.zeros((S, n)), "kpeak": np.zeros((S, n), dtype=np.int32), "crest": np.zeros((S, n)),
           "slack": np.zeros((S, n))}
    lib.emul_waveform(C.c_int(n), C.c_int(Hn), C.c_int(S), C.c_int(T), _p(orders), _p(U), _p(ct), _p(st), C.c_int(len(sel)), _p(sel),
                      *[_p(out[k]) for k in ("v", "peak", "kpeak", "crest", "slack")])
    return out


def rms(U_bus):
    U_bus = np.ascontiguousarray(U_bus, dtype=np.complex128)
    return float(load().emul_wave_rms(C.c_int(len(U_bus)), _p(U_bus)))


def empty(n):
    out = {name: np.zeros((3,) if name == "counts" else (n,), dtype=dt) for name, dt in zip(NAMES, DTYPES)}
    for a in _A:
        out[a][:] = -1
    return out


def accumulate(peak, crest, ids, flags, thd_max, peak_limit=None, crest_limit=np.inf, queue=False, into=None, slots=None, gids=None, id_base=0):
    """The emulated k_wave_add over the storages peak, crest [S][n] and the list of distortion_emul.list_args with records (flags, thd_max) -> dict
    of the ABI's arrays; `into`: keep going"""
    lib = load()
    peak, crest = np.ascontiguousarray(peak, dtype=np.float64), np.ascontiguousarray(crest, dtype=np.float64)
    n = peak.shape[1]
    out = empty(n) if into is None else into
    f = np.stack([out[k] for k in _F])
    arg = np.stack([out[k] for k in _A])
    over = np.stack([out[k] for k in _O])
    head, recs = list_args(ids, flags, thd_max, slots, gids, id_base)
    lim = np.ascontiguousarray(np.full(n, np.inf) if peak_limit is None else peak_limit, dtype=np.float64)
    lib.emul_wave_add(C.c_int(n), *head, _p(peak), _p(crest), *recs, C.c_int(int(queue)), _p(lim), C.c_double(float(crest_limit)),
                      _p(out["counts"]), _p(f), _p(arg), _p(over))
    for group, names in ((f, _F), (arg, _A), (over, _O)):
        for i, k in enumerate(names):
            out[k] = group[i].copy()
    return out
