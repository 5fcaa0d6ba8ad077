"""Loader of the host emulation of the distortion accumulator (tests/cpu_emul/distortion_emul.cpp: the per-entry functions of
csrc/hpf_distortion.hpp, what k_distortion_add runs per thread) and the scenario sets the host tests share.  Test infrastructure only."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpu_emul", "distortion_emul.cpp")
LIB = os.path.join(HERE, "cpu_emul", "libhpf_distortion_emul.so")
HDR = os.path.join(os.path.dirname(HERE), "harmonic-power-flow_amd", "csrc", "hpf_distortion.hpp")
GOLD = os.path.join(HERE, "golden")

SHAPES = (lambda n, Hn, B: (3,),) + (lambda n, Hn, B: (Hn, n),) * 5 + (lambda n, Hn, B: (n,),) * 5 + (lambda n, Hn, B: (n, B + 1),)
NAMES = ("counts", "x_max", "x_arg", "x_sum", "x_sumsq", "x_over", "thd_max", "thd_arg", "thd_sum", "thd_sumsq", "thd_over", "thd_hist")
DTYPES = (np.int64, np.float64, np.int32, np.float64, np.float64, np.uint32, np.float64, np.int32, np.float64, np.float64, np.uint32, np.uint32)


def load():
    if (not os.path.exists(LIB)) or os.path.getmtime(LIB) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.dirname(HDR), SRC, "-o", LIB])
    return C.CDLL(LIB)


def empty(n, Hn, bins):
    out = {name: np.zeros(sh(n, Hn, bins), dtype=dt) for name, dt, sh in zip(NAMES, DTYPES, SHAPES)}
    out["x_arg"][:] = -1
    out["thd_arg"][:] = -1
    return out


def accumulate(Vm, ids, flags, n, Hn, limit=None, thd_limit=np.inf, hist_max=1.0, bins=64, queue=False, into=None):
    """The emulated accumulator over the scenarios Vm [S][Hn*n] (stacked order) -> dict of the ABI's arrays; `into`: keep accumulating."""
    lib = load()
    out = empty(n, Hn, bins) if into is None else into
    Vm = np.ascontiguousarray(Vm, dtype=np.float64)
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    flags = np.ascontiguousarray(flags, dtype=np.int32)
    lim = np.ascontiguousarray(np.full(Hn, np.inf) if limit is None else limit, dtype=np.float64)
    lib.emul_distortion(C.c_int(n), C.c_int(Hn), C.c_int(len(ids)), Vm.ctypes.data_as(C.c_void_p), ids.ctypes.data_as(C.c_void_p),
                        flags.ctypes.data_as(C.c_void_p), C.c_int(int(queue)), lim.ctypes.data_as(C.c_void_p), C.c_double(thd_limit),
                        C.c_double(hist_max), C.c_int(bins), *[out[name].ctypes.data_as(C.c_void_p) for name in NAMES])
    return out


def midpoint_limit(v):
    """Midpoint between the two adjacent sorted values of v around its median: about half the samples lie above, none on it."""
    s = np.sort(np.asarray(v).ravel())
    k = len(s) // 2
    return 0.5 * (s[k - 1] + s[k])


def golden_case(name, S=20):
    """The final voltages of a golden network replicated into S scenarios with small deterministic perturbations; scenario 7 did not converge."""
    g = np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=True)
    V = g["V_final"][:, 0].astype(np.float64)
    n = int(g["n"])
    Hn = len(V) // n
    k = np.arange(len(V))
    Vm = np.stack([V * (1.0 + 0.03 * np.sin(0.7 * s + 0.37 * k) + 0.002 * s) for s in range(S)])
    ids = np.arange(S)
    flags = np.ones(S, dtype=np.int32)
    flags[7] = 2
    return Vm, ids, flags, n, Hn


def settings_for(Vm, flags, n, Hn, bins=64):
    """limits at midpoints of the NumPy samples, hist_max = 1.25 x the largest THD"""
    import distortion_ref as ref
    x, thd = ref.samples(Vm, n, Hn)
    ok = ((np.asarray(flags) & 1) != 0) & np.isfinite(thd).all(axis=1)
    limit = np.array([midpoint_limit(x[ok, q, :]) for q in range(Hn)])
    return dict(limit=limit, thd_limit=float(midpoint_limit(thd[ok])), hist_max=float(1.25 * thd[ok].max()), bins=bins)
