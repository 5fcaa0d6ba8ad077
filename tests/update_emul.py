"""Loader of the host emulation of the state update (tests/cpu_emul/update_emul.cpp: the functions of csrc/hpf_update.hpp).  Test
infrastructure only."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpu_emul", "update_emul.cpp")
LIB = os.path.join(HERE, "cpu_emul", "libhpf_update_emul.so")
CSRC = os.path.join(os.path.dirname(HERE), "harmonic-power-flow_amd", "csrc")
HDRS = [os.path.join(CSRC, f) for f in ("hpf_update.hpp", "hpf_assembly.hpp")]


def load():
    if (not os.path.exists(LIB)) or os.path.getmtime(LIB) < max(os.path.getmtime(p) for p in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", CSRC, SRC, "-o", LIB])
    return C.CDLL(LIB)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def update(k, c, vm, va, u, e, dth, dv, rectangular=True):
    """The emulated k_update_rect (rectangular=False: k_update<false>) over a list of entries -> dict vm, va (the new state), target (U', complex;
    NaN where the entry takes the polar update), U, E (what the kernel stores)"""
    lib = load()
    k = np.ascontiguousarray(k, dtype=np.int32)
    vm, va, dth, dv = (np.ascontiguousarray(a, dtype=np.float64) for a in (vm, va, dth, dv))
    u, e = (np.ascontiguousarray(a, dtype=np.complex128) for a in (u, e))
    cnt = len(k)
    out = {"vm": np.empty(cnt), "va": np.empty(cnt), "target": np.empty(cnt, dtype=np.complex128), "U": np.empty(cnt, dtype=np.complex128),
           "E": np.empty(cnt, dtype=np.complex128)}
    lib.emul_update(C.c_int(cnt), C.c_int(c), C.c_int(int(rectangular)), _p(k), _p(vm), _p(va), _p(u), _p(e), _p(dth), _p(dv),
                    *[_p(out[n]) for n in ("vm", "va", "target", "U", "E")])
    return out
