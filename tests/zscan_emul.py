"""Loader of the host emulation of the impedance scan (tests/cpu_emul/zscan_emul.cpp: the functions of csrc/hpf_zscan.hpp in the kernels'
order) and the networks the scan tests share.  Test infrastructure only."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpu_emul", "zscan_emul.cpp")
LIB = os.path.join(HERE, "cpu_emul", "libhpf_zscan_emul.so")
CSRC = os.path.join(os.path.dirname(HERE), "harmonic-power-flow_amd", "csrc")
HDRS = [os.path.join(CSRC, f) for f in ("hpf_zscan.hpp", "hpf_penetration.hpp", "hpf_waveform.hpp", "hpf_distortion.hpp", "hpf_assembly.hpp")] + \
    [os.path.join(HERE, "cpu_emul", "zfactor_emul.hpp")]     # (the factor and the solve the three emulations share)
INPUTS = os.path.join(HERE, "golden", "inputs")


def load():
    if (not os.path.exists(LIB)) or os.path.getmtime(LIB) < max(os.path.getmtime(p) for p in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", CSRC, SRC, "-o", LIB])
    return C.CDLL(LIB)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _net_args(model):
    a = [np.ascontiguousarray(model[k], dtype=np.int32 if k in ("fr", "to") else np.float64) for k in ("fr", "to", "R", "X", "gsh", "bsh", "xsh")]
    return a, [C.c_int(int(model["n"])), C.c_int(int(model["nb"]))] + [_p(x) for x in a]


def scan(model, h, y_extra=None, sel=(), chunk=0, full=True):
    """The emulated hpf_impedance_scan -> (code, Z or None, Zt, zpeak, fpeak), like api.impedance_scan_arrays"""
    lib = load()
    n, F = int(model["n"]), len(h)
    keep, args = _net_args(model)
    h = np.ascontiguousarray(h, dtype=np.float64)
    sel = np.ascontiguousarray(sel, dtype=np.int32)
    yx = None if y_extra is None else np.ascontiguousarray(y_extra, dtype=np.complex128)
    Z = np.empty((F, n), dtype=np.complex128) if full else None
    Zt = np.empty((F, len(sel), n), dtype=np.complex128)
    zpeak, fpeak = np.empty(n), np.empty(n, dtype=np.int32)
    rc = lib.emul_zscan(*args, C.c_int(F), _p(h), _p(yx), C.c_int(len(sel)), _p(sel), C.c_int(int(chunk)), _p(Z), _p(Zt), _p(zpeak), _p(fpeak))
    assert rc in (0, 3), rc
    return rc, Z, Zt, zpeak, fpeak


def plan(model):
    """The header's planner -> (parent, parent branch, depth, ties), or its error code"""
    lib = load()
    n = int(model["n"])
    keep, args = _net_args(model)
    out = [np.empty(n, dtype=np.int32) for _ in range(3)] + [np.empty(8, dtype=np.int32)]
    k = lib.emul_zscan_plan(*args[:4], *[_p(a) for a in out])
    return k if k < 0 else (out[0], out[1], out[2], out[3][:k].copy())


# ---- networks ---------------------------------------------------------------------------------------------------------------------------------
def raw_model(n, edges, R=None, X=None, xsh0=0.005):
    """A model from a bare edge list (0-based pairs): R, X default to a deterministic spread; bus 0 carries the bus shunt of the feeders"""
    e = sorted((min(a, b), max(a, b)) for a, b in edges)
    nb = len(e)
    k = np.arange(nb)
    xsh = np.zeros(n)
    xsh[0] = xsh0
    return dict(n=n, nb=nb, fr=np.array([a for a, _ in e], dtype=np.int32), to=np.array([b for _, b in e], dtype=np.int32),
                R=np.asarray(0.01 * (1 + (k * 7) % 5) if R is None else R, dtype=float),
                X=np.asarray(0.02 * (1 + (k * 3) % 4) if X is None else X, dtype=float), gsh=np.zeros(n), bsh=np.zeros(n), xsh=xsh)


def chain(n):
    return raw_model(n, [(i, i + 1) for i in range(n - 1)])


def star(n):
    return raw_model(n, [(0, i) for i in range(1, n)])


_CACHE = {}


def network(name):
    """"net1" / "net2" (the reference's files) or "synN" (synth.gen(N), seed 0) -> dict(buses, lines, model)"""
    if name not in _CACHE:
        import harmonic_power_flow_amd as hp
        from harmonic_power_flow_amd import admittance, synth
        if name.startswith("syn"):
            fb, fl = synth.gen(int(name[3:]), seed=0, outdir=tempfile.mkdtemp())
        else:
            fb, fl = os.path.join(INPUTS, name + "_buses.csv"), os.path.join(INPUTS, name + "_lines.csv")
        buses, lines, m, n, c = hp.init_network(fb, fl, settings=hp.Settings())
        _CACHE[name] = dict(buses=buses, lines=lines, model=admittance.line_model(buses, lines), files=(fb, fl))
    return _CACHE[name]


def capacitors(model, h, banks):
    """y_extra [F][n] of capacitor banks {0-based bus: b}: j h b"""
    yx = np.zeros((len(h), int(model["n"])), dtype=np.complex128)
    for i, b in banks.items():
        yx[:, i] += 1j * np.asarray(h) * b
    return yx
