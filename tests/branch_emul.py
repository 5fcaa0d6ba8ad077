"""Loader of the host emulation of the branch flows and the branch statistics (tests/cpu_emul/branch_emul.cpp: the functions of
csrc/hpf_branch.hpp in the kernels' order) and the networks / scenario sets the branch tests share.  Test infrastructure only."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import branch_ref as ref
from distortion_emul import list_args

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpu_emul", "branch_emul.cpp")
LIB = os.path.join(HERE, "cpu_emul", "libhpf_branch_emul.so")
CSRC = os.path.join(os.path.dirname(HERE), "harmonic-power-flow_amd", "csrc")
HDRS = [os.path.join(CSRC, f) for f in ("hpf_branch.hpp", "hpf_distortion.hpp", "hpf_accum.hpp", "hpf_assembly.hpp")]
GOLD = os.path.join(HERE, "golden")
INPUTS = os.path.join(GOLD, "inputs")

NAMES = ("counts", "irms_max", "irms_arg", "irms_sum", "irms_sumsq", "irms_over", "loss_max", "loss_arg", "loss_sum", "loss_sumsq",
         "lossh_max", "lossh_arg", "lossh_sum", "lossh_sumsq")
_F = ("irms_max", "irms_sum", "irms_sumsq", "loss_max", "loss_sum", "loss_sumsq", "lossh_max", "lossh_sum", "lossh_sumsq")
_A = ("irms_arg", "loss_arg", "lossh_arg")


def load():
    if (not os.path.exists(LIB)) or os.path.getmtime(LIB) < max(os.path.getmtime(p) for p in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", CSRC, SRC, "-o", LIB])
    return C.CDLL(LIB)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def table(n, rowptr, col):
    lib = load()
    rowptr = np.ascontiguousarray(rowptr, dtype=np.int32)
    col = np.ascontiguousarray(col, dtype=np.int32)
    out = [np.empty(len(col), dtype=np.int32) for _ in range(3)]
    nb = lib.emul_branch_table(C.c_int(n), _p(rowptr), _p(col), *[_p(a) for a in out])
    return tuple(a[:nb].copy() for a in out)


def _device_layout(fr, to, y, U):
    """y [Hn][nb] -> [nb][Hn]; U [S][Hn][n] -> [S][n][Hn]"""
    return (np.ascontiguousarray(fr, dtype=np.int32), np.ascontiguousarray(to, dtype=np.int32),
            np.ascontiguousarray(np.asarray(y, dtype=np.complex128).T), np.ascontiguousarray(np.asarray(U, dtype=np.complex128).transpose(0, 2, 1)))


def flows(fr, to, y, U):
    """The emulated k_branch_flows: fr, to [nb], y [Hn][nb], U [S][Hn][n] -> dict in the ABI's shapes"""
    lib = load()
    S, Hn, n = U.shape
    nb = len(fr)
    fr, to, yb, Ub = _device_layout(fr, to, y, U)
    out = {"I": np.zeros((S, Hn, nb), dtype=np.complex128), "irms": np.zeros((S, nb)), "thd_i": np.zeros((S, nb)), "loss": np.zeros((S, nb)),
           "loss_harm": np.zeros((S, nb)), "loss_h": np.zeros((S, Hn))}
    lib.emul_branch_flows(C.c_int(n), C.c_int(Hn), C.c_int(nb), C.c_int(S), _p(fr), _p(to), _p(yb), _p(Ub),
                          *[_p(out[k]) for k in ("I", "irms", "thd_i", "loss", "loss_harm", "loss_h")])
    return out


def empty(nb):
    out = {name: np.zeros((3,) if name == "counts" else (nb,), dtype=dt) for name, dt in zip(NAMES, (
        np.int64, np.float64, np.int32, np.float64, np.float64, np.uint32, np.float64, np.int32, np.float64, np.float64, np.float64, np.int32,
        np.float64, np.float64))}
    for a in _A:
        out[a][:] = -1
    return out


def accumulate(fr, to, y, U, ids, flags, thd_max, rating=None, queue=False, into=None, slots=None, gids=None, id_base=0):
    """The emulated k_branch_add over the storages U [S][Hn][n] and the list of distortion_emul.list_args with records (flags, thd_max) -> dict
    of the ABI's arrays; `into`: keep going"""
    lib = load()
    _, Hn, n = U.shape
    nb = len(fr)
    fr, to, yb, Ub = _device_layout(fr, to, y, U)
    out = empty(nb) if into is None else into
    f = np.stack([out[k] for k in _F])
    arg = np.stack([out[k] for k in _A])
    head, recs = list_args(ids, flags, thd_max, slots, gids, id_base)
    lim = np.ascontiguousarray(np.full(nb, np.inf) if rating is None else rating, dtype=np.float64)
    lib.emul_branch_add(C.c_int(n), C.c_int(Hn), C.c_int(nb), *head, _p(fr), _p(to), _p(yb), _p(Ub), *recs, C.c_int(int(queue)), _p(lim),
                        _p(out["counts"]), _p(f), _p(arg), _p(out["irms_over"]))
    for i, k in enumerate(_F):
        out[k] = f[i].copy()
    for i, k in enumerate(_A):
        out[k] = arg[i].copy()
    return out


def midpoint_limit(v):
    """Midpoint between the two adjacent sorted values of v around its median: about half the samples lie above, none on it."""
    s = np.sort(np.asarray(v).ravel())
    k = len(s) // 2
    return 0.5 * (s[k - 1] + s[k])


_NETS = {}


def network(name):
    """Golden case `name` ("net1_H51_c", "lin4_H11_c", "syn1000_H51_c", ...) -> dict: buses, lines, n, Hn, harmonics, rowptr, col, Yval (the
    package's admittances, pinned bit for bit to the reference's Y_all by the oracle tests), fr / to / ypos / y of its branches, and the golden's
    final voltages Vm, Va [Hn*n] (stacked order)."""
    if name in _NETS:
        return _NETS[name]
    import harmonic_power_flow_amd as hp
    from harmonic_power_flow_amd import synth
    g = np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=True)
    net = name.split("_")[0]
    if net.startswith("syn"):
        fb, fl = synth.gen(int(net[3:]), seed=0, outdir=tempfile.mkdtemp())
    else:
        fb, fl = os.path.join(INPUTS, net + "_buses.csv"), os.path.join(INPUTS, net + "_lines.csv")
    harmonics = [int(h) for h in g["harmonics"]]
    st = hp.Settings(H_MAX=max(harmonics))
    assert list(st.HARMONICS) == harmonics
    buses, lines, m, n, c = hp.init_network(fb, fl, settings=st)
    Y = hp.build_admittance_matrices(buses, lines, harmonics)
    fr, to, ypos = ref.branches(Y.rowptr, Y.col)
    out = dict(buses=buses, lines=lines, n=n, Hn=len(harmonics), harmonics=harmonics, rowptr=Y.rowptr, col=Y.col, Yval=Y.Yval, fr=fr, to=to,
               ypos=ypos, y=ref.series(Y.Yval, ypos), Vm=g["V_final"][:, 0].astype(np.float64), Va=g["V_final"][:, 1].astype(np.float64),
               files=(fb, fl), settings=st)
    _NETS[name] = out
    return out


def scenario_set(net, S=20):
    """The golden's final voltages replicated into S scenarios with small deterministic perturbations of magnitude and angle; scenario 7 did not
    converge -> Vm, Va [S][Hn*n], ids, flags"""
    k = np.arange(len(net["Vm"]))
    Vm = np.stack([net["Vm"] * (1.0 + 0.03 * np.sin(0.7 * s + 0.37 * k) + 0.002 * s) for s in range(S)])
    Va = np.stack([net["Va"] + 1e-3 * np.cos(0.3 * s + 0.11 * k) for s in range(S)])
    flags = np.ones(S, dtype=np.int32)
    if S > 7:
        flags[7] = 2
    return Vm, Va, np.arange(S), flags
