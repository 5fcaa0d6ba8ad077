"""Loader of the host emulation of the per-scenario source currents (tests/cpu_emul/sources_emul.cpp: the functions of csrc/hpf_sources.hpp and the
mismatch row with a source pointer) and the scenario generator the source tests share.  Test infrastructure only."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpu_emul", "sources_emul.cpp")
LIB = os.path.join(HERE, "cpu_emul", "libhpf_sources_emul.so")
CSRC = os.path.join(os.path.dirname(HERE), "harmonic-power-flow_amd", "csrc")
HDRS = [os.path.join(CSRC, f) for f in ("hpf_sources.hpp", "hpf_assembly.hpp")]

# the source scenarios of tests/test_sources_oracle.py and tests/test_gpu_sources.py: S_SCEN scenarios, scale a in A_RANGE, shift phi in PHI_RANGE (rad)
S_SCEN = 24
# (the ranges a in [0.5, 1.5], phi in [-0.3, 0.3] were tried first: the ORACLE's harmonic NR -- the reference's polar update from its flat start --
#  diverges on all 24 coupled syn100 scenarios with them and on 4 - 5 of 24 at half that width; at a quarter it converges on every one)
A_RANGE = (0.875, 1.125)
PHI_RANGE = (-0.075, 0.075)
SEED = 20260


def scale_shift(nnl, n_scen=S_SCEN, seed=SEED):
    """-> (a, phi) [n_scen][nnl]: units in service and time shift (rad at the fundamental) of every nonlinear bus, fixed seed"""
    rng = np.random.default_rng(seed)
    return rng.uniform(*A_RANGE, size=(n_scen, nnl)), rng.uniform(*PHI_RANGE, size=(n_scen, nnl))


def load():
    if (not os.path.exists(LIB)) or os.path.getmtime(LIB) < max(os.path.getmtime(p) for p in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-mfma", "-fPIC", "-shared", "-I", CSRC, SRC, "-o", LIB])
    return C.CDLL(LIB)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def expand(a, phi, order, i_n, cs=None):
    """source_expand over flat arrays (cs = (cos, sin): source_from_cs with those values) -> complex array"""
    lib = load()
    a, phi = (np.ascontiguousarray(x, dtype=np.float64) for x in (a, phi))
    order = np.ascontiguousarray(order, dtype=np.int32)
    i_n = np.ascontiguousarray(i_n, dtype=np.complex128)
    out = np.empty(len(a), dtype=np.complex128)
    if cs is None:
        lib.emul_source_expand(C.c_int(len(a)), _p(a), _p(phi), _p(order), _p(i_n), _p(out))
    else:
        c, s = (np.ascontiguousarray(x, dtype=np.float64) for x in cs)
        lib.emul_source_from_cs(C.c_int(len(a)), _p(a), _p(c), _p(s), _p(i_n), _p(out))
    return out


def mismatch(n, m, c, Hn, rowptr, col, Yval, dev, Y_N, I_N, coupled, U, P, Q, src=None):
    """emulated harmonic mismatch f [N] of one scenario (host layouts: Yval [Hn][nnz], U stacked q*n + i); src [n-m][Hn] complex or None"""
    lib = load()
    rowptr, col, dev = (np.ascontiguousarray(x, dtype=np.int32) for x in (rowptr, col, dev))
    diag = np.array([rowptr[i] + list(col[rowptr[i]:rowptr[i + 1]]).index(i) for i in range(n)], dtype=np.int32)
    Yval, Y_N, I_N, U = (np.ascontiguousarray(x, dtype=np.complex128) for x in (Yval, Y_N, I_N, U))
    P, Q = (np.ascontiguousarray(x, dtype=np.float64) for x in (P, Q))
    src = None if src is None else np.ascontiguousarray(src, dtype=np.complex128)
    f = np.empty(2 * n * Hn - 1 - c)
    lib.emul_mismatch_sources(C.c_int(n), C.c_int(m), C.c_int(c), C.c_int(Hn), C.c_int(len(col)), C.c_int(len(I_N)), C.c_int(int(coupled)),
                              _p(rowptr), _p(col), _p(diag), _p(Yval), _p(dev), _p(Y_N), _p(I_N), _p(U), _p(P), _p(Q),
                              _p(src) if src is not None else None, _p(f))
    return f


# ---- the independent reference: the unmodified oracle on a network whose nonlinear buses each have a device of their own -------------------------
def oracle_network(fb, fl, harmonics, coupled, ne_dir):
    """-> dict(net, mats = (rowptr, col, Yval), NE, I_N_bus [n-m][Hn]: the model's source currents of every nonlinear bus)"""
    import hpf_oracle as o
    net = o.init_network(fb, fl)
    mats = o.build_admittance_matrices(net, harmonics)
    NE = o.import_Norton_Equivalents(net, harmonics, coupled, ne_dir)
    I_N_bus = np.array([NE[net.component[i]][0] for i in range(net.m, net.n)], dtype=np.complex128).reshape(net.n - net.m, len(harmonics))
    return dict(net=net, mats=mats, NE=NE, I_N_bus=I_N_bus, harmonics=list(harmonics), coupled=coupled)


def oracle_solve(case, load_scale, I_src, thresh_h=1e-9, max_iter_h=50):
    """The oracle's pf + harmonic NR of one scenario: loads scaled per bus by load_scale [n], source currents I_src [n-m][Hn] (None: the model's).
    oracle/hpf_oracle.py looks Norton data up per bus through net.component: every nonlinear bus gets a component name of its own and an NE entry
    (I_src of the bus, the Y_N of its device) -- the unmodified oracle then solves exactly the scenario with per-bus sources."""
    import copy
    import hpf_oracle as o
    net, (rowptr, col, Yval), NE = case["net"], case["mats"], case["NE"]
    nt = copy.copy(net)
    nt.P, nt.Q = net.P * load_scale, net.Q * load_scale
    if I_src is not None:
        nt.component = np.array(net.component, dtype=object)
        NE = dict(NE)
        for i in range(net.m, net.n):
            name = "source_bus_%d" % i
            NE[name] = (np.asarray(I_src[i - net.m], dtype=complex), NE[net.component[i]][1])
            nt.component[i] = name
    Vm, Va, _, _ = o.pf(nt, rowptr, col, Yval)
    mdl = o.Model(nt, case["harmonics"], rowptr, col, Yval, NE, case["coupled"])
    return o.hpf_from_model(mdl, Vm, Va, thresh_h=thresh_h, max_iter_h=max_iter_h)
