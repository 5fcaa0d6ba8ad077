"""Loader of the host emulation of the resonance mode analysis (tests/cpu_emul/rma_emul.cpp: the functions of csrc/hpf_resonance.hpp in the
kernels' order), the networks the resonance tests share and their dense reference (numpy.linalg.eig of zscan_ref.dense_Y).  Test infrastructure
only."""
import ctypes as C
import os
import subprocess

import numpy as np

import zscan_emul as ze
import zscan_ref as ref

SRC = os.path.join(ze.HERE, "cpu_emul", "rma_emul.cpp")
LIB = os.path.join(ze.HERE, "cpu_emul", "libhpf_rma_emul.so")
HDRS = ze.HDRS + [os.path.join(ze.CSRC, "hpf_resonance.hpp")]
OUTPUTS = ("lam", "zm", "res", "top", "pf")
GRID = np.linspace(0.5, 50.5, 130)
BANKS = {"syn12": {5: 0.002, 9: 0.02}, "syn40": {17: 0.01, 33: 0.004}}


def load():
    if (not os.path.exists(LIB)) or os.path.getmtime(LIB) < max(os.path.getmtime(p) for p in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", ze.CSRC, SRC, "-o", LIB])
    return C.CDLL(LIB)


def shape(name):
    """-> (model, banks) of a shape's name: n1, n2, chainN, starN, synN (with the banks of BANKS), net1"""
    if name in ("n1", "n2"):
        return ze.chain(int(name[1:])), {}
    if name.startswith("chain"):
        return ze.chain(int(name[5:])), {}
    if name.startswith("star"):
        return ze.star(int(name[4:])), {}
    return ze.network(name)["model"], BANKS.get(name, {})


def y_extra(model, h, banks):
    return ze.capacitors(model, h, banks) if banks else None


def outputs(n, F, full=True):
    return dict(lam=np.empty(F, dtype=np.complex128), zm=np.empty(F), res=np.empty(F), top=np.empty(F, dtype=np.int32),
                pf=np.empty((F, n), dtype=np.complex128) if full else None)


def modes(model, h, y_extra=None, iters=32, chunk=0, full=True):
    """The emulated hpf_resonance_modes -> (code, dict of the arrays OUTPUTS; pf is None with full=False), like api.resonance_modes_arrays"""
    lib = load()
    n, F = int(model["n"]), len(h)
    keep, args = ze._net_args(model)
    h = np.ascontiguousarray(h, dtype=np.float64)
    yx = None if y_extra is None else np.ascontiguousarray(y_extra, dtype=np.complex128)
    out = outputs(n, F, full)
    rc = lib.emul_resonance_modes(*args, C.c_int(F), ze._p(h), ze._p(yx), C.c_int(int(iters)), C.c_int(int(chunk)), *[ze._p(out[k]) for k in OUTPUTS])
    assert rc in (0, 3), rc
    return rc, out


_DENSE = {}


def dense(name, h=GRID):
    """numpy.linalg.eig of the dense Y(h) of a shape on the grid h, computed once per (shape, grid) and shared (left unchanged) -> dict of
    lam1 [F] the eigenvalue of smallest modulus, gap [F] = |lam1 / lam2|, pf [F][n] = v_i^2 / sum_j v_j^2 of its eigenvector, kY [F] = kappa_2(Y),
    nY [F] = ||Y||_2, kV [F] = kappa_2 of the eigenvector matrix, sep [F] = min_{j != 1} |lam_j - lam1|"""
    key = (name, len(h), float(h[0]), float(h[-1]))
    if key not in _DENSE:
        model, banks = shape(name)
        n, F = int(model["n"]), len(h)
        yx = y_extra(model, h, banks)
        d = dict(lam1=np.empty(F, dtype=np.complex128), gap=np.empty(F), pf=np.empty((F, n), dtype=np.complex128), kY=np.empty(F), nY=np.empty(F),
                 kV=np.empty(F), sep=np.empty(F))
        for f, x in enumerate(h):
            Y = ref.dense_Y(model, x, None if yx is None else yx[f])
            lam, V = np.linalg.eig(Y)
            order = np.argsort(np.abs(lam))
            l1, v = lam[order[0]], V[:, order[0]]
            sv = np.linalg.svd(Y, compute_uv=False)
            d["lam1"][f], d["pf"][f] = l1, v * v / np.sum(v * v)
            d["gap"][f] = abs(l1) / abs(lam[order[1]]) if n > 1 else 0.0
            d["sep"][f] = np.abs(lam[order[1:]] - l1).min() if n > 1 else np.inf
            d["kY"][f], d["nY"][f], d["kV"][f] = sv[0] / sv[-1], sv[0], np.linalg.cond(V, 2)
        _DENSE[key] = d
    return _DENSE[key]


def bound_shares(out, d):
    """-> the share used of the eigenvalue bound 4 eps kappa_2(Y) kappa_2(V) and of the participation bound 4 eps ||Y||_2 kappa_2(V) / sep, [F] each"""
    e_lam = np.abs(out["lam"] - d["lam1"]) / np.abs(d["lam1"])
    e_pf = np.abs(out["pf"] - d["pf"]).max(axis=1)
    return e_lam / (4 * ref.EPS * d["kY"] * d["kV"]), e_pf / (4 * ref.EPS * d["nY"] * d["kV"] / d["sep"])


def same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
