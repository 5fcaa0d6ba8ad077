"""Loader of the host emulation of the harmonic penetration (tests/cpu_emul/pen_emul.cpp: the functions of csrc/hpf_penetration.hpp in the
kernels' order), the inputs the penetration tests share and their dense reference.  Test infrastructure only."""
import ctypes as C
import os
import subprocess

import numpy as np

import zscan_emul as ze
import zscan_ref as ref

SRC = os.path.join(ze.HERE, "cpu_emul", "pen_emul.cpp")
LIB = os.path.join(ze.HERE, "cpu_emul", "libhpf_pen_emul.so")
HDRS = ze.HDRS                                              # (hpf_penetration.hpp and zfactor_emul.hpp are among them)
OUTPUTS = ("V", "rss", "vmax", "varg", "vsum", "vsumsq", "rss_max", "rss_arg", "rss_sum", "rss_sumsq")


def load():
    if (not os.path.exists(LIB)) or os.path.getmtime(LIB) < max(os.path.getmtime(p) for p in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", ze.CSRC, SRC, "-o", LIB])
    return C.CDLL(LIB)


def outputs(n, F, S, full=True):
    """Fresh output arrays of one call, in the order of OUTPUTS (V is None with full=False)"""
    return dict(V=np.empty((S, F, n), dtype=np.complex128) if full else None, rss=np.empty((S, n)),
                vmax=np.empty((F, n)), varg=np.empty((F, n), dtype=np.int32), vsum=np.empty((F, n)), vsumsq=np.empty((F, n)),
                rss_max=np.empty(n), rss_arg=np.empty(n, dtype=np.int32), rss_sum=np.empty(n), rss_sumsq=np.empty(n))


def penetration(model, h, I, inj, y_extra=None, chunk_f=0, chunk_s=0, full=True):
    """The emulated hpf_penetration -> (code, dict of arrays), like api.penetration_arrays"""
    lib = load()
    n, F = int(model["n"]), len(h)
    keep, args = ze._net_args(model)
    h = np.ascontiguousarray(h, dtype=np.float64)
    inj = np.ascontiguousarray(inj, dtype=np.int32)
    I = np.ascontiguousarray(I, dtype=np.complex128)
    S = I.shape[0]
    assert I.shape == (S, F, len(inj))
    yx = None if y_extra is None else np.ascontiguousarray(y_extra, dtype=np.complex128)
    out = outputs(n, F, S, full)
    rc = lib.emul_penetration(*args, C.c_int(F), ze._p(h), ze._p(yx), C.c_int(S), C.c_int(len(inj)), ze._p(inj), ze._p(I), C.c_int(int(chunk_f)),
                              C.c_int(int(chunk_s)), *[ze._p(out[k]) for k in OUTPUTS])
    assert rc in (0, 3), rc
    return rc, out


def chunks(F, S, chunk_f, chunk_s, per_f, per_j):
    """The header's chunk lengths -> (Fc, Sc)"""
    a, b = C.c_int32(), C.c_int32()
    load().emul_pen_chunks(C.c_int(F), C.c_int(S), C.c_int(chunk_f), C.c_int(chunk_s), C.c_longlong(per_f), C.c_longlong(per_j), C.byref(a), C.byref(b))
    return a.value, b.value


def currents(S, F, n_inj, seed=0):
    """Seeded injected currents [S][F][n_inj]: magnitudes 0.01 .. 1, any angle"""
    rng = np.random.default_rng(seed)
    return rng.uniform(0.01, 1.0, (S, F, n_inj)) * np.exp(2j * np.pi * rng.uniform(size=(S, F, n_inj)))


def dense(model, h, I, inj, y_extra=None):
    """numpy.linalg.solve on zscan_ref.dense_Y -> V [S][F][n], kappa_2 [F]"""
    n, (S, F, _) = int(model["n"]), I.shape
    V, kappa = np.empty((S, F, n), dtype=np.complex128), np.empty(F)
    for f, x in enumerate(h):
        Y = ref.dense_Y(model, x, None if y_extra is None else y_extra[f])
        kappa[f] = np.linalg.cond(Y, 2)
        b = np.zeros((n, S), dtype=np.complex128)
        b[np.asarray(inj)] = I[:, f, :].T
        V[:, f, :] = np.linalg.solve(Y, b).T
    return V, kappa


def bound_share(V, Vref, kappa):
    """the error of every (s, f), relative to max_i |Vref_i|, over 2^-52 kappa_2 of the point -> [S][F]"""
    err = np.abs(V - Vref).max(axis=2) / np.abs(Vref).max(axis=2)
    return err / (ref.EPS * kappa[None, :])


def stats_numpy(V):
    """The statistics of hpf_penetration from V [S][F][n] with every operation rounded on its own and the sums in the header's order"""
    a = np.sqrt(V.real * V.real + V.imag * V.imag)
    sq = np.zeros(a[:, 0, :].shape)
    for f in range(V.shape[1]):
        sq = sq + (V[:, f, :].real * V[:, f, :].real + V[:, f, :].imag * V[:, f, :].imag)
    rss = np.sqrt(sq)

    def four(x):                                            # x [S][...]: over axis 0, ascending
        s1, s2 = np.zeros(x.shape[1:]), np.zeros(x.shape[1:])
        for row in x:
            s1, s2 = s1 + row, s2 + row * row
        return x.max(axis=0), x.argmax(axis=0).astype(np.int32), s1, s2
    out = dict(rss=rss)
    out["vmax"], out["varg"], out["vsum"], out["vsumsq"] = four(a)
    out["rss_max"], out["rss_arg"], out["rss_sum"], out["rss_sumsq"] = four(rss)
    return out


def same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
