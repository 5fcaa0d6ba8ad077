"""Loader of the host emulation of the distortion accumulator (tests/cpu_emul/distortion_emul.cpp: the per-entry functions of
csrc/hpf_distortion.hpp, what k_distortion_add runs per thread) and the scenario sets the host tests share.  Test infrastructure only."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpu_emul", "distortion_emul.cpp")
LIB = os.path.join(HERE, "cpu_emul", "libhpf_distortion_emul.so")
CSRC = os.path.join(os.path.dirname(HERE), "harmonic-power-flow_amd", "csrc")
HDRS = [os.path.join(CSRC, f) for f in ("hpf_distortion.hpp", "hpf_accum.hpp")]
GOLD = os.path.join(HERE, "golden")

SHAPES = (lambda n, Hn, B: (3,),) + (lambda n, Hn, B: (Hn, n),) * 5 + (lambda n, Hn, B: (n,),) * 5 + (lambda n, Hn, B: (n, B + 1),)
NAMES = ("counts", "x_max", "x_arg", "x_sum", "x_sumsq", "x_over", "thd_max", "thd_arg", "thd_sum", "thd_sumsq", "thd_over", "thd_hist")
DTYPES = (np.int64, np.float64, np.int32, np.float64, np.float64, np.uint32, np.float64, np.int32, np.float64, np.float64, np.uint32, np.uint32)


def load():
    if (not os.path.exists(LIB)) or os.path.getmtime(LIB) < max(os.path.getmtime(p) for p in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", CSRC, SRC, "-o", LIB])
    return C.CDLL(LIB)


def list_args(ids, flags, thd_max=None, slots=None, gids=None, id_base=0):
    """The device's scenario list (csrc/hpf_accum.hpp) from per-entry arrays, for the three emulated accumulators: entry l is storage slots[l]
    (None: l; a negative slot ends the list) with scenario number gids[l] and id id_base + number.  gids None: the numbers are `ids`, the tests'
    free labels (id_base 0); both None: the number is l, and the emulator gets NULL as the device does.  flags / thd_max [L] are the records of
    the entries; the emulators index records by number -> (ctypes L, slots, gids, id_base, nrec), (ctypes flags, thd_max by number)."""
    L = len(flags)
    g = gids if gids is not None else ids
    num = np.arange(L) if g is None else np.asarray(g)
    assert gids is not None or id_base == 0
    nrec = int(num.max()) + 1 if L else 0
    fl, th = np.zeros(nrec, dtype=np.int32), np.zeros(nrec)
    fl[num] = flags
    if thd_max is not None:
        th[num] = thd_max

    def ptr(a):
        return None if a is None else np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(C.c_void_p)

    return ((C.c_int(L), ptr(slots), ptr(g), C.c_int(id_base), C.c_int(nrec)), (fl.ctypes.data_as(C.c_void_p), th.ctypes.data_as(C.c_void_p)))


def empty(n, Hn, bins):
    out = {name: np.zeros(sh(n, Hn, bins), dtype=dt) for name, dt, sh in zip(NAMES, DTYPES, SHAPES)}
    out["x_arg"][:] = -1
    out["thd_arg"][:] = -1
    return out


def accumulate(Vm, ids, flags, n, Hn, limit=None, thd_limit=np.inf, hist_max=1.0, bins=64, queue=False, into=None, slots=None, gids=None,
               id_base=0):
    """The emulated accumulator over the storages Vm [S][Hn*n] (stacked order) and the list of list_args -> dict of the ABI's arrays; `into`:
    keep accumulating."""
    lib = load()
    out = empty(n, Hn, bins) if into is None else into
    Vm = np.ascontiguousarray(Vm, dtype=np.float64)
    head, (fl, _) = list_args(ids, flags, None, slots, gids, id_base)
    lim = np.ascontiguousarray(np.full(Hn, np.inf) if limit is None else limit, dtype=np.float64)
    lib.emul_distortion(C.c_int(n), C.c_int(Hn), *head, Vm.ctypes.data_as(C.c_void_p), fl, C.c_int(int(queue)), lim.ctypes.data_as(C.c_void_p),
                        C.c_double(thd_limit), C.c_double(hist_max), C.c_int(bins), *[out[name].ctypes.data_as(C.c_void_p) for name in NAMES])
    return out


LIST_TIED = (1, 4)       # list_cases: the tests give these two storages the same, largest state


def list_cases(S=6):
    """The list cases the three accumulator tests share, the rules of csrc/hpf_accum.hpp restated in NumPy over S = 6 storages:
    (a) a -1 at position 3 of the slots: the entries from there on count for nothing (one of them did not converge: not even skipped);
    (b) gids a permutation, id_base 1000: of the tied storages LIST_TIED the later one carries the smaller id;
    (c) no slots, no gids (NULL to the emulator); a warm-started (bit 8) and a rectangular-update (bit 9) record that did not converge are
        deferred whoever asks, one plain non-converged record is skipped.
    -> [(keywords flags / slots / gids / id_base of accumulate, storages, ids, flags and deferred mask of the entries that count, counts)]"""
    one = np.ones(S, dtype=np.int32)
    fa, fc = one.copy(), one.copy()
    fa[4] = 2
    fc[[1, 3, 5]] = 256 | 2, 512 | 2, 2
    out = []
    for kw, counts in ((dict(flags=fa, slots=np.array([4, 2, 5, -1, 1, 0]), gids=None, id_base=0), [3, 0, 0]),
                       (dict(flags=one, slots=None, gids=np.array([3, 5, 0, 4, 1, 2]), id_base=1000), [6, 0, 0]),
                       (dict(flags=fc, slots=None, gids=None, id_base=0), [3, 1, 2])):
        slots = np.arange(S) if kw["slots"] is None else kw["slots"]
        k = int(np.argmax(slots < 0)) if (slots < 0).any() else S
        num = np.arange(S) if kw["gids"] is None else kw["gids"]
        fl = kw["flags"][:k]
        out.append((kw, slots[:k], kw["id_base"] + num[:k], fl, ((fl & (256 | 512)) != 0) & ((fl & 1) == 0), counts))
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
