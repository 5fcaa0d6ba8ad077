"""The reference's call shapes (`Harmonic Power Flow/hcne_generalized.py`, HG) on top of the HIP library.

Same names, argument meaning, return objects and printed warnings as the reference: `init_network` HG:113,
`build_admittance_matrices` HG:132, `import_Norton_Equivalents` HG:278, `pf` HG:244, `hpf` HG:511,
`harmonic_mismatch` HG:360, `build_harmonic_jacobian` HG:401, `update_harmonic_state_vec` HG:476, `get_THD` HG:563,
plus the `solve` convenience wrapper the north-star asks for.  The reference reads module globals (`buses, m, n, c,
HARMONICS, base_*`); here they live in an explicit `Settings` object, with a module-level
default (`settings`) and a "current network" context filled by `init_network`, so reference-style scripts keep
working unchanged.

Everything numerical runs on the GPU through `DeviceModel`; nothing here falls back to the CPU.
"""
import atexit
import collections
import contextlib
import hashlib
import os

import numpy as np
import pandas as pd
import scipy.sparse as sp

import ctypes as C

from . import _lib, admittance, ingest
from .device import DeviceModel
from .settings import Settings

settings = Settings()          # module-level defaults, HG:578-593
_ctx = {"buses": None, "lines": None}


class AdmittanceSet:
    """Per-harmonic admittance matrices in device layout (shared CSR pattern).  `to_frame()` gives the reference's
    dense `Y_all` DataFrame."""

    def __init__(self, rowptr, col, Yval, harmonics, n):
        self.rowptr, self.col, self.Yval, self.harmonics, self.n = rowptr, col, Yval, list(harmonics), n
        self._key = None              # digest of the three arrays (handle cache), computed once per object

    def key(self):
        if self._key is None:
            self._key = _digest(self.rowptr, self.col, self.Yval)
        return self._key

    def to_frame(self):
        return admittance.to_dense_frame(self.rowptr, self.col, self.Yval, self.harmonics, self.n)

    def dense(self, h):
        q = self.harmonics.index(h)
        return sp.csr_matrix((self.Yval[q], self.col, self.rowptr), shape=(self.n, self.n)).toarray()


def _as_admittance(Y, harmonics, n):
    if isinstance(Y, AdmittanceSet):
        return Y
    rowptr, col, Yval = admittance.from_dense_frame(Y, harmonics, n)
    return AdmittanceSet(rowptr, col, Yval, harmonics, n)


def init_network(filename_buses, filename_lines, from_csv=True, settings=None):
    """HG:113-128."""
    st = settings or globals()["settings"]
    buses, lines, m, n, c = ingest.init_network(filename_buses, filename_lines, from_csv, st)
    _ctx["buses"], _ctx["lines"] = buses, lines
    return buses, lines, m, n, c


_ADMITTANCES = collections.OrderedDict()      # digest of the inputs -> AdmittanceSet: repeated hpf() calls on one network (HG:511) build it once


def build_admittance_matrices(buses, lines, harmonics):
    """HG:132-171 -> AdmittanceSet (call `.to_frame()` for the reference's DataFrame).  The result is a function of the line table, the bus
    shunts and the harmonics alone; the last four are kept (by a digest of exactly those inputs), so the reference's sweep -- hpf() per load
    case -- builds the matrices of a network once.  Treat an AdmittanceSet as read-only."""
    harmonics = list(harmonics)
    key = _digest(lines.fromID.to_numpy(), lines.toID.to_numpy(), lines.R.to_numpy(dtype=float), lines.X.to_numpy(dtype=float),
                  lines.G.to_numpy(dtype=float), lines.B.to_numpy(dtype=float), buses["X_sh"].to_numpy(dtype=float),
                  np.asarray(harmonics, dtype=np.int64))
    hit = _ADMITTANCES.pop(key, None)
    if hit is None:
        rowptr, col, Yval = admittance.build_admittance_csr(buses, lines, harmonics)
        hit = AdmittanceSet(rowptr, col, Yval, harmonics, len(buses))
    _ADMITTANCES[key] = hit
    while len(_ADMITTANCES) > 4:
        _ADMITTANCES.popitem(last=False)
    return hit


def import_Norton_Equivalents(buses, coupled, settings=None, ne_dir=None):
    """HG:278-310."""
    return ingest.import_Norton_Equivalents(buses, coupled, settings or globals()["settings"], ne_dir)


def init_voltages(buses, harmonics):
    """HG:174-184."""
    idx = pd.MultiIndex.from_product([list(harmonics), buses.index.values], names=["harmonic", "bus"])
    V = pd.DataFrame(np.zeros((len(harmonics) * len(buses), 2)), index=idx, columns=["V_m", "V_a"])
    V.iloc[:len(buses), 0] = 1
    V.iloc[len(buses):, 0] = 0.1
    return V


_FRAME_INDEX = {}


def _frame(Vm, Va, harmonics, n):
    key = (tuple(harmonics), int(n))
    idx = _FRAME_INDEX.get(key)                          # (a MultiIndex is immutable: the result frames of repeated calls share it; 0.5 ms per build)
    if idx is None:
        if len(_FRAME_INDEX) > 8:
            _FRAME_INDEX.clear()
        idx = _FRAME_INDEX[key] = pd.MultiIndex.from_product([list(harmonics), list(range(n))], names=["harmonic", "bus"])
    return pd.DataFrame({"V_m": np.asarray(Vm), "V_a": np.asarray(Va)}, index=idx)


def _device_model(buses, Y, NE, coupled, harmonics, solver="auto", max_scenarios=1, device=0, assembly_only=False, options=None):
    m, n, c = ingest.network_constants(buses)
    Hn = len(harmonics)
    if NE is None:
        dev = np.full(n, -1, dtype=np.int32)
        dev[m:] = 0
        Y_N = np.zeros((1, Hn, Hn) if coupled else (1, Hn), dtype=np.complex128)
        I_N = np.zeros((1, Hn), dtype=np.complex128)
        n_dev = 1
    else:
        dev, Y_N, I_N, n_dev = ingest.norton_arrays(buses, NE, coupled, Hn)
    return DeviceModel(n, m, c, harmonics, Y.rowptr, Y.col, Y.Yval, dev, Y_N, I_N, n_dev, coupled,
                       solver=solver, device=device, max_scenarios=max_scenarios, assembly_only=assembly_only, options=options)


# ---- handle cache -------------------------------------------------------------------------------------------------------------------------
# The reference's sweep is repeated hpf() calls (HG:511) with other buses.P / buses.Q; its functions are stateless, ours own a device handle whose
# creation (tree planning on the host, uploads, allocation: 15 ms at 1 000 buses x 26 harmonics) costs more than the solve.  The reference call
# shapes therefore BORROW a handle from a small LRU keyed on everything hpf_create consumes -- network constants, admittance pattern and values,
# Norton arrays, harmonics, solver, and the HPF_* environment switches hpf_create reads -- and set loads / state / options themselves on every
# call, so a borrowed handle and a fresh one give bit-identical results.  Not thread-safe (neither is the reference: module globals).
_HANDLES = collections.OrderedDict()
_HANDLE_CACHE = {"size": 4, "hits": 0, "misses": 0}


def _digest(*arrays):
    h = hashlib.blake2b(digest_size=16)
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str((a.dtype.str, a.shape)).encode())
        h.update(a.view(np.uint8).reshape(-1).data)
    return h.digest()


def handle_cache(size=None):
    """Size of the LRU of device handles behind hpf / pf / harmonic_mismatch / build_harmonic_jacobian (default 4; 0 switches it off: every
    call creates and destroys its own handle, as before round 5).  Returns the statistics dict (size, hits, misses)."""
    if size is not None:
        _HANDLE_CACHE["size"] = max(int(size), 0)
        while len(_HANDLES) > _HANDLE_CACHE["size"]:
            _HANDLES.popitem(last=False)[1].close()
    return dict(_HANDLE_CACHE, held=len(_HANDLES))


def close_all():
    """Destroy every cached device handle (also run at interpreter exit)."""
    while _HANDLES:
        _HANDLES.popitem(last=False)[1].close()


atexit.register(close_all)


@contextlib.contextmanager
def _borrow_model(buses, Y, NE, coupled, harmonics, solver="auto", assembly_only=False, device=0):
    """A DeviceModel of one scenario for the duration of a reference-shaped call: from the cache, or created (and then kept)."""
    if _HANDLE_CACHE["size"] <= 0:
        dm = _device_model(buses, Y, NE, coupled, harmonics, solver=solver, device=device, assembly_only=assembly_only)
        try:
            yield dm
        finally:
            dm.close()
        return
    m, n, c = ingest.network_constants(buses)
    if NE is None:
        ne_key = b"none"
    else:
        dev, Y_N, I_N, n_dev = ingest.norton_arrays(buses, NE, coupled, len(harmonics))
        ne_key = _digest(dev, Y_N, I_N)
    # (the environment is part of a handle's build only under HPF_ENV_SWITCHES=1 -- hpf.h -- but keying on it always is harmless)
    env = tuple(sorted((k, v) for k, v in os.environ.items() if k.startswith("HPF_")))
    key = (n, m, c, tuple(harmonics), bool(coupled), solver, bool(assembly_only), int(device), Y.key(), ne_key, env)
    dm = _HANDLES.pop(key, None)
    if dm is None:
        _HANDLE_CACHE["misses"] += 1
        dm = _device_model(buses, Y, NE, coupled, harmonics, solver=solver, device=device, assembly_only=assembly_only)
    else:
        _HANDLE_CACHE["hits"] += 1
    try:
        yield dm
    except BaseException:
        dm.close()                                     # (a failed call may leave the handle in any state: not kept)
        raise
    _HANDLES[key] = dm
    while len(_HANDLES) > _HANDLE_CACHE["size"]:
        _HANDLES.popitem(last=False)[1].close()


def pf(Y, buses, thresh_f=1e-6, max_iter_f=30, plt_convergence=False, settings=None, verbose=True, _model=None):
    """HG:244-275 -> (V, err_t, n_iter_f): fundamental Newton-Raphson on the device from the reference's start
    (1 p.u. / 0.1 p.u., angle 0)."""
    st = settings or globals()["settings"]
    n = len(buses)
    Y = _as_admittance(Y, st.HARMONICS, n)
    with (contextlib.nullcontext(_model) if _model is not None else _borrow_model(buses, Y, None, False, Y.harmonics, solver="dense")) as dm:
        dm.set_loads(buses["P"].to_numpy(dtype=float), buses["Q"].to_numpy(dtype=float))
        dm.set_state(None, None, n_scen=1)
        n_iter, err, hist = dm.fund_pf(thresh_f, max_iter_f)
        Vm, Va = dm.get_state()
    n_iter_f = int(n_iter[0])
    err_t = {i: float(hist[0, i]) for i in range(n_iter_f)}
    V = _frame(Vm[0], Va[0], Y.harmonics, n)
    if plt_convergence:
        import matplotlib.pyplot as plt
        plt.plot(list(err_t.keys()), list(err_t.values()))
    if verbose:
        print(V.loc[Y.harmonics[0]])
        if n_iter_f < max_iter_f:
            print("Fundamental power flow converged after " + str(n_iter_f) + " iterations.")
        elif n_iter_f == max_iter_f:
            print("Warning! Maximum of " + str(n_iter_f) + " iterations reached.")
    return V, err_t, n_iter_f


def _postprocess(Vm, Va):
    """HG:545-549."""
    Vm, Va = Vm.copy(), Va.copy()
    neg = Vm < 0
    Va[neg] += np.pi
    Va = Va % (2 * np.pi)
    Vm[neg] = -Vm[neg]
    return Vm, Va


def hpf(buses, lines, coupled, thresh_h=1e-4, max_iter_h=50, plt_convergence=False, settings=None, ne_dir=None,
        solver="auto", verbose=True, return_jacobian=True, details=None, extra_iters=0, check_steps=False, update="polar", sources=None):
    """HG:511-560 -> (V, err_h, n_iter_h, J).

    `sources` (not in the reference, default None = the Norton source currents I_N of the device files): source currents of the nonlinear buses for
    this one scenario (include/hpf.h "Source currents") -- {"scale": [n-m], "shift": [n-m]} (either may be missing: 1 / 0): scale
    units of each bus's device, their waveform shifted in time by shift rad at the fundamental; or {"currents": [n-m][Hn]} complex, p.u., used as
    given.  Y_N stays the device's.  ValueError for wrong shapes, before any device call.

    `update` (not in the reference, default "polar" = the reference's update): "rectangular" applies every harmonic Newton step to
    U = Vm e^(j Va) instead of adding it to (Va, Vm) (option "rectangular_update", include/hpf.h): 3 - 4 iterations from the
    reference's start where the reference takes 20 - 30, the same fixed point, other iterates -- n_iter_h, err_h and the last digits of V differ
    from the reference's.  The handle's option is put back on return.  ValueError for any other string.

    `check_steps` (not in the reference, default False): every harmonic Newton step's normwise backward error is evaluated on the device
    (option "step_residual_check"); a step above the limit repeats the solve with partial pivoting (radial block tree) or retries it on
    the dense LU (meshed, solver="auto"); `details` then carries step_eta_max and step_flagged.

    `J` is the Jacobian of the last iteration as scipy CSR like the reference (HG:537,560), at every size: the device writes
    the CSR arrays directly (hpf_jacobian_csr_last; 1.2 M entries at 1 000 buses x 26 harmonics).  return_jacobian=False skips it;
    J is None only when the loop took no iteration (the reference would raise NameError there, HG:560).  `details`, if a dict, receives err_hist, the pf seed, n_iter_f, solver name and device stats.
    `extra_iters` (not in the reference, default 0 = the reference's behaviour): Newton iterations taken AFTER the stop rule.
    The reference stops at err_h <= 1e-4, up to 4e-7 p.u. away from the fixed point, and where exactly below the
    threshold the last iterate lands depends on the rounding of the linear solver; one or two more iterations put the result on
    the fixed point itself, which does not (n_iter_h and err_h still report the reference's stop)."""
    if not (isinstance(update, str) and update in DeviceModel.UPDATES):
        raise ValueError("hpf: update=%r ('polar' or 'rectangular')" % (update,))
    st = settings or globals()["settings"]
    harmonics = st.HARMONICS
    n = len(buses)
    src = None
    if sources is not None:
        from .sweep import sources_argument
        if not isinstance(sources, dict):
            raise ValueError("hpf: sources=%r ({'currents': ..} or {'scale': .., 'shift': ..})" % (sources,))
        src = sources_argument({k: np.asarray(v)[None] for k, v in sources.items()}, 1, n - ingest.network_constants(buses)[0], len(harmonics), "hpf")
    Y = build_admittance_matrices(buses, lines, harmonics)                       # HG:523
    NE = import_Norton_Equivalents(buses, coupled, st, ne_dir)                    # HG:528
    with _borrow_model(buses, Y, NE, coupled, harmonics, solver=solver) as dm:
        dm.set_loads(buses["P"].to_numpy(dtype=float), buses["Q"].to_numpy(dtype=float))
        if src:
            dm.set_sources(src[1], src[0])
        dm.set_state(None, None, n_scen=1)
        nf, ef, hf = dm.fund_pf(st.thresh_f, st.max_iter_f)                       # HG:525 (pf with its defaults)
        seed = dm.get_state()
        if verbose:
            Vs = _frame(seed[0][0], seed[1][0], harmonics, n)
            print(Vs.loc[harmonics[0]])
            if int(nf[0]) < st.max_iter_f:
                print("Fundamental power flow converged after " + str(int(nf[0])) + " iterations.")
            else:
                print("Warning! Maximum of " + str(int(nf[0])) + " iterations reached.")
        # (block-tree: hpf_solve itself watches the static pivot order and repeats a flagged scenario with partial pivoting)
        want_J = bool(return_jacobian)
        dm.set_option("keep_previous_state", 1 if want_J else 0)      # (explicit both ways: the handle may be a borrowed one)
        dm.set_option("step_residual_check", 1 if check_steps else 0)  # (likewise)
        with dm.update_mode(update):
            n_iter, err, hist = dm.solve(thresh_h, max_iter_h)                    # HG:530-542
        stats = dm.stats()
        step_eta_max = float(dm.step_residuals()[1][0]) if check_steps else None
        # a meshed network on the block-tree path has no pivoted repeat of its own (hpf.h): with solver="auto" a scenario the static-pivot monitor
        # flagged, or whose mismatch turned non-finite, is solved again on the dense rocSOLVER path where that fits
        retry_dense = (solver == "auto" and dm.solver == "block_tree" and dm.tree_census()["ties"] > 0 and
                       bool(stats["flags"][0] & (4 | 8 | 64)) and not (stats["flags"][0] & 16) and 8.0 * dm.N * dm.N <= 64e9)
        if details is not None:
            details["repeated_with_pivoting"] = bool(stats["flags"][0] & 16)
            details["step_eta_max"] = step_eta_max                      # (None: check off; after a repeat: of the repeat)
            details["step_flagged"] = bool(stats["flags"][0] & 64)
        if verbose and (stats["flags"][0] & 16) and (stats["flags"][0] & 64):
            print("Warning! A Newton step missed the residual check; the solve was repeated with partial pivoting.")
        elif verbose and (stats["flags"][0] & 16):
            print("Warning! Static-pivot block elimination was flagged; the solve was repeated with partial pivoting.")
        if extra_iters > 0 and np.isfinite(err[0]):
            dm.mismatch(want_f=False)
            with dm.update_mode(update):
                dm.iterate(int(extra_iters))
                dm.sync()
        Vm_raw, Va_raw = dm.get_state()
        n_iter_h = int(n_iter[0])
        J = None
        if want_J and n_iter_h > 0:
            # the reference returns the Jacobian built in its last iteration, i.e. at the state before the last update: the solve
            # kept that state on the device
            J = dm.jacobian_csr(0, last=True)
        if details is not None:
            details.update(err_hist=hist[0, :n_iter_h + 1].copy(), seed=(seed[0][0].copy(), seed[1][0].copy()),
                           n_iter_f=int(nf[0]), err_f=hf[0, :int(nf[0])].copy(), solver=dm.solver,
                           tree=(dm.tree_census() if dm.solver == "block_tree" else None),
                           stats=stats, Vm_raw=Vm_raw[0].copy(), Va_raw=Va_raw[0].copy(), N=dm.N)
    if retry_dense:
        if verbose and (stats["flags"][0] & 64):
            print("Warning! A Newton step of the bordered block-tree path missed the residual check; solving again with the dense LU.")
        elif verbose:
            print("Warning! The bordered block-tree step was flagged (static pivot order / non-finite mismatch); solving again with the dense LU.")
        return hpf(buses, lines, coupled, thresh_h=thresh_h, max_iter_h=max_iter_h, plt_convergence=plt_convergence, settings=settings, ne_dir=ne_dir,
                   solver="dense", verbose=verbose, return_jacobian=return_jacobian, details=details, extra_iters=extra_iters,
                   check_steps=check_steps, update=update, sources=sources)
    Vm, Va = _postprocess(Vm_raw[0], Va_raw[0])                                   # HG:545-549
    V = _frame(Vm, Va, harmonics, n)
    err_h = float(err[0])
    if plt_convergence:
        import matplotlib.pyplot as plt
        plt.plot(range(n_iter_h), hist[0, 1:n_iter_h + 1])
    if verbose:
        print(V)
        if n_iter_h < max_iter_h:
            print("Harmonic power flow converged after " + str(n_iter_h) + " iterations.")
        elif n_iter_h == max_iter_h:
            print("Warning! Maximum of " + str(n_iter_h) + " iterations reached.")
    return V, err_h, n_iter_h, J


def _state_arrays(V):
    return (np.ascontiguousarray(V["V_m"].to_numpy(dtype=float)), np.ascontiguousarray(V["V_a"].to_numpy(dtype=float)))


def harmonic_mismatch(V, Y, buses, NE, settings=None):
    """HG:360-390 -> (f, err_h) for the voltages in DataFrame `V`."""
    st = settings or globals()["settings"]
    n = len(buses)
    harmonics = list(dict.fromkeys(V.index.get_level_values(0)))
    Y = _as_admittance(Y, harmonics, n)
    coupled = np.asarray(next(iter(NE.values()))[1]).shape[0] > 1 if NE else False
    with _borrow_model(buses, Y, NE, coupled, harmonics, solver="dense", assembly_only=True) as dm:
        dm.set_loads(buses["P"].to_numpy(dtype=float), buses["Q"].to_numpy(dtype=float))
        dm.set_state(*_state_arrays(V))
        f, err = dm.mismatch()
    return f[0], float(err[0])


def build_harmonic_jacobian(V, Y, NE, coupled, buses=None):
    """HG:401-473 -> real scipy CSR matrix in the reference's row/column order."""
    buses = buses if buses is not None else _ctx["buses"]
    if buses is None:
        raise ValueError("pass buses= or call init_network first (the reference reads the global `buses`)")
    n = len(buses)
    harmonics = list(dict.fromkeys(V.index.get_level_values(0)))
    Y = _as_admittance(Y, harmonics, n)
    with _borrow_model(buses, Y, NE, coupled, harmonics, solver="dense", assembly_only=True) as dm:
        dm.set_loads(buses["P"].to_numpy(dtype=float), buses["Q"].to_numpy(dtype=float))
        dm.set_state(*_state_arrays(V))
        J = dm.jacobian_csr(0)
    return J


def harmonic_state_vector(V, c=None, buses=None):
    """HG:393-398."""
    if c is None:
        b = buses if buses is not None else _ctx["buses"]
        c = ingest.network_constants(b)[2]
    return np.append(V.V_a.to_numpy()[1:], V.V_m.to_numpy()[c:])


def _dims_from_context(N):
    """(n, c, Hn) of the network the last init_network call loaded, if a Jacobian of N unknowns can belong to it (N = 2 n Hn - 1 - c)."""
    b = _ctx["buses"]
    if b is None:
        return None
    n = len(b)
    c = ingest.network_constants(b)[2]
    Hn, rem = divmod(N + 1 + c, 2 * n)
    return (n, c, Hn) if rem == 0 and Hn >= 1 else None


# update_harmonic_state_vec: the relative residual above which hpf_sparse_solve's result is not taken, and the largest dense N x N system
# (bytes) it hands to the dense LU instead
SPARSE_RESIDUAL_MAX = 1e-10
DENSE_FALLBACK_BYTES = 16e9


def _relative_residual(J, dx, f):
    """|f - J dx|_inf / (| |J| |_inf |dx|_inf + |f|_inf) of a CSR matrix, in float64."""
    r = np.abs(f - J @ dx).max() if f.size else 0.0
    den = float(abs(J).sum(axis=1).max()) * np.abs(dx).max() + np.abs(f).max()
    return float(r / den) if den > 0 else float(r)


def update_harmonic_state_vec(J, x, f, device=0, dims=None):
    """HG:476-479: x - spsolve(J, f), the linear solve on the GPU.

    J sparse (what `build_harmonic_jacobian` / `hpf` return, and what the reference passes, HG:478): `hpf_sparse_solve` -- the CSR entries are
    scattered on the device into bus-major 2Hn x 2Hn blocks and eliminated along the feeder tree; no N x N array exists on host or device, so the
    1 000-bus x 26-harmonic Jacobian (N = 51 998, 1.2 M entries) is solved like the 46-unknown one.  The row / column numbering of the reference's
    stacked matrix is a function of (n, c, Hn): taken from `dims=(n, c, Hn)`, else from the matrix itself (the Jacobians this package returns
    carry it), else from the network of the last `init_network` call.  A meshed network's Jacobian (spanning tree + loop-closing lines) takes the
    same route -- tree part factorised once, dense border system of the lines' endpoint buses.  hpf_sparse_solve pivots only inside a bus block,
    so its result is checked here: the relative residual |f - J dx|_inf / (| |J| |_inf |dx|_inf + |f|_inf) (float64, one host matvec) above
    SPARSE_RESIDUAL_MAX, or a bus block without a pivot (HPF_E_SINGULAR), sends the system to the dense LU with partial pivoting over the whole
    matrix -- where that fits DENSE_FALLBACK_BYTES, else a RuntimeError names the cause.  Dense arrays, and sparse matrices the sparse route
    refuses (bus graph not connected from bus 0, block pattern not symmetric, border beyond 16 384 unknowns), go to the dense rocSOLVER LU
    (`hpf_dense_solve`), which is bounded by 8 N^2 bytes of host and device memory (DENSE_FALLBACK_BYTES)."""
    lib = _lib.load()
    fv = np.ascontiguousarray(f, dtype=np.float64)
    N = fv.size
    dp = C.POINTER(C.c_double)
    if sp.issparse(J):
        if J.shape != (N, N):
            raise ValueError("J must be %d x %d" % (N, N))
        d = dims or getattr(J, "_hpf_dims", None) or _dims_from_context(N)
        if d is not None and 2 * d[0] * d[2] - 1 - d[1] == N and 2 * d[2] <= 128:
            Jc = J.tocsr()
            if Jc.nnz >= 2 ** 31:
                raise ValueError("hpf_sparse_solve takes 32-bit CSR indices (nnz < 2^31)")
            indptr = np.ascontiguousarray(Jc.indptr, dtype=np.int32)
            indices = np.ascontiguousarray(Jc.indices, dtype=np.int32)
            data = np.ascontiguousarray(Jc.data, dtype=np.float64)
            dx = np.empty(N)
            ip = C.POINTER(C.c_int32)
            rc = lib.hpf_sparse_solve(int(device), int(d[0]), int(d[1]), int(d[2]), indptr.ctypes.data_as(ip), indices.ctypes.data_as(ip),
                                      data.ctypes.data_as(dp), fv.ctypes.data_as(dp), dx.ctypes.data_as(dp))
            why = None
            if rc == 0:
                eta = _relative_residual(Jc, dx, fv)
                if eta <= SPARSE_RESIDUAL_MAX:
                    return np.asarray(x, dtype=np.float64) - dx
                why = "its result has a relative residual of %.1e (> %.0e): a near-singular bus block" % (eta, SPARSE_RESIDUAL_MAX)
            elif rc == 3:                                  # HPF_E_SINGULAR: a bus block (or the border system) without a pivot
                why = "a bus block without a pivot (HPF_E_SINGULAR)"
            elif rc != -3:                                 # (HPF_E_TOPOLOGY: a pattern the sparse route does not take -> the dense LU below)
                raise RuntimeError("hpf_sparse_solve failed: %s (code %d)" % (lib.hpf_strerror(rc).decode(), rc))
            if why is not None and 8.0 * N * N > DENSE_FALLBACK_BYTES:
                raise RuntimeError("update_harmonic_state_vec: hpf_sparse_solve met %s, and the dense LU that would solve it needs %.1f GB "
                                   "(limit %.1f GB)" % (why, 8e-9 * N * N, 1e-9 * DENSE_FALLBACK_BYTES))
        if 8.0 * N * N > DENSE_FALLBACK_BYTES:
            raise ValueError("update_harmonic_state_vec: a sparse Jacobian of %d unknowns %s; the dense fallback would need %.1f GB on the host -- "
                             "solve such a network with hpf() (bordered block-tree step)"
                             % (N, "that hpf_sparse_solve refuses (HPF_E_TOPOLOGY)" if d is not None else "whose (n, c, Hn) is unknown (pass dims=)", 8e-9 * N * N))
    Jd = np.asfortranarray(J.toarray() if hasattr(J, "toarray") else np.asarray(J), dtype=np.float64)
    if Jd.shape != (N, N):
        raise ValueError("J must be %d x %d" % (N, N))
    dx = np.empty(N)
    rc = lib.hpf_dense_solve(int(device), N, Jd.ctypes.data_as(dp), fv.ctypes.data_as(dp), dx.ctypes.data_as(dp))
    if rc != 0:
        raise RuntimeError("hpf_dense_solve failed: %s (code %d)" % (lib.hpf_strerror(rc).decode(), rc))
    return np.asarray(x, dtype=np.float64) - dx


def get_THD(V):
    """HG:563-572 -> DataFrame[THD_F, THD_R] per bus (harmonic labels >= 3 are the non-fundamental rows).  One pass over the [Hn][n]
    magnitudes; the per-bus sums run over the harmonics in ascending order like the reference's Python `sum` (HG:567-570), so the values
    are the reference's to the last bit."""
    harmonics = list(dict.fromkeys(V.index.get_level_values(0)))
    n = len(V) // len(harmonics)
    Vm = V["V_m"].to_numpy(dtype=float).reshape(len(harmonics), n)
    hs = np.zeros(n)
    for q in range(1, len(harmonics)):               # sequential over harmonics, vectorised over buses
        hs = hs + Vm[q] ** 2
    tot = Vm[0] ** 2
    for q in range(1, len(harmonics)):
        tot = tot + Vm[q] ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        thd_f = np.sqrt(hs) / Vm[0]
        thd_r = np.sqrt(hs) / np.sqrt(tot)
    return pd.DataFrame({"THD_F": thd_f, "THD_R": thd_r})


def line_branches(lines, br_from, br_to, n):
    """Map every row of `lines` (fromID, toID: 1-based bus IDs) to its branch -> (branch [L] int, sign [L] float): branch e = the stored pair
    (min, max) of the line's two buses (parallel lines share one: the matrix holds the last of them, HG:150-155), sign +1 where the line runs
    from the lower-numbered bus to the higher (the branch's own direction), -1 otherwise.  A line from a bus to itself has no branch: -1, NaN."""
    f = lines.fromID.to_numpy(dtype=np.int64) - 1
    t = lines.toID.to_numpy(dtype=np.int64) - 1
    key = np.minimum(f, t) * n + np.maximum(f, t)
    bkey = np.asarray(br_from, dtype=np.int64) * n + np.asarray(br_to, dtype=np.int64)      # ascending: CSR order
    e = np.minimum(np.searchsorted(bkey, key), max(len(bkey) - 1, 0))
    hit = (f != t) & (bkey[e] == key if len(bkey) else np.zeros(len(key), bool))
    return np.where(hit, e, -1), np.where(hit, np.where(f < t, 1.0, -1.0), np.nan)


def _line_results(V, lines, buses):
    """Branch flows of the voltage frame V on the GPU (a borrowed assembly-only handle, like harmonic_mismatch), mapped to the rows of `lines`
    -> harmonics, branch of every line, sign of every line, the flows dict, series admittances y [Hn][nb]."""
    n = len(buses)
    harmonics = list(dict.fromkeys(V.index.get_level_values(0)))
    Y = build_admittance_matrices(buses, lines, harmonics)
    with _borrow_model(buses, Y, None, False, harmonics, solver="dense", assembly_only=True) as dm:
        dm.set_state(*_state_arrays(V))
        fl = dm.branch_flows()
        br_from, br_to, ypos = dm.branches()
    e, sign = line_branches(lines, br_from, br_to, n)
    return harmonics, e, sign, fl, -Y.Yval[:, ypos]


def _take(a, e):
    """a [..., nb] at the branches e [L] (-1: NaN)"""
    out = np.full(a.shape[:-1] + (len(e),), np.nan, dtype=a.dtype)
    ok = e >= 0
    out[..., ok] = a[..., e[ok]]
    return out


def line_flows(V, lines, buses, settings=None):
    """Harmonic current and series loss of every line for the voltages in DataFrame `V` (not in the reference: its current_balance, HG:326-357,
    forms bus injections only) -> DataFrame indexed (harmonic, line) with fromID, toID, I_m, I_a (p.u. / rad, positive from the line's fromID to
    its toID) and loss (p.u., R |I|^2 with R = Re(1 / y) of the branch).  The currents are evaluated on the GPU (hpf_branch_flows); every row of
    `lines` is mapped to the branch of the admittance matrix that holds its bus pair, so parallel lines report the one line the matrix contains
    (HG:150-155)."""
    harmonics, e, sign, fl, y = _line_results(V, lines, buses)
    Ib = fl["I"][0]                                                     # [Hn][nb]
    with np.errstate(invalid="ignore", divide="ignore"):
        lb = np.where(np.abs(y) > 0, y.real / (y.real * y.real + y.imag * y.imag) * (Ib.real * Ib.real + Ib.imag * Ib.imag), 0.0)
    I = _take(Ib, e) * sign
    Hn = len(harmonics)
    idx = pd.MultiIndex.from_product([harmonics, lines.index.values], names=["harmonic", "line"])
    return pd.DataFrame({"fromID": np.tile(lines.fromID.to_numpy(), Hn), "toID": np.tile(lines.toID.to_numpy(), Hn),
                         "I_m": np.abs(I).reshape(-1), "I_a": np.angle(I).reshape(-1), "loss": _take(lb, e).reshape(-1)}, index=idx)


def line_summary(V, lines, buses, settings=None):
    """Per line of `lines` (same index) for the voltages in `V`: I_rms (RMS current over all harmonics, p.u.: the thermal loading), THD_I
    (harmonic over fundamental current; inf / NaN on a line without fundamental current), loss and loss_harm (series loss over all harmonics / over
    the harmonics above the fundamental, p.u.) -- the device's sums over ascending harmonics (hpf_branch_flows)."""
    harmonics, e, sign, fl, y = _line_results(V, lines, buses)
    return pd.DataFrame({"fromID": lines.fromID.to_numpy(), "toID": lines.toID.to_numpy(), "I_rms": _take(fl["irms"][0], e),
                         "THD_I": _take(fl["thd_i"][0], e), "loss": _take(fl["loss"][0], e), "loss_harm": _take(fl["loss_harm"][0], e)},
                        index=lines.index)


def waveforms(V, buses, harmonics=None, samples=1024, at=None):
    """Time-domain bus voltages of the voltage frame `V` over one fundamental period (not in the reference), evaluated on the GPU (hpf_waveform; a
    borrowed assembly-only handle whose admittance pattern is the diagonal alone: the waveforms need the voltages only) -> (table, v):
    table = DataFrame per bus (index = the "bus" level of V) with peak (largest |v| over the `samples` samples, p.u. of the nominal peak voltage),
    kpeak (its sample), crest (peak / rms; sqrt 2 for a pure sine) and slack (the continuous peak lies in [peak, peak + slack]);
    v = DataFrame [len(at)][samples] of the samples of the buses in `at` -- POSITIONS 0 .. n-1 in V's bus order; its rows carry the bus labels of
    those positions (None: no samples, v is None).
    harmonics: the orders of V's harmonic level (None: read from V); samples: a power of two, 64 .. 4096."""
    n = len(buses)
    harmonics = list(dict.fromkeys(V.index.get_level_values(0))) if harmonics is None else [int(h) for h in harmonics]
    Y = AdmittanceSet(np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.ones((len(harmonics), n), dtype=np.complex128), harmonics, n)
    with _borrow_model(buses, Y, None, False, harmonics, solver="dense", assembly_only=True) as dm:
        dm.set_state(*_state_arrays(V))
        w = dm.waveform(samples, at)
    labels = pd.Index(list(dict.fromkeys(V.index.get_level_values(1))), name="bus")          # the bus labels of V, like get_THD's rows
    table = pd.DataFrame({k: w[k][0] for k in ("peak", "kpeak", "crest", "slack")}, index=labels)
    v = None if w["v"] is None else pd.DataFrame(w["v"][0], index=labels[w["buses"]], columns=pd.Index(range(int(samples)), name="sample"))
    return table, v


class ImpedanceScan:
    """Result of `impedance_scan`: h [F] the grid; Z [F][n] complex driving-point impedances (None with full=False); Zt [F][len(transfer)][n] the
    transfer columns Z_ij of the buses in `transfer`; peak [n] = max over the grid of |Z_ii|, peak_h [n] the harmonic order of that peak
    (peak_index [n] its grid index)."""

    def __init__(self, h, Z, Zt, peak, peak_index, bus_ids, transfer):
        self.h, self.Z, self.Zt, self.peak, self.peak_index = h, Z, Zt, peak, peak_index
        self.peak_h = h[peak_index]
        self.bus_ids, self.transfer = bus_ids, transfer

    def _pos(self, bus):
        return self.bus_ids.index(int(bus))

    def resonances(self, bus, prominence=0.0):
        """Parallel resonances seen from `bus` (1-based ID): the strict local maxima of |Z_ii| along the grid, on the host from Z -> DataFrame
        (index = grid index; h, z_abs, prominence).  The prominence of a maximum is (peak - base) / peak, base = the larger of the two minima
        of |Z| between the maximum and the nearest higher grid point on either side (or the end of the grid); maxima below `prominence`
        are left out."""
        if self.Z is None:
            raise ValueError("resonances needs the full scan (full=True)")
        a = np.abs(self.Z[:, self._pos(bus)])
        rows = []
        for f in range(1, len(a) - 1):
            if not (a[f] > a[f - 1] and a[f] > a[f + 1]):
                continue
            base = 0.0
            for side in (a[:f][::-1], a[f + 1:]):
                higher = np.nonzero(side > a[f])[0]
                base = max(base, float(side[:higher[0]].min() if len(higher) else side.min()))
            prom = (a[f] - base) / a[f]
            if prom >= prominence:
                rows.append((f, self.h[f], a[f], prom))
        return pd.DataFrame([r[1:] for r in rows], index=pd.Index([r[0] for r in rows], name="index"), columns=["h", "z_abs", "prominence"])


def impedance_scan_arrays(model, h, y_extra=None, sel=(), chunk=0, full=True, device=0):
    """hpf_impedance_scan on the arrays of `admittance.line_model`: h [F] real orders, y_extra [F][n] complex or None, sel 0-based bus indices
    -> (code, Z or None, Zt, zpeak, fpeak); code 0 or 3 (HPF_E_SINGULAR: the outputs are written), any other code raises."""
    lib = _lib.load()
    n, F = int(model["n"]), len(h)
    h = np.ascontiguousarray(h, dtype=np.float64)
    sel = np.ascontiguousarray(sel, dtype=np.int32)
    arr = {k: np.ascontiguousarray(model[k], dtype=np.int32 if k in ("fr", "to") else np.float64) for k in ("fr", "to", "R", "X", "gsh", "bsh", "xsh")}
    ip, dp = _lib.c_int_p, _lib.c_dbl_p
    net = _lib.hpf_zscan_net(n, int(model["nb"]), arr["fr"].ctypes.data_as(ip), arr["to"].ctypes.data_as(ip),
                             *[arr[k].ctypes.data_as(dp) for k in ("R", "X", "gsh", "bsh", "xsh")])
    yx = None if y_extra is None else np.ascontiguousarray(y_extra, dtype=np.complex128)
    if yx is not None and yx.shape != (F, n):
        raise ValueError("y_extra must be [F][n]")
    Z = np.empty((F, n), dtype=np.complex128) if full else None
    Zt = np.empty((F, len(sel), n), dtype=np.complex128)
    zpeak, fpeak = np.empty(n), np.empty(n, dtype=np.int32)
    rc = lib.hpf_impedance_scan(int(device), C.byref(net), F, h.ctypes.data_as(dp), None if yx is None else yx.ctypes.data_as(dp), len(sel),
                                sel.ctypes.data_as(ip), int(chunk), None if Z is None else Z.ctypes.data_as(dp),
                                Zt.ctypes.data_as(dp) if len(sel) else None, zpeak.ctypes.data_as(dp), fpeak.ctypes.data_as(ip))
    if rc not in (0, 3):
        raise _lib.HpfError(rc, 0, "hpf_impedance_scan")
    return rc, Z, Zt, zpeak, fpeak


def impedance_scan(buses, lines, h, shunts=None, capacitors=None, transfer=None, full=True, device=0, settings=None, ne_dir=None, coupled=True):
    """Frequency scan of the network on the GPU (not in the reference): the driving-point impedance Z_ii(h) of every bus, and the transfer
    impedances Z_ij(h) to the buses in `transfer`, over the grid `h` of real harmonic orders > 0 -> ImpedanceScan.  The network is
    `admittance.line_model(buses, lines)`: the reference's admittance matrix (HG:147-170) at every h, never formed.
    capacitors={bus ID: b} adds the admittance j h b at that bus (b in p.u. at the fundamental); shunts: an [F][n] complex array of shunt
    admittances added as given, or "norton": every grid point must be one of settings.HARMONICS, and the (q, q) entry of the Norton admittance
    Y_N (uncoupled: entry q) of its device is added at every nonlinear bus (settings, ne_dir, coupled: as for hpf) -- ValueError otherwise.
    Bus arguments are the reference's 1-based IDs, as in line_flows.  A grid point at which some Z_ii is not finite (a network without any
    shunt at h = 1) leaves inf / NaN in the result."""
    model, h, ids, yx = _scan_network(buses, lines, h, shunts, capacitors, settings, ne_dir, coupled)
    transfer = [int(b) for b in (transfer or [])]
    sel = [ids.index(b) for b in transfer]
    _, Z, Zt, zpeak, fpeak = impedance_scan_arrays(model, h, yx, sel, 0, full, device)
    return ImpedanceScan(h, Z, Zt, zpeak, fpeak, ids, transfer)


def _norton_on_grid(buses, h, what, settings, ne_dir, coupled):
    """The Norton equivalents at the grid points of h, every one of which must be in settings.HARMONICS (ValueError otherwise; `what` names the
    argument) -> dev_of_bus [n], Y_N, I_N (ingest.norton_arrays), q [F] the position of every grid point in settings.HARMONICS"""
    st = settings or globals()["settings"]
    harmonics = list(st.HARMONICS)
    if any(x not in harmonics for x in h):
        raise ValueError("%s=\"norton\" needs every grid point in settings.HARMONICS" % what)
    q = np.array([harmonics.index(x) for x in h])
    NE = import_Norton_Equivalents(buses, coupled, st, ne_dir)
    dev, Y_N, I_N, _ = ingest.norton_arrays(buses, NE, coupled, len(harmonics))
    return dev, Y_N, I_N, q


def _scan_network(buses, lines, h, shunts, capacitors, settings, ne_dir, coupled):
    """What impedance_scan and penetration share: the line model, the grid as a float64 vector, the 1-based bus IDs in bus order and the shunt
    admittances y_extra [F][n] (or None) of `shunts` and `capacitors`"""
    model = admittance.line_model(buses, lines)
    n = model["n"]
    h = np.ascontiguousarray(h, dtype=np.float64).reshape(-1)
    F = len(h)
    ids = [int(b) for b in buses["ID"]] if "ID" in buses else list(range(1, n + 1))
    yx = None
    if isinstance(shunts, str):
        if shunts != "norton":
            raise ValueError("shunts must be an [F][n] array or \"norton\"")
        dev, Y_N, _, q = _norton_on_grid(buses, h, "shunts", settings, ne_dir, coupled)
        yx = np.zeros((F, n), dtype=np.complex128)
        for i in np.nonzero(dev >= 0)[0]:
            yx[:, i] = Y_N[dev[i], q, q] if coupled else Y_N[dev[i], q]
    elif shunts is not None:
        yx = np.array(shunts, dtype=np.complex128)
        if yx.shape != (F, n):
            raise ValueError("shunts must be [F][n] = [%d][%d]" % (F, n))
    if capacitors:
        yx = np.zeros((F, n), dtype=np.complex128) if yx is None else yx
        for bus, b in capacitors.items():
            yx[:, ids.index(int(bus))] += 1j * h * float(b)
    return model, h, ids, yx


class Penetration:
    """Result of `penetration`: h [F] the grid; V [S][F][n] complex bus voltages (None with full=False); rss [S][n] = sqrt(sum_f |V|^2) over the
    whole grid; over the S scenarios, per (grid point, bus): vmax [F][n] the largest |V|, varg [F][n] its scenario (ties: the smallest), vmean and
    vstd [F][n] of |V|; per bus: rss_max, rss_arg, rss_mean, rss_std [n] of rss.  bus_ids: the 1-based IDs of the n columns; at: those of the
    injecting buses."""

    def __init__(self, h, S, out, bus_ids, at):
        self.h, self.S, self.bus_ids, self.at = h, S, bus_ids, at
        self.V, self.rss = out["V"], out["rss"]
        for pre in ("v", "rss_"):
            setattr(self, pre + "max", out[pre + "max"])
            setattr(self, pre + "arg", out[pre + "arg"])
            mean = out[pre + "sum"] / S
            setattr(self, pre + "mean", mean)
            setattr(self, pre + "std", np.sqrt(np.maximum(out[pre + "sumsq"] / S - mean * mean, 0.0)))


PENETRATION_OUTPUTS = ("V", "rss", "vmax", "varg", "vsum", "vsumsq", "rss_max", "rss_arg", "rss_sum", "rss_sumsq")


def penetration_arrays(model, h, I, inj, y_extra=None, chunk_f=0, chunk_s=0, full=True, device=0):
    """hpf_penetration on the arrays of `admittance.line_model`: h [F] real orders, I [S][F][n_inj] complex currents injected at the 0-based bus
    indices inj, y_extra [F][n] complex or None -> (code, dict of the arrays PENETRATION_OUTPUTS; V is None with full=False); code 0 or 3
    (HPF_E_SINGULAR: the outputs are written), any other code raises."""
    lib = _lib.load()
    n, F = int(model["n"]), len(h)
    h = np.ascontiguousarray(h, dtype=np.float64)
    inj = np.ascontiguousarray(inj, dtype=np.int32).reshape(-1)
    I = np.ascontiguousarray(I, dtype=np.complex128)
    if I.ndim != 3 or I.shape[1:] != (F, len(inj)):
        raise ValueError("I must be [S][F][n_inj] = [S][%d][%d], got %s" % (F, len(inj), I.shape))
    S = I.shape[0]
    arr = {k: np.ascontiguousarray(model[k], dtype=np.int32 if k in ("fr", "to") else np.float64) for k in ("fr", "to", "R", "X", "gsh", "bsh", "xsh")}
    ip, dp = _lib.c_int_p, _lib.c_dbl_p
    net = _lib.hpf_zscan_net(n, int(model["nb"]), arr["fr"].ctypes.data_as(ip), arr["to"].ctypes.data_as(ip),
                             *[arr[k].ctypes.data_as(dp) for k in ("R", "X", "gsh", "bsh", "xsh")])
    yx = None if y_extra is None else np.ascontiguousarray(y_extra, dtype=np.complex128)
    if yx is not None and yx.shape != (F, n):
        raise ValueError("y_extra must be [F][n]")
    out = {"V": np.empty((S, F, n), dtype=np.complex128) if full else None, "rss": np.empty((S, n))}
    for pre, shape in (("v", (F, n)), ("rss_", (n,))):
        out.update({pre + "max": np.empty(shape), pre + "arg": np.empty(shape, dtype=np.int32), pre + "sum": np.empty(shape),
                    pre + "sumsq": np.empty(shape)})
    ptrs = [None if out[k] is None else out[k].ctypes.data_as(ip if k.endswith("arg") else dp) for k in PENETRATION_OUTPUTS]
    rc = lib.hpf_penetration(int(device), C.byref(net), F, h.ctypes.data_as(dp), None if yx is None else yx.ctypes.data_as(dp), S, len(inj),
                             inj.ctypes.data_as(ip), I.ctypes.data_as(dp), int(chunk_f), int(chunk_s), *ptrs)
    if rc not in (0, 3):
        raise _lib.HpfError(rc, 0, "hpf_penetration")
    return rc, out


def penetration(buses, lines, h, currents, at=None, shunts=None, capacitors=None, sources=None, full=True, device=0, settings=None, ne_dir=None,
                coupled=True):
    """Harmonic penetration on the GPU (the "current injection method"; not in the reference): the bus voltages V(h) = Y(h)^-1 I(h) that S
    scenarios of injected harmonic currents produce over the grid `h` of real harmonic orders > 0, with statistics over the scenarios
    -> Penetration.  The network, `shunts` and `capacitors` are those of impedance_scan (shunts="norton" makes the Norton admittances part of
    Y(h): the harmonic part of an uncoupled Norton model is then exactly this linear solve).
    currents: [S][F][len(at)] complex, or [F][len(at)] for one scenario -- the current injected INTO the network at the buses `at` (1-based IDs,
    each once), p.u.; or "norton": I_N[dev(i)][q] of its device, as stored, at every nonlinear bus (`at` must be None, every grid point one of
    settings.HARMONICS; settings, ne_dir, coupled: as for hpf).  With currents="norton", sources={"scale": a, "shift": phi} ([S][n - m], either
    may be missing: 1 / 0) makes S scenarios of a units of each bus's device, their waveform shifted in time by phi rad at the fundamental:
    I = a e^(j h phi) I_N, expanded on the host (sweep.source_currents).  A grid point at which Y(h) is singular leaves inf / NaN in the result."""
    model, h, ids, yx = _scan_network(buses, lines, h, shunts, capacitors, settings, ne_dir, coupled)
    F = len(h)
    if isinstance(currents, str):
        if currents != "norton" or at is not None:
            raise ValueError("currents must be an array with the bus IDs `at`, or \"norton\" with at=None")
        dev, _, I_N, q = _norton_on_grid(buses, h, "currents", settings, ne_dir, coupled)
        inj = np.nonzero(dev >= 0)[0]
        I_bus = I_N[dev[inj]][:, q]                           # [n - m][F]
        if sources is None:
            I = np.ascontiguousarray(I_bus.T)[None]
        else:
            if not isinstance(sources, dict) or not sources or not set(sources) <= {"scale", "shift"}:
                raise ValueError("penetration: sources=%r ({'scale': .., 'shift': ..})" % (sources,))
            from .sweep import source_currents, sources_argument
            S = len(next(iter(sources.values())))
            _, ab = sources_argument(sources, S, len(inj), F, "penetration")
            I = np.ascontiguousarray(source_currents(I_bus, ab[:, :, 0], ab[:, :, 1], h).transpose(0, 2, 1))
    else:
        if sources is not None:
            raise ValueError("penetration: sources needs currents=\"norton\"")
        if at is None:
            raise ValueError("penetration: currents as an array needs the bus IDs `at`")
        inj = np.array([ids.index(int(b)) for b in at], dtype=np.int32)
        I = np.asarray(currents, dtype=np.complex128)
        I = I[None] if I.ndim == 2 else I
        if I.ndim != 3 or I.shape[1:] != (F, len(inj)):
            raise ValueError("currents must be [S][F][len(at)] = [S][%d][%d] (or [F][len(at)]), got %s" % (F, len(inj), I.shape))
    _, out = penetration_arrays(model, h, I, inj, yx, 0, 0, full, device)
    return Penetration(h, I.shape[0], out, ids, [ids[i] for i in inj])


class ResonanceModes:
    """Result of `resonance_modes`: h [F] the grid; per grid point lam [F] complex the eigenvalue of Y(h) of smallest modulus, zm [F] its modal
    impedance 1 / |lam|, residual [F] the relative residual of the returned eigenpair, top [F] the 1-based ID of the bus with the largest
    participation; pf [F][n] complex participation factors (sum over the buses = 1; None with full=False).  bus_ids: the IDs of the n columns."""

    def __init__(self, h, out, bus_ids):
        self.h, self.bus_ids = h, bus_ids
        self.lam, self.zm, self.residual, self.pf = out["lam"], out["zm"], out["res"], out["pf"]
        self.top = np.array(bus_ids)[out["top"]]

    def converged(self, tol=1e-8):
        """Mask [F] of the grid points whose eigenpair is resolved: residual <= tol (a NaN is not).  32 steps leave 2e-10 or less where the two
        smallest eigenvalues are a factor of two apart; a point where two modes cross stays above any tolerance."""
        return self.residual <= tol

    def modes(self, prominence=0.0, tol=1e-8):
        """The resonances of the network: the strict local maxima of zm along the grid among the converged points, on the host -> DataFrame
        (index = grid index; h, zm, top = the bus ID of the largest participation, pf_top = its |pf|, bus1 .. bus5 = the IDs of the five buses of
        largest |pf|, descending; prominence).  Prominence as in ImpedanceScan.resonances: (peak - base) / peak, base = the larger of the two minima
        of zm between the maximum and the nearest higher converged point on either side (or the end of the grid); maxima below `prominence` are
        left out."""
        if self.pf is None:
            raise ValueError("modes needs the participation factors (full=True)")
        idx = np.nonzero(self.converged(tol))[0]
        a = self.zm[idx]
        nb = min(5, len(self.bus_ids))
        rows = []
        for q in range(1, len(a) - 1):
            if not (a[q] > a[q - 1] and a[q] > a[q + 1]):
                continue
            base = 0.0
            for side in (a[:q][::-1], a[q + 1:]):
                higher = np.nonzero(side > a[q])[0]
                base = max(base, float(side[:higher[0]].min() if len(higher) else side.min()))
            prom = (a[q] - base) / a[q]
            if prom >= prominence:
                f = int(idx[q])
                mag = np.abs(self.pf[f])
                order = np.argsort(-mag, kind="stable")[:nb]
                rows.append((f, self.h[f], a[q], int(self.top[f]), float(mag[self.bus_ids.index(int(self.top[f]))])) +
                            tuple(self.bus_ids[i] for i in order) + (prom,))
        cols = ["h", "zm", "top", "pf_top"] + ["bus%d" % (j + 1) for j in range(nb)] + ["prominence"]
        return pd.DataFrame([r[1:] for r in rows], index=pd.Index([r[0] for r in rows], name="index"), columns=cols)


RESONANCE_OUTPUTS = ("lam", "zm", "res", "top", "pf")


def resonance_modes_arrays(model, h, y_extra=None, iters=32, chunk=0, full=True, device=0):
    """hpf_resonance_modes on the arrays of `admittance.line_model`: h [F] real orders, y_extra [F][n] complex or None, iters steps of inverse
    iteration -> (code, lam, zm, res, top (0-based), pf or None); code 0 or 3 (HPF_E_SINGULAR: the outputs are written), any other code raises."""
    lib = _lib.load()
    n, F = int(model["n"]), len(h)
    h = np.ascontiguousarray(h, dtype=np.float64)
    arr = {k: np.ascontiguousarray(model[k], dtype=np.int32 if k in ("fr", "to") else np.float64) for k in ("fr", "to", "R", "X", "gsh", "bsh", "xsh")}
    ip, dp = _lib.c_int_p, _lib.c_dbl_p
    net = _lib.hpf_zscan_net(n, int(model["nb"]), arr["fr"].ctypes.data_as(ip), arr["to"].ctypes.data_as(ip),
                             *[arr[k].ctypes.data_as(dp) for k in ("R", "X", "gsh", "bsh", "xsh")])
    yx = None if y_extra is None else np.ascontiguousarray(y_extra, dtype=np.complex128)
    if yx is not None and yx.shape != (F, n):
        raise ValueError("y_extra must be [F][n]")
    lam, zm, res, top = np.empty(F, dtype=np.complex128), np.empty(F), np.empty(F), np.empty(F, dtype=np.int32)
    pf = np.empty((F, n), dtype=np.complex128) if full else None
    rc = lib.hpf_resonance_modes(int(device), C.byref(net), F, h.ctypes.data_as(dp), None if yx is None else yx.ctypes.data_as(dp), int(iters),
                                 int(chunk), lam.ctypes.data_as(dp), zm.ctypes.data_as(dp), res.ctypes.data_as(dp), top.ctypes.data_as(ip),
                                 None if pf is None else pf.ctypes.data_as(dp))
    if rc not in (0, 3):
        raise _lib.HpfError(rc, 0, "hpf_resonance_modes")
    return rc, lam, zm, res, top, pf


def resonance_modes(buses, lines, h, shunts=None, capacitors=None, iters=32, full=True, device=0, settings=None, ne_dir=None, coupled=True):
    """Resonance mode analysis on the GPU (not in the reference): at every point of the grid `h` of real harmonic orders > 0 the critical mode of
    the network -- the eigenvalue of Y(h) of smallest modulus, its modal impedance 1 / |lambda| and the participation factors of the buses
    -> ResonanceModes.  Where impedance_scan shows a peak in many |Z_ii| at once, this says that they are one mode and which buses excite and
    observe it most (where a filter has to go).  The network, `shunts` and `capacitors` are those of impedance_scan.  `iters` (1 .. 256) steps of
    inverse iteration run at every point, nothing is adapted: ResonanceModes.converged tells the resolved points (two modes that cross at a grid
    point are not); only the critical mode of a point is returned.  A grid point at which Y(h) is singular leaves inf / NaN in the result."""
    model, h, ids, yx = _scan_network(buses, lines, h, shunts, capacitors, settings, ne_dir, coupled)
    _, lam, zm, res, top, pf = resonance_modes_arrays(model, h, yx, iters, 0, full, device)
    return ResonanceModes(h, dict(lam=lam, zm=zm, res=res, top=top, pf=pf), ids)


def solve(filename_buses, filename_lines, coupled=True, settings=None, ne_dir=None, solver="auto", verbose=False, extra_iters=0,
          check_steps=False, line_flows=False, update="polar", sources=None, waveforms=False):
    """Convenience wrapper (= init_network + hpf + get_THD) -> dict(V, err_h, n_iter_h, THD, details).  check_steps, update, sources: see hpf.
    line_flows=True adds the keys "line_flows" and "line_summary" (the two functions of that name on the result); waveforms=True (or a number of
    samples) adds the key "waveforms": the per-bus table of the function of that name."""
    st = settings or globals()["settings"]
    buses, lines, m, n, c = init_network(filename_buses, filename_lines, settings=st)
    details = {}
    V, err_h, n_iter_h, J = hpf(buses, lines, coupled, st.thresh_h, st.max_iter_h, settings=st, ne_dir=ne_dir,
                                solver=solver, verbose=verbose, details=details, extra_iters=extra_iters, check_steps=check_steps,
                                update=update, sources=sources)
    # converged = the stop rule err_h <= thresh_h was met (flags bit 0) -- not "the loop ended": a NaN mismatch ends it too
    out = {"V": V, "err_h": err_h, "n_iter_h": n_iter_h, "THD": get_THD(V), "details": details,
           "converged": bool(details["stats"]["flags"][0] & 1)}
    if line_flows:
        out["line_flows"] = globals()["line_flows"](V, lines, buses, st)
        out["line_summary"] = line_summary(V, lines, buses, st)
    if waveforms:
        out["waveforms"] = globals()["waveforms"](V, buses, list(st.HARMONICS), 1024 if waveforms is True else int(waveforms))[0]
    return out
