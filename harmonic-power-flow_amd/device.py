"""`DeviceModel`: owner of one libhpf handle (one network x harmonic set x Norton data on one GPU) and the thin
NumPy-facing wrappers around the C ABI.  All heavy work happens in HIP kernels / rocSOLVER; this file only marshals
arrays."""
import ctypes as C

import numpy as np

from . import _lib


def _dp(a):
    return a.ctypes.data_as(_lib.c_dbl_p)


def _ip(a):
    return a.ctypes.data_as(_lib.c_int_p)


BLOCK_TREE_MAX_B = 112       # widest bus block 2 Hn of the block tree (7 register tiles of 16 rows: tree_build_into of hpf_tree_plan.hpp)


def is_radial(n, rowptr, col):
    """True if the admittance pattern is a tree spanning all buses (n-1 undirected edges, connected from bus 0)."""
    nnz = len(col)
    if nnz != n + 2 * (n - 1):
        return False
    seen = np.zeros(n, dtype=bool)
    seen[0] = True
    stack = [0]
    while stack:
        i = stack.pop()
        for j in col[rowptr[i]:rowptr[i + 1]]:
            if not seen[j]:
                seen[j] = True
                stack.append(int(j))
    return bool(seen.all())


def device_memory():
    """-> (blocks, bytes) of device memory the library holds right now, over every handle of the process (hpf_debug_device_memory: the library's
    own bookkeeping, exact and independent of what else runs on the device -- 0, 0 once every handle is closed)."""
    blocks, nbytes = C.c_int64(), C.c_int64()
    _lib.load().hpf_debug_device_memory(C.byref(blocks), C.byref(nbytes))
    return int(blocks.value), int(nbytes.value)


class DeviceModel:
    """One libhpf handle of capacity `max_scenarios`.  The capacity is NOT a build parameter of the block tree (it was in rounds 3-4): every
    handle eliminates the Gauss-Jordan skeleton with compress steps (fewer, wider elimination levels), so the Newton steps of a
    scenario -- and the iteration count of a solver-sensitive case -- are bit-identical in handles of any capacity and any batch size.  A sweep of
    several hundred LIVE scenarios runs 5 - 8 % faster per step without the steps: `options="HPF_COMPRESS=0"` (rounding-level different Newton
    steps, like every other tree-build switch).  `tree_census()["compress_steps"]` reports what a handle uses."""

    def __init__(self, n, m, c, harmonics, rowptr, col, Yval, dev_of_bus, Y_N, I_N, n_dev, coupled,
                 solver="auto", device=0, max_scenarios=1, assembly_only=False, options=None):
        """options: build switches of THIS handle, "HPF_LAZY=0 HPF_SLEAF=1 ..." (hpf_create_opts; include/hpf.h lists them).  The process
        environment is consulted for the same names only when HPF_ENV_SWITCHES=1 is set (A/B tooling, the test-suite)."""
        lib = _lib.load()
        self.lib = lib
        self.n, self.m, self.c = int(n), int(m), int(c)
        self.harmonics = list(harmonics)
        self.Hn = len(self.harmonics)
        self.coupled = bool(coupled)
        self.rowptr = np.ascontiguousarray(rowptr, dtype=np.int32)
        self.col = np.ascontiguousarray(col, dtype=np.int32)
        self.Yval = np.ascontiguousarray(Yval, dtype=np.complex128)
        self.dev_of_bus = np.ascontiguousarray(dev_of_bus, dtype=np.int32)
        self.Y_N = np.ascontiguousarray(Y_N, dtype=np.complex128)
        self.I_N = np.ascontiguousarray(I_N, dtype=np.complex128)
        N = 2 * self.n * self.Hn - 1 - self.c
        auto = solver == "auto"
        if solver == "auto":
            # radial feeders: block-tree elimination; meshed networks (spanning tree + loop-closing lines) of 32 buses and more: the block-tree
            # path's bordered step (tried first, dense if the library refuses the topology: border beyond 16 384 unknowns) -- 0.3 - 1.1 ms per
            # iteration where the dense LU takes 2 - 250 (tools/mesh_vs_dense.py: N = 478 ... 15 598; rounds 2 - 4 drew the line at N > 8 192);
            # smaller networks (the reference's net1 - net3): dense rocSOLVER LU
            if is_radial(self.n, self.rowptr, self.col):
                solver = "block_tree" if self.n >= 32 else "dense"
            else:
                solver = "block_tree_or_dense" if self.n >= 32 else "dense"
        if solver in ("block_tree", "block_tree_or_dense") and 2 * self.Hn > BLOCK_TREE_MAX_B:
            # bus blocks wider than the block tree's kernels take (tree_build_into; hpf_create answers HPF_E_ARG): "auto" goes to the dense GPU
            # path where the Jacobians fit, as it does for a meshed feeder the bordered step refuses; an explicit request is an error that
            # names the limit
            fits = assembly_only or 8 * N * N * int(max_scenarios) <= 240e9
            if not (auto and fits):
                raise ValueError("solver='block_tree': bus blocks of 2*Hn = %d rows (%d harmonics); the block tree takes 2*Hn <= %d%s"
                                 % (2 * self.Hn, self.Hn, BLOCK_TREE_MAX_B,
                                    (", and the dense path would need %.0f GB for the Jacobians of N = %d unknowns x %d scenarios"
                                     % (8e-9 * N * N * max_scenarios, N, max_scenarios)) if auto else "; solver='dense' has no such limit"))
            solver = "dense"
        self._solver_request = solver
        if solver == "block_tree_or_dense":
            solver = "block_tree"
        self.solver = solver
        # (assembly_only: a handle used for hpf_mismatch / hpf_jacobian_csr alone never allocates the dense Jacobian)
        if solver == "dense" and not assembly_only and 8 * N * N * int(max_scenarios) > 240e9:
            raise ValueError("dense solver: N = %d unknowns x %d scenarios need %.0f GB for the Jacobians alone; radial feeders and feeders "
                             "with loop-closing lines of this size use solver='block_tree'" % (N, max_scenarios, 8e-9 * N * N * max_scenarios))
        d = _lib.hpf_desc()
        d.n, d.m, d.c, d.Hn, d.nnz = self.n, self.m, self.c, self.Hn, len(self.col)
        d.n_dev, d.coupled = int(n_dev), int(self.coupled)
        d.solver = {"dense": _lib.SOLVER_DENSE, "block_tree": _lib.SOLVER_BLOCK_TREE}[solver]
        d.device, d.max_scenarios = int(device), int(max_scenarios)
        d.rowptr, d.col = _ip(self.rowptr), _ip(self.col)
        d.Yval = self.Yval.view(np.float64).ctypes.data_as(_lib.c_dbl_p)
        d.dev_of_bus = _ip(self.dev_of_bus)
        d.Y_N = self.Y_N.view(np.float64).ctypes.data_as(_lib.c_dbl_p)
        d.I_N = self.I_N.view(np.float64).ctypes.data_as(_lib.c_dbl_p)
        self._h = C.c_void_p()
        opts = options.encode() if options else None
        rc = lib.hpf_create_opts(C.byref(self._h), C.byref(d), opts)
        if rc == -3 and self._solver_request == "block_tree_or_dense" and 8 * N * N * int(max_scenarios) <= 240e9:
            # too many loop-closing lines for the bordered block-tree step: the dense GPU path (still no CPU path anywhere)
            self.solver = "dense"
            d.solver = _lib.SOLVER_DENSE
            rc = lib.hpf_create_opts(C.byref(self._h), C.byref(d), opts)
        _lib.check(rc, None, "hpf_create")
        self.S_max = int(lib.hpf_max_scenarios(self._h))
        self.N = lib.hpf_num_unknowns(self._h)
        self.Nf = lib.hpf_num_unknowns_fund(self._h)
        self.n_levels = lib.hpf_tree_levels(self._h)
        self.n_depths = lib.hpf_tree_depths(self._h)

    # -- lifetime ------------------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self.lib.hpf_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, code, where):
        _lib.check(code, self._h, where)

    @property
    def S(self):
        """Scenarios of the current batch -- asked from the library (hpf_num_scenarios), never mirrored here: the per-batch entry points of the
        C ABI write exactly that many rows, so every output array below is sized from it (a host-side copy that disagreed with the library's
        count was a heap overrun in round 4, DESIGN_LOG.md)."""
        return int(self.lib.hpf_num_scenarios(self._h)) if getattr(self, "_h", None) else 0

    def _batch(self, where):
        S = self.S
        if S < 1:
            raise _lib.HpfError(-2, 0, where)          # HPF_E_STATE: no batch in the handle (fresh handle, or after solve_queue)
        return S

    # -- state ---------------------------------------------------------------------------------------------
    def set_loads(self, P, Q):
        P = np.ascontiguousarray(np.atleast_2d(P), dtype=np.float64)
        Q = np.ascontiguousarray(np.atleast_2d(Q), dtype=np.float64)
        assert P.shape == Q.shape and P.shape[1] == self.n
        self._chk(self.lib.hpf_set_loads(self._h, P.shape[0], _dp(P), _dp(Q)), "hpf_set_loads")

    def set_state(self, Vm=None, Va=None, n_scen=None):
        if Vm is None:
            S = n_scen or self.S or 1
            self._chk(self.lib.hpf_set_state(self._h, S, None, None), "hpf_set_state")
            return
        Vm = np.ascontiguousarray(np.atleast_2d(Vm), dtype=np.float64)
        Va = np.ascontiguousarray(np.atleast_2d(Va), dtype=np.float64)
        assert Vm.shape == Va.shape and Vm.shape[1] == self.n * self.Hn
        self._chk(self.lib.hpf_set_state(self._h, Vm.shape[0], _dp(Vm), _dp(Va)), "hpf_set_state")

    def get_state(self):
        Vm = np.empty((self._batch("hpf_get_state"), self.n * self.Hn))
        Va = np.empty_like(Vm)
        self._chk(self.lib.hpf_get_state(self._h, _dp(Vm), _dp(Va)), "hpf_get_state")
        return Vm, Va

    # -- start state (hpf_start_*) ---------------------------------------------------------------------------
    def set_start(self, Vm, Va):
        """The handle's start state from host arrays [Hn*n] (stacked order, raw as get_state returns them): while it is set, every scenario of
        solve_queue begins there instead of at the reference's flat start + pf (include/hpf.h, "Start state")."""
        Vm = np.ascontiguousarray(Vm, dtype=np.float64).reshape(-1)
        Va = np.ascontiguousarray(Va, dtype=np.float64).reshape(-1)
        assert Vm.shape == Va.shape == (self.n * self.Hn,)
        self._chk(self.lib.hpf_start_set(self._h, _dp(Vm), _dp(Va)), "hpf_start_set")

    def capture_start(self, scen=0):
        """The start state from scenario `scen` of the current batch (after solve()), device to device."""
        self._chk(self.lib.hpf_start_capture(self._h, int(scen)), "hpf_start_capture")

    def get_start(self):
        """-> (Vm, Va) [Hn*n] of the start state; HPF_E_STATE when none is set."""
        Vm = np.empty(self.n * self.Hn)
        Va = np.empty_like(Vm)
        self._chk(self.lib.hpf_start_get(self._h, _dp(Vm), _dp(Va)), "hpf_start_get")
        return Vm, Va

    def has_start(self):
        """True while the handle holds a start state (hpf_start_get answers HPF_E_STATE without one, before any device call)."""
        try:
            self.get_start()
        except _lib.HpfError as e:
            if e.code != -2:
                raise
            return False
        return True

    def clear_start(self):
        self._chk(self.lib.hpf_start_clear(self._h), "hpf_start_clear")

    def apply_start(self, n_scen):
        """set_state of the start state tiled to n_scen scenarios, on the device; solve() then marks the records with flags bit 8."""
        self._chk(self.lib.hpf_start_apply(self._h, int(n_scen)), "hpf_start_apply")

    # -- per-scenario source currents (hpf_set_sources / hpf_queue_sources) ----------------------------------
    SOURCE_FORMS = {"currents": _lib.SRC_CURRENTS, "scale_shift": _lib.SRC_SCALE_SHIFT}

    def _sources_args(self, data, form, where):
        """(n_scen, form code, float64 array, orders) for the C ABI.  form="currents": data [S][n-m][Hn] complex; "scale_shift": data [S][n-m][2]
        = (a, phi) per scenario and nonlinear bus (a 2-D array is one scenario).  ValueError for another form or shape, before any device call."""
        if not (isinstance(form, str) and form in self.SOURCE_FORMS):
            raise ValueError("%s: form=%r ('currents' or 'scale_shift')" % (where, form))
        nnl = self.n - self.m
        if form == "currents":
            a = np.ascontiguousarray(data, dtype=np.complex128)
            tail = (nnl, self.Hn)
        else:
            a = np.ascontiguousarray(data, dtype=np.float64)
            tail = (nnl, 2)
        if a.ndim == 2:
            a = a[None]
        if a.ndim != 3 or a.shape[1:] != tail or a.shape[0] < 1:
            raise ValueError("%s: form %r takes an array [n_scen][%d][%d], got %s" % (where, form, tail[0], tail[1], a.shape))
        return a.shape[0], self.SOURCE_FORMS[form], np.ascontiguousarray(a).view(np.float64), np.ascontiguousarray(self.harmonics, dtype=np.int32)

    def set_sources(self, data, form="currents"):
        """Norton source currents of the current batch (after set_loads; include/hpf.h "Source currents"): scenario s forms the current balance of
        nonlinear bus i with I_src[s][i-m][q] in place of the model's I_N.  form="currents": data = I_src [S][n-m][Hn] complex, p.u.;
        form="scale_shift": data [S][n-m][2] = (a, phi): a units of the bus's device, shifted in time by phi rad at the fundamental (harmonic h
        rotates by h phi; the orders are self.harmonics), expanded on the device.  set_loads drops them."""
        S, code, a, orders = self._sources_args(data, form, "set_sources")
        self._chk(self.lib.hpf_set_sources(self._h, S, code, _dp(a), _ip(orders)), "hpf_set_sources")

    def get_sources(self):
        """-> I_src [S][n-m][Hn] complex as the device holds them; HPF_E_STATE when the batch has none (never set, cleared, or after set_loads)."""
        out = np.empty((self._batch("hpf_get_sources"), self.n - self.m, self.Hn), dtype=np.complex128)
        self._chk(self.lib.hpf_get_sources(self._h, out.view(np.float64).ctypes.data_as(_lib.c_dbl_p)), "hpf_get_sources")
        return out

    def clear_sources(self):
        self._chk(self.lib.hpf_clear_sources(self._h), "hpf_clear_sources")

    def queue_sources(self, data, form="currents"):
        """The sources of the NEXT solve_queue call, one row per scenario of its P, Q (forms as set_sources); a call with another number of
        scenarios is refused (HPF_E_ARG) and the registration dropped."""
        S, code, a, orders = self._sources_args(data, form, "queue_sources")
        self._chk(self.lib.hpf_queue_sources(self._h, S, code, _dp(a), _ip(orders)), "hpf_queue_sources")

    # -- kernels -------------------------------------------------------------------------------------------
    def mismatch(self, fund=False, want_f=True):
        N = self.Nf if fund else self.N
        S = self._batch("hpf_mismatch")
        f = np.empty((S, N)) if want_f else None
        err = np.empty(S)
        fn = self.lib.hpf_fund_mismatch if fund else self.lib.hpf_mismatch
        self._chk(fn(self._h, _dp(f) if want_f else None, _dp(err)), "hpf_mismatch")
        return f, err

    def jacobian(self, scen=0, fund=False):
        N = self.Nf if fund else self.N
        J = np.empty((N, N), order="F")
        fn = self.lib.hpf_fund_jacobian if fund else self.lib.hpf_jacobian
        self._chk(fn(self._h, int(scen), J.ctypes.data_as(_lib.c_dbl_p)), "hpf_jacobian")
        return J

    def jacobian_last(self, scen=0):
        """Jacobian of the last iteration of the last solve (HG:537,560); needs set_option("keep_previous_state", 1) before it."""
        J = np.empty((self.N, self.N), order="F")
        self._chk(self.lib.hpf_jacobian_last(self._h, int(scen), J.ctypes.data_as(_lib.c_dbl_p)), "hpf_jacobian_last")
        return J

    def jacobian_nnz(self):
        nnz = C.c_int64()
        self._chk(self.lib.hpf_jacobian_nnz(self._h, C.byref(nnz)), "hpf_jacobian_nnz")
        return int(nnz.value)

    def jacobian_csr(self, scen=0, last=False):
        """build_harmonic_jacobian (HG:401-473) as the reference returns it: scipy CSR of the stacked real matrix (HG:469-472), assembled
        on the device straight into the CSR arrays (hpf_jacobian_csr; no dense N x N).  last=True: at the state the scenario's last
        Newton step started from (what hpf() returns, HG:537,560; needs set_option("keep_previous_state", 1) before the solve)."""
        import scipy.sparse as sp
        nnz = self.jacobian_nnz()
        indptr = np.empty(self.N + 1, dtype=np.int32)
        indices = np.empty(nnz, dtype=np.int32)
        data = np.empty(nnz, dtype=np.float64)
        fn = self.lib.hpf_jacobian_csr_last if last else self.lib.hpf_jacobian_csr
        self._chk(fn(self._h, int(scen), _ip(indptr), _ip(indices), _dp(data)), "hpf_jacobian_csr")
        J = sp.csr_matrix((data, indices, indptr), shape=(self.N, self.N))
        J._hpf_dims = (self.n, self.c, self.Hn)        # the numbering of its rows / columns (api.update_harmonic_state_vec reads it)
        return J

    def fund_pf(self, thresh=1e-6, max_iter=30):
        S = self._batch("hpf_fund_pf")
        n_iter = np.zeros(S, dtype=np.int32)
        err = np.empty(S)
        hist = np.empty((S, max(max_iter, 1)))
        self._chk(self.lib.hpf_fund_pf(self._h, float(thresh), int(max_iter), _ip(n_iter), _dp(err), _dp(hist)),
                  "hpf_fund_pf")
        return n_iter, err, hist[:, :max_iter]

    def solve(self, thresh=1e-4, max_iter=50, trace=False):
        """hpf_solve -> (n_iter [S], err [S], err_hist [S][max_iter+1]); with trace=True additionally the per-iteration states
        (Vm_traj, Va_traj) [S][max_iter+1][Hn*n] (entry k = state after iteration k; frozen scenarios repeat their last state)."""
        S = self._batch("hpf_solve")
        n_iter = np.zeros(S, dtype=np.int32)
        err = np.empty(S)
        hist = np.empty((S, max_iter + 1))
        if trace:
            Vt = np.full((S, max_iter + 1, self.n * self.Hn), np.nan)
            At = np.full_like(Vt, np.nan)
            self._chk(self.lib.hpf_set_trace(self._h, _dp(Vt), _dp(At), max_iter + 1), "hpf_set_trace")
        try:
            self._chk(self.lib.hpf_solve(self._h, float(thresh), int(max_iter), _ip(n_iter), _dp(err), _dp(hist)),
                      "hpf_solve")
        finally:
            if trace:
                self.lib.hpf_set_trace(self._h, None, None, 0)
        if trace:
            return n_iter, err, hist, Vt, At
        return n_iter, err, hist

    def solve_queue(self, P, Q, thresh_f=1e-6, max_iter_f=30, thresh=1e-4, max_iter=50, want_voltages=False):
        """hpf_solve_queue: every row of P, Q [n_scen][n] is one scenario (reference start, pf, harmonic NR -- with a start state set: the start
        state, no pf, thresh_f / max_iter_f ignored, records with flags bit 8); the handle's S_max slots are
        refilled with pending scenarios as running ones meet the stop rule.  -> records (n_iter, flags, err, thd_max) [n_scen]
        [, raw Vm, Va [n_scen][Hn*n]].  Leaves the handle without a batch (set_loads / set_state before the per-batch calls)."""
        P = np.ascontiguousarray(np.atleast_2d(P), dtype=np.float64)
        Q = np.ascontiguousarray(np.atleast_2d(Q), dtype=np.float64)
        assert P.shape == Q.shape and P.shape[1] == self.n
        n_scen = P.shape[0]
        st = (_lib.hpf_stat * n_scen)()
        Vm = Va = None
        if want_voltages:
            Vm = np.empty((n_scen, self.n * self.Hn))
            Va = np.empty_like(Vm)
        self._chk(self.lib.hpf_solve_queue(self._h, n_scen, _dp(P), _dp(Q), float(thresh_f), int(max_iter_f), float(thresh), int(max_iter),
                                           st, _dp(Vm) if want_voltages else None, _dp(Va) if want_voltages else None), "hpf_solve_queue")
        rec = np.frombuffer(st, dtype=[("n_iter", "<i4"), ("flags", "<i4"), ("err", "<f8"), ("thd_max", "<f8")]).copy()
        return (rec, Vm, Va) if want_voltages else rec

    def iterate(self, iters):
        self._chk(self.lib.hpf_iterate(self._h, int(iters)), "hpf_iterate")

    def sync(self):
        self._chk(self.lib.hpf_sync(self._h), "hpf_sync")

    def stats(self):
        st = (_lib.hpf_stat * self._batch("hpf_get_stats"))()
        self._chk(self.lib.hpf_get_stats(self._h, st), "hpf_get_stats")
        return np.array([(s.n_iter, s.flags, s.err, s.thd_max) for s in st],
                        dtype=[("n_iter", "i4"), ("flags", "i4"), ("err", "f8"), ("thd_max", "f8")])

    def stats_to_device(self, data_ptr):
        self._chk(self.lib.hpf_get_stats_dev(self._h, C.c_void_p(int(data_ptr))), "hpf_get_stats_dev")

    def step_residuals(self):
        """(eta_last [S], eta_max [S]): normwise backward error of every scenario's last Newton step and the largest one of the solve
        (hpf_get_step_residuals; needs set_option("step_residual_check", 1); NaN where no step was taken)."""
        S = self._batch("hpf_get_step_residuals")
        last, big = np.empty(S), np.empty(S)
        self._chk(self.lib.hpf_get_step_residuals(self._h, _dp(last), _dp(big)), "hpf_get_step_residuals")
        return last, big

    # -- the three sweep accumulators: what their begin / get pairs share ---------------------------------------
    @staticmethod
    def _limits(values, count):
        """limit argument of an accumulator -> contiguous float64 [count], or None (no limits)"""
        lim = None if values is None else np.ascontiguousarray(values, dtype=np.float64)
        assert lim is None or lim.shape == (count,)
        return lim

    def _stats_get(self, cls, call, shapes, *settings):
        """zeroed arrays of cls.ARRAYS in `shapes` -> filled by the C call -> cls(*settings, **arrays)"""
        a = {name: np.zeros(shape, dtype=dt) for name, dt, shape in zip(cls.ARRAYS, cls.DTYPES, shapes)}
        self._chk(getattr(self.lib, call)(self._h, *[a[name].ctypes.data_as(C.c_void_p) for name in cls.ARRAYS]), call)
        return cls(*settings, **a)

    # -- distortion accumulator (hpf_distortion_*) ----------------------------------------------------------
    def distortion_begin(self, limit=None, thd_limit=np.inf, hist_max=1.0, bins=64):
        """Open (or reset) the handle's distortion accumulator: from now on every converged scenario hpf_solve_queue harvests, and every batch
        handed to distortion_add, is folded into per-bus / per-harmonic statistics on the device.  limit [Hn] (None: no limits): x_over counts
        the scenarios with x[q][i] > limit[q]; thd_limit likewise for THD; the THD histogram has `bins` (1..256) uniform bins on [0, hist_max)."""
        lim = self._limits(limit, self.Hn)
        self._chk(self.lib.hpf_distortion_begin(self._h, _dp(lim) if lim is not None else None, float(thd_limit), float(hist_max), int(bins)),
                  "hpf_distortion_begin")
        self._dist = (lim, float(thd_limit), float(hist_max), int(bins))

    def distortion_add(self, first_id=0):
        """Fold the current batch (after solve()) into the accumulator, scenario s under id first_id + s."""
        self._chk(self.lib.hpf_distortion_add(self._h, int(first_id)), "hpf_distortion_add")

    def distortion_get(self):
        """-> sweep.DistortionStats of everything added since distortion_begin (arrays in the ABI's order [Hn][n]); the accumulator stays open."""
        from .sweep import DistortionStats
        dist = getattr(self, "_dist", None) or (None, np.inf, 1.0, 1)
        shapes = ((3,),) + ((self.Hn, self.n),) * 5 + ((self.n,),) * 5 + ((self.n, dist[3] + 1),)
        return self._stats_get(DistortionStats, "hpf_distortion_get", shapes, self.harmonics, *dist[:3])

    def distortion_end(self):
        self._chk(self.lib.hpf_distortion_end(self._h), "hpf_distortion_end")
        self._dist = None

    # -- branch flows and branch statistics (hpf_branch_*) ---------------------------------------------------
    @property
    def nb(self):
        """Branches of the handle: stored pairs (i, j), i < j, of the admittance pattern (hpf_num_branches)."""
        return int(self.lib.hpf_num_branches(self._h))

    def branches(self):
        """-> (from [nb], to [nb], ypos [nb]) int32: the two buses of every branch (from < to) and the position of (from, to) in `col`."""
        out = [np.empty(self.nb, dtype=np.int32) for _ in range(3)]
        self._chk(self.lib.hpf_get_branches(self._h, *[_ip(a) for a in out]), "hpf_get_branches")
        return tuple(out)

    def branch_flows(self, want_I=True):
        """Series currents and losses of every branch at the handle's current state (after solve(), or after set_state() alone) -> dict:
        I [S][Hn][nb] complex (p.u., positive from the lower-numbered bus to the higher; None with want_I=False), irms, thd_i, loss, loss_harm
        [S][nb], loss_h [S][Hn] (include/hpf.h, hpf_branch_flows)."""
        S, nb = self._batch("hpf_branch_flows"), self.nb
        out = {"I": np.empty((S, self.Hn, nb), dtype=np.complex128) if want_I else None}
        for k in ("irms", "thd_i", "loss", "loss_harm"):
            out[k] = np.empty((S, nb))
        out["loss_h"] = np.empty((S, self.Hn))
        self._chk(self.lib.hpf_branch_flows(self._h, out["I"].view(np.float64).ctypes.data_as(_lib.c_dbl_p) if want_I else None,
                                            *[_dp(out[k]) for k in ("irms", "thd_i", "loss", "loss_harm", "loss_h")]), "hpf_branch_flows")
        return out

    def branch_stats_begin(self, rating=None):
        """Open (or reset) the handle's branch statistics: from now on every converged scenario hpf_solve_queue harvests, and every batch handed to
        branch_stats_add, is folded into per-branch statistics of irms, loss and harmonic loss on the device.  rating [nb] in p.u. (None: no
        ratings): irms_over counts the scenarios with irms[e] > rating[e]."""
        r = self._limits(rating, self.nb)
        self._chk(self.lib.hpf_branch_stats_begin(self._h, _dp(r) if r is not None else None), "hpf_branch_stats_begin")
        self._brating = r

    def branch_stats_add(self, first_id=0):
        """Fold the current batch (after solve()) into the branch statistics, scenario s under id first_id + s."""
        self._chk(self.lib.hpf_branch_stats_add(self._h, int(first_id)), "hpf_branch_stats_add")

    def branch_stats_get(self):
        """-> sweep.BranchStats of everything added since branch_stats_begin; the accumulator stays open."""
        from .sweep import BranchStats
        shapes = ((3,),) + ((self.nb,),) * (len(BranchStats.ARRAYS) - 1)
        return self._stats_get(BranchStats, "hpf_branch_stats_get", shapes, getattr(self, "_brating", None))

    def branch_stats_end(self):
        self._chk(self.lib.hpf_branch_stats_end(self._h), "hpf_branch_stats_end")
        self._brating = None

    # -- voltage waveforms and waveform statistics (hpf_waveform*) -------------------------------------------
    def _orders(self):
        return np.ascontiguousarray(self.harmonics, dtype=np.int32)

    def waveform(self, T=1024, buses=None):
        """Time-domain bus voltages over one fundamental period at the handle's current state (after solve(), or after set_state() alone), T samples
        (a power of two, 64..4096), orders = self.harmonics -> dict: peak, crest, slack [S][n] (p.u. of the nominal peak voltage; the continuous
        peak lies in [peak, peak + slack]), kpeak [S][n] int32 (sample of the peak), and for buses = a list of bus indices: buses, v [S][len][T]
        (None without it) (include/hpf.h, hpf_waveform)."""
        S = self._batch("hpf_waveform")
        sel = None if buses is None else np.ascontiguousarray(buses, dtype=np.int32).reshape(-1)
        out = {k: np.empty((S, self.n)) for k in ("peak", "crest", "slack")}
        out["kpeak"] = np.empty((S, self.n), dtype=np.int32)
        n_sel = 0 if sel is None else len(sel)
        out["buses"], out["v"] = sel, (np.empty((S, n_sel, max(int(T), 0))) if n_sel else None)
        self._chk(self.lib.hpf_waveform(self._h, _ip(self._orders()), int(T), n_sel, _ip(sel) if n_sel else None, _dp(out["v"]) if n_sel else None,
                                        _dp(out["peak"]), _ip(out["kpeak"]), _dp(out["crest"]), _dp(out["slack"])), "hpf_waveform")
        return out

    def waveform_stats_begin(self, T=1024, peak_limit=None, crest_limit=np.inf):
        """Open (or reset) the handle's waveform statistics: from now on every converged scenario hpf_solve_queue harvests, and every batch handed to
        waveform_stats_add, has the peak and the crest factor of every bus's voltage waveform (T samples per period) folded into per-bus statistics
        on the device.  peak_limit [n] in p.u. (None: no limits) and crest_limit: the `over` arrays count the scenarios strictly above them."""
        lim = self._limits(peak_limit, self.n)
        self._chk(self.lib.hpf_waveform_stats_begin(self._h, _ip(self._orders()), int(T), _dp(lim) if lim is not None else None, float(crest_limit)),
                  "hpf_waveform_stats_begin")
        self._wstat = (int(T), lim, float(crest_limit))

    def waveform_stats_add(self, first_id=0):
        """Fold the current batch (after solve()) into the waveform statistics, scenario s under id first_id + s."""
        self._chk(self.lib.hpf_waveform_stats_add(self._h, int(first_id)), "hpf_waveform_stats_add")

    def waveform_stats_get(self):
        """-> sweep.WaveformStats of everything added since waveform_stats_begin; the accumulator stays open."""
        from .sweep import WaveformStats
        shapes = ((3,),) + ((self.n,),) * (len(WaveformStats.ARRAYS) - 1)
        return self._stats_get(WaveformStats, "hpf_waveform_stats_get", shapes, *(getattr(self, "_wstat", None) or (0, None, np.inf)))

    def waveform_stats_end(self):
        self._chk(self.lib.hpf_waveform_stats_end(self._h), "hpf_waveform_stats_end")
        self._wstat = None

    def set_option(self, name, value):
        self._chk(self.lib.hpf_set_option(self._h, name.encode(), int(value)), "hpf_set_option")
        self.__dict__.setdefault("_options", {})[name] = int(value)

    UPDATES = ("polar", "rectangular")

    def update_mode(self, update):
        """Context manager: the handle's option "rectangular_update" set from update = "polar" | "rectangular" (ValueError for anything else)
        for the block, and put back to what it was on exit -- a cached handle never carries the mode into a later call."""
        import contextlib
        if not (isinstance(update, str) and update in self.UPDATES):
            raise ValueError("update=%r ('polar' or 'rectangular')" % (update,))

        @contextlib.contextmanager
        def scope():
            before = self.__dict__.get("_options", {}).get("rectangular_update", 0)
            self.set_option("rectangular_update", int(update == "rectangular"))
            try:
                yield self
            finally:
                self.set_option("rectangular_update", before)
        return scope()

    def set_stream(self, stream_ptr):
        self._chk(self.lib.hpf_set_stream(self._h, C.c_void_p(int(stream_ptr)) if stream_ptr else None),
                  "hpf_set_stream")

    def timing(self, on=True):
        self._chk(self.lib.hpf_timing_enable(self._h, int(on)), "hpf_timing_enable")

    def timing_reset(self):
        self._chk(self.lib.hpf_timing_reset(self._h), "hpf_timing_reset")

    def timing_get(self):
        out = {}
        for which, name in enumerate(("mismatch", "jacobian", "solve", "update", "back", "gj", "gj_dev", "step_residual")):
            ms = C.c_double()
            cnt = C.c_int64()
            self._chk(self.lib.hpf_timing_get(self._h, which, C.byref(ms), C.byref(cnt)), "hpf_timing_get")
            out[name] = (ms.value, cnt.value)
        return out

    def setup_times(self):
        """Milliseconds hpf_create spent: total, tree planning on the host, tree uploads, per-scenario allocation (hpf_setup_times)."""
        ms = (C.c_double * 4)()
        self._chk(self.lib.hpf_setup_times(self._h, ms, 4), "hpf_setup_times")
        return dict(zip(("create_ms", "tree_plan_ms", "tree_upload_ms", "alloc_ms"), (float(v) for v in ms)))

    def scenario_groups(self, live):
        """Scenario groups (streams) a step of `live` running scenarios is split into (hpf_scenario_groups)."""
        return int(self.lib.hpf_scenario_groups(self._h, int(live)))

    def solve_flops(self):
        return float(self.lib.hpf_solve_flops(self._h))

    def tree_census(self):
        """Which kernel takes which bus of the block tree (hpf_tree_census)."""
        out = (C.c_int32 * 19)()
        self._chk(self.lib.hpf_tree_census(self._h, out, 19), "hpf_tree_census")
        names = ("dense_buses", "gauss_jordan", "const_leaves", "lazy_leaves", "bordered", "nested_bordered", "levels", "depths", "ties",
                 "fused_levels", "compress_steps", "border_repivots", "border_unknowns", "root_path_buses", "bordered_form", "back_walks", "back_tails",
                 "batch_tile", "leaf_batch_tile")
        return dict(zip(names, (int(v) for v in out)))

    def solve_bytes(self):
        """Algorithmic HBM bytes of the linear-solve span of one scenario and one Newton step (hpf_solve_bytes)."""
        return float(self.lib.hpf_solve_bytes(self._h))

    def back_bytes(self):
        return float(self.lib.hpf_back_bytes(self._h))

    def kernel_model(self, which):
        """(algorithmic bytes, flops) of one kernel class per scenario and Newton step, launches per step and scenario group
        (hpf_kernel_model; which: "gj" = the general factor kernel k_factor_q<B,false>, "solve" = whole factor sweep, "back",
        "step_residual" = the residual check of a step)."""
        by, fl, ln = C.c_double(), C.c_double(), C.c_int32()
        idx = {"solve": 2, "back": 4, "gj": 5, "step_residual": 7}[which]
        self._chk(self.lib.hpf_kernel_model(self._h, idx, C.byref(by), C.byref(fl), C.byref(ln)), "hpf_kernel_model")
        return by.value, fl.value, ln.value
