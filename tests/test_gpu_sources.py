"""Per-scenario Norton source currents (hpf_set_sources / hpf_queue_sources, include/hpf.h "Source currents"; run with -m gpu on
an MI355X).

Shapes, the smallest that reach every path (as tests/test_gpu_warm_start.py): syn100 x harmonics to 11 -- Hn = 6, so rows q < 4 take the 4-group
body of the Norton product and q = 4, 5 the tail; tiles of 256 threads mix linear and nonlinear buses -- coupled and uncoupled; radial with
8 slots and 24 scenarios, so that slots refill; the same feeder with 2 loop-closing lines (meshed waves); net2 of the golden inputs (DENSE).
The scenarios are the ones of tests/test_sources_oracle.py (tests/sources_emul.py: a in [0.875, 1.125], phi in [-0.075, 0.075], the widest
ranges of that scan on which the ORACLE converges on all 24).

Two yardsticks, neither of them code of this feature: the unmodified CPU oracle on a network whose nonlinear buses each carry a component of
their own, and a handle built through api._device_model on that same per-bus network (I_N rows = I_src: the kernels without sources).

Bounds.  Bit for bit wherever the library promises it.  Form 1 on the device against sweep.source_currents: 6 * 2^-52 |a| |I_N[q]| per component
(derived in tests/test_sources_emul.py).  Against the oracle: both stop at thresh_h = 1e-9, |dU| <= 1e-8 p.u. is the project's fixed-point gate
(DESIGN.md 1).  Iteration counts are printed, not asserted."""
import numpy as np
import pytest

from conftest import INPUTS

import sources_emul as se

pytestmark = pytest.mark.gpu
TH = 1e-9
S_SCEN = se.S_SCEN
NONSUM_D = ("x_max", "x_arg", "x_over", "thd_max", "thd_arg", "thd_over", "thd_hist")
NONSUM_B = ("irms_max", "irms_arg", "irms_over", "loss_max", "loss_arg", "lossh_max", "lossh_arg")
RESOLVE_THRESH, RESOLVE_MAX_ITER = 5e-8, 3           # (test_the_re_solve_paths_carry_the_sources)


def _hp():
    import harmonic_power_flow_amd as hp
    return hp


def _net(kind, outdir, coupled=True):
    """-> dict: settings, files, buses, Y, NE, solver, the 24 scenarios (P, Q, a, phi, I_src by the host) and the oracle's description"""
    import os
    hp = _hp()
    from harmonic_power_flow_amd import synth, sweep
    st = hp.Settings(H_MAX=11)
    if kind == "dense":
        fb, fl = os.path.join(INPUTS, "net2_buses.csv"), os.path.join(INPUTS, "net2_lines.csv")
    else:
        fb, fl = synth.gen(100, seed=0, outdir=str(outdir))
        if kind == "meshed":
            synth.add_ties(fl, 100, 2)
    buses, lines, m, n, c = hp.init_network(fb, fl, settings=st)
    Y = hp.build_admittance_matrices(buses, lines, st.HARMONICS)
    NE = hp.import_Norton_Equivalents(buses, coupled, st, INPUTS)
    case = se.oracle_network(fb, fl, list(st.HARMONICS), coupled, INPUTS)
    scale = np.stack([synth.scenario_scale(n, s) for s in range(S_SCEN)])
    a, phi = se.scale_shift(n - m)
    return dict(st=st, buses=buses, Y=Y, NE=NE, coupled=coupled, solver="dense" if kind == "dense" else "block_tree", n=n, m=m,
                Hn=len(st.HARMONICS), P=buses["P"].to_numpy(float) * scale, Q=buses["Q"].to_numpy(float) * scale, scale=scale, a=a, phi=phi,
                ab=np.stack([a, phi], axis=2), I_src=sweep.source_currents(case["I_N_bus"], a, phi, st.HARMONICS), case=case)


def _model(net, slots, options=None):
    from harmonic_power_flow_amd import api
    return api._device_model(net["buses"], net["Y"], net["NE"], net["coupled"], net["st"].HARMONICS, solver=net["solver"], max_scenarios=slots,
                             options=options)


def _per_bus_model(net, I_src_s, slots=1):
    """the second yardstick: one device type per nonlinear bus, I_N = the scenario's I_src, Y_N of the bus's device -- no sources involved"""
    from harmonic_power_flow_amd import api
    buses = net["buses"].copy()
    comp = buses["component"].to_numpy().astype(object)
    NE = {}
    for i in range(net["m"], net["n"]):
        name = "source_bus_%d" % i
        NE[name] = (np.asarray(I_src_s[i - net["m"]]), net["NE"][comp[i]][1])
        comp[i] = name
    buses["component"] = comp
    return api._device_model(buses, net["Y"], NE, net["coupled"], net["st"].HARMONICS, solver=net["solver"], max_scenarios=slots)


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _U(res):
    return res[1] * np.exp(1j * res[2])


def _oracle_U(net):
    out = []
    for s in range(S_SCEN):
        r = se.oracle_solve(net["case"], net["scale"][s], net["I_src"][s], TH)
        assert r["err_h"] <= TH
        out.append((r["Vm_raw"] * np.exp(1j * r["Va_raw"]), r["n_iter_h"]))
    return np.stack([u for u, _ in out]), [k for _, k in out]


def _queue(net, slots, form="scale_shift", **options):
    dm = _model(net, slots)
    try:
        for k, v in options.items():
            dm.set_option(k, v)
        dm.queue_sources(net["ab"] if form == "scale_shift" else net["I_src"], form)
        return dm.solve_queue(net["P"], net["Q"], thresh=TH, want_voltages=True)
    finally:
        dm.close()


@pytest.fixture(scope="module")
def radial(tmp_path_factory):
    net = _net("radial", tmp_path_factory.mktemp("syn100"))
    net["queue"] = _queue(net, 8)
    net["U_oracle"], net["it_oracle"] = _oracle_U(net)
    return net


@pytest.fixture(scope="module")
def radial_uc(tmp_path_factory):
    return _net("radial", tmp_path_factory.mktemp("syn100uc"), coupled=False)


@pytest.fixture(scope="module")
def meshed(tmp_path_factory):
    return _net("meshed", tmp_path_factory.mktemp("syn100m"))


@pytest.fixture(scope="module")
def dense(tmp_path_factory):
    return _net("dense", tmp_path_factory.mktemp("net2"))


def _batch_run(dm, net, S):
    dm.set_state(None, None, n_scen=S)
    f, err = dm.mismatch()
    dm.fund_pf(1e-6, 30)
    dm.solve(TH, 50)
    return (f, err, dm.stats()) + dm.get_state()


def test_off_is_untouched(radial):
    """sources set and cleared, sources dropped by set_loads, and a handle that never had any: f, records and voltages bit for bit; get_sources
    without sources answers HPF_E_STATE"""
    net, S = radial, 5
    from harmonic_power_flow_amd import _lib
    res = []
    for variant in ("fresh", "cleared", "dropped"):
        dm = _model(net, 8)
        try:
            dm.set_loads(net["P"][:S], net["Q"][:S])
            if variant == "cleared":
                dm.set_sources(net["ab"][:S], "scale_shift")
                assert (dm.get_sources() != 0).any()
                dm.clear_sources()
                dm.clear_sources()                            # (already clear: HPF_OK)
            if variant == "dropped":
                dm.set_sources(net["I_src"][:S], "currents")
                dm.set_loads(net["P"][:S], net["Q"][:S])
            with pytest.raises(_lib.HpfError) as e:
                dm.get_sources()
            assert e.value.code == -2
            res.append(_batch_run(dm, net, S))
        finally:
            dm.close()
    assert _same(res[0], res[1]) and _same(res[0], res[2])
    assert not (res[0][2]["flags"] & 1024).any()


@pytest.mark.parametrize("kind", ["radial", "radial_uc", "dense"])
def test_mismatch_with_sources_is_the_mismatch_of_the_per_bus_device_handle(kind, request):
    """fails without the feature.  Flat state and a solved state (the per-bus handle's own solution), scenarios 0 and 1 as a batch of two"""
    net = request.getfixturevalue(kind)
    dm = _model(net, 2)
    try:
        dm.set_loads(net["P"][:2], net["Q"][:2])
        dm.set_sources(net["I_src"][:2], "currents")
        assert dm.get_sources().tobytes() == net["I_src"][:2].tobytes()
        for s in range(2):
            hb = _per_bus_model(net, net["I_src"][s])
            try:
                hb.set_loads(net["P"][s], net["Q"][s])
                hb.set_state(None, None, n_scen=1)
                states = [hb.get_state()]
                hb.fund_pf(1e-6, 30)
                hb.solve(TH, 50)
                assert hb.stats()["flags"][0] & 1
                states.append(hb.get_state())
                for Vm, Va in states:
                    hb.set_state(Vm, Va)
                    fb, eb = hb.mismatch()
                    dm.set_state(np.tile(Vm, (2, 1)), np.tile(Va, (2, 1)))
                    f, e = dm.mismatch()
                    assert f[s].tobytes() == fb[0].tobytes() and e[s] == eb[0], (kind, s)
            finally:
                hb.close()
        # the model's own currents as sources: the mismatch without sources
        Vm, Va = states[1]
        dm.set_sources(np.tile(net["case"]["I_N_bus"], (2, 1, 1)), "currents")
        f1, _ = dm.mismatch()
        dm.clear_sources()
        f0, _ = dm.mismatch()
        assert f1.tobytes() == f0.tobytes() and (f != f0).any()
    finally:
        dm.close()


def test_form_one_on_the_device(radial):
    net, S = radial, 8
    dm = _model(net, 8)
    try:
        dm.set_loads(net["P"][:S], net["Q"][:S])
        dm.set_sources(net["ab"][:S], "scale_shift")
        got = dm.get_sources()
        one = _batch_run(dm, net, S)
        dm.set_loads(net["P"][:S], net["Q"][:S])
        dm.set_sources(got, "currents")
        assert dm.get_sources().tobytes() == got.tobytes()
        two = _batch_run(dm, net, S)
    finally:
        dm.close()
    bound = 6.0 * 2.0 ** -52 * np.abs(net["a"][:S, :, None]) * np.abs(net["case"]["I_N_bus"])[None]
    d = got - net["I_src"][:S]
    err = np.maximum(np.abs(d.real), np.abs(d.imag))
    print("\nSOURCES form 1, device against sweep.source_currents: worst difference / bound %.3f, entries that differ %d of %d"
          % ((err / bound).max(), int((err > 0).sum()), err.size))
    assert (err <= bound).all()
    assert _same(one, two) and (one[2]["flags"] & (1 | 1024) == (1 | 1024)).all()


@pytest.mark.parametrize("kind", ["radial", "meshed", "dense"])
def test_against_the_oracle(kind, request):
    net = request.getfixturevalue(kind)
    if kind == "radial":
        res, U_o, it_o = net["queue"], net["U_oracle"], net["it_oracle"]
    else:
        res = _queue(net, 8, form="scale_shift" if kind == "meshed" else "currents")    # (waves: k_source_expand from row g0 / device-to-device copies)
        U_o, it_o = _oracle_U(net)
    rec = res[0]
    du = float(np.abs(_U(res) - U_o).max())
    print("\nSOURCES %s against the oracle: iterations %s (oracle %s), |dU| %.3e" % (kind, rec["n_iter"].tolist(), it_o, du))
    assert ((rec["flags"] & (1 | 1024)) == (1 | 1024)).all()
    assert du <= 1e-8


@pytest.mark.parametrize("variant", ["three_slots", "chunk_1", "chunk_4_currents", "alone"])
def test_a_scenario_with_sources_does_not_depend_on_its_company(radial, variant):
    net = radial
    assert ((net["queue"][0]["flags"] & 1024) != 0).all()
    if variant == "three_slots":
        got = _queue(net, 3)
    elif variant == "chunk_1":
        got = _queue(net, 8, queue_chunk=1)
    elif variant == "chunk_4_currents":
        dm = _model(net, 8)                                   # form 0 of what the device expanded: k_source_gather instead of k_source_expand
        try:
            cur = []
            for a0 in range(0, S_SCEN, 8):
                dm.set_loads(net["P"][a0:a0 + 8], net["Q"][a0:a0 + 8])
                dm.set_sources(net["ab"][a0:a0 + 8], "scale_shift")
                cur.append(dm.get_sources())
            dm.set_option("queue_chunk", 4)
            dm.queue_sources(np.concatenate(cur), "currents")
            got = dm.solve_queue(net["P"], net["Q"], thresh=TH, want_voltages=True)
        finally:
            dm.close()
    else:
        dm = _model(net, 8)
        try:
            rec, Vm, Va = net["queue"][0].copy(), np.empty_like(net["queue"][1]), np.empty_like(net["queue"][2])
            for s in range(S_SCEN):
                dm.set_loads(net["P"][s], net["Q"][s])
                dm.set_sources(net["ab"][s], "scale_shift")
                dm.set_state(None, None, n_scen=1)
                dm.fund_pf(1e-6, 30)
                dm.solve(TH, 50)
                rec[s] = dm.stats()[0]
                Vm[s], Va[s] = (x[0] for x in dm.get_state())
            got = (rec, Vm, Va)
        finally:
            dm.close()
    assert _same(got, net["queue"]), variant


def test_a_registration_for_another_sweep_is_refused_and_argument_checks_with_a_handle(radial):
    net = radial
    from harmonic_power_flow_amd import _lib
    dm = _model(net, 8)

    def code(fn, *args):
        with pytest.raises(_lib.HpfError) as e:
            fn(*args)
        return e.value.code
    try:
        assert code(dm.set_sources, net["ab"][:2], "scale_shift") == -2          # no batch
        dm.queue_sources(net["ab"][:5], "scale_shift")
        assert code(dm.solve_queue, net["P"], net["Q"]) == -1                     # 5 registered, 24 asked for: nothing solved ...
        plain = dm.solve_queue(net["P"][:3], net["Q"][:3], thresh=TH)             # ... and the registration is gone
        assert not (plain["flags"] & 1024).any()
        dm.set_loads(net["P"][:3], net["Q"][:3])
        assert code(dm.set_sources, net["ab"][:2], "scale_shift") == -1          # 2 rows for a batch of 3
        bad = net["ab"][:3].copy()
        bad[1, 2, 0] = np.nan
        assert code(dm.set_sources, bad, "scale_shift") == -1
        bad = net["I_src"][:3].copy()
        bad[2, 0, 1] = np.inf
        assert code(dm.set_sources, bad, "currents") == -1 and code(dm.queue_sources, bad, "currents") == -1
        h, dp = dm._h, net["ab"].ctypes.data_as(_lib.c_dbl_p)
        assert dm.lib.hpf_set_sources(h, 3, 2, dp, None) == -1 and dm.lib.hpf_set_sources(h, 3, 1, dp, None) == -1
        assert dm.lib.hpf_set_sources(h, 3, 0, None, None) == -1 and dm.lib.hpf_get_sources(h, None) == -1
        with pytest.raises(ValueError):
            dm.set_sources(net["ab"][:3], "phasors")
        with pytest.raises(ValueError):
            dm.set_sources(net["ab"][:3], "currents")
        assert code(dm.get_sources) == -2                                         # none of the refused calls left sources behind
    finally:
        dm.close()


@pytest.mark.parametrize("refill", [True, False])
def test_the_re_solve_paths_carry_the_sources(radial, refill):
    """Warm start, rectangular update, and a cold re-solve forced by the iteration cap.  The base case is deliberately distant: the feeder at
    THREE times its nominal loads (and the model's I_N), so that a warm scenario starts further from its solution than a cold one, which has the
    pf of its own loads.  Measured on the MI355X (mismatch after 3 rectangular iterations, 24 scenarios): cold at most 1.7e-8; warm from that
    base 1.0e-6, 3.3e-7, 1.8e-7, 1.4e-7, 7.1e-8, 5.4e-8, ... ; the base case itself 3.3e-10.  With thresh_h = 5e-8 and max_iter_h = 3 the base
    case converges, every cold solve converges, and the warm scenarios above the threshold come back not converged (bit 8 without bit 0) and are
    solved again cold WITH THEIR SOURCES: 6 of 24 (a re-solve that forgot the sources would land on the fixed point of the model's I_N, 1e-2 p.u.
    away).  The fixed point is the oracle's of check 4 (thresh 1e-9), the bound 1e-8."""
    net = radial
    from harmonic_power_flow_amd import sweep
    dm = _model(net, 8)
    try:
        rec, Vm, Va = sweep.solve_scenarios(dm, net["P"], net["Q"], thresh_h=RESOLVE_THRESH, max_iter_h=RESOLVE_MAX_ITER, want_voltages=True,
                                            refill=refill, update="rectangular", sources={"scale": net["a"], "shift": net["phi"]},
                                            start={"P": 3.0 * net["buses"]["P"].to_numpy(float), "Q": 3.0 * net["buses"]["Q"].to_numpy(float)})
    finally:
        dm.close()
    cold = (rec["flags"] & 256) == 0
    du = float(np.abs(Vm * np.exp(1j * Va) - net["U_oracle"]).max())
    print("\nSOURCES re-solves, refill=%s: %d of %d solved again cold, iterations %s, flags %s, largest mismatch %.3e, |dU| %.3e"
          % (refill, int(cold.sum()), S_SCEN, rec["n_iter"].tolist(), sorted(set(rec["flags"].tolist())), rec["err"].max(), du))
    assert ((rec["flags"] & (1 | 512 | 1024)) == (1 | 512 | 1024)).all()
    assert cold.sum() >= 1
    assert du <= 1e-8


def test_the_step_residual_check_sees_the_sources(radial):
    net, S = radial, 8
    dm = _model(net, 8)
    try:
        dm.set_option("step_residual_check", 1)
        dm.queue_sources(net["ab"], "scale_shift")
        rec = dm.solve_queue(net["P"], net["Q"], thresh=TH)
        dm.set_loads(net["P"][:S], net["Q"][:S])
        dm.set_sources(net["ab"][:S], "scale_shift")
        dm.set_state(None, None, n_scen=S)
        dm.fund_pf(1e-6, 30)
        dm.solve(TH, 50)
        eta = dm.step_residuals()[1]
        st = dm.stats()
    finally:
        dm.close()
    print("\nSOURCES step residual check: step_eta_max %.3e" % eta.max())
    assert not (rec["flags"] & 64).any() and not (st["flags"] & 64).any()
    assert eta.max() < 1e-10


def test_the_accumulators_of_a_sweep_with_sources(radial):
    net = radial
    from harmonic_power_flow_amd import sweep
    dm = _model(net, 8)
    try:
        rec, dist, br = sweep.solve_scenarios(dm, net["P"], net["Q"], thresh_h=TH, sources={"currents": net["I_src"]},
                                              distortion={"thd_limit": 0.05, "bins": 16}, branches={})
        dm.distortion_begin(None, 0.05, 1.0, 16)
        dm.branch_stats_begin(None)
        for s in range(S_SCEN):
            dm.set_loads(net["P"][s], net["Q"][s])
            dm.set_sources(net["I_src"][s], "currents")
            dm.set_state(None, None, n_scen=1)
            dm.fund_pf(1e-6, 30)
            dm.solve(TH, 50)
            dm.distortion_add(s)
            dm.branch_stats_add(s)
        dist1, br1 = dm.distortion_get(), dm.branch_stats_get()
        dm.distortion_end()
        dm.branch_stats_end()
    finally:
        dm.close()
    assert dist.counts.tolist() == [S_SCEN, 0, 0] and br.counts.tolist() == [S_SCEN, 0, 0]
    assert dist1.counts.tolist() == [S_SCEN, 0, 0] and br1.counts.tolist() == [S_SCEN, 0, 0]
    for f in NONSUM_D:
        assert np.array_equal(getattr(dist, f), getattr(dist1, f)), f
    for f in NONSUM_B:
        assert np.array_equal(getattr(br, f), getattr(br1, f)), f
    assert ((rec["flags"] & (1 | 1024)) == (1 | 1024)).all()


def test_hpf_takes_the_sources_of_one_scenario(dense):
    """the reference-shaped call: hp.hpf(..., sources=) on net2 against the oracle's solution of scenario 0 at the feeder's own loads"""
    net = dense
    hp = _hp()
    import os
    fb, fl = os.path.join(INPUTS, "net2_buses.csv"), os.path.join(INPUTS, "net2_lines.csv")
    buses, lines, m, n, c = hp.init_network(fb, fl, settings=net["st"])
    det = {}
    hp.hpf(buses, lines, True, thresh_h=TH, settings=net["st"], ne_dir=INPUTS, verbose=False, return_jacobian=False, details=det,
           sources={"scale": net["a"][0], "shift": net["phi"][0]})
    r = se.oracle_solve(net["case"], np.ones(n), net["I_src"][0], TH)
    du = float(np.abs(det["Vm_raw"] * np.exp(1j * det["Va_raw"]) - r["Vm_raw"] * np.exp(1j * r["Va_raw"])).max())
    print("\nSOURCES hp.hpf on net2: %d iterations (oracle %d), |dU| %.3e" % (det["stats"]["n_iter"][0], r["n_iter_h"], du))
    assert det["stats"]["flags"][0] & 1024 and r["err_h"] <= TH and du <= 1e-8
    with pytest.raises(ValueError):
        hp.hpf(buses, lines, True, settings=net["st"], ne_dir=INPUTS, verbose=False, sources={"scale": np.ones(n - m + 1)})
