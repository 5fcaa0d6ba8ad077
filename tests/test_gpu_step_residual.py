"""The device-side residual check of the Newton steps (option "step_residual_check": k_step_residual + k_step_eta, hpf_get_step_residuals,
hpf_stat.flags bits 6 / 7) against the host yardstick tests/stepcheck.py on the SAME J (hpf_jacobian_csr), f and step.

Bounds.  The device evaluates eta in float64 with one fma per product: its rounding is at most (k + 4) 2^-53 of the denominator, k the
largest number of stored entries in a row of J; the host value is formed in long double.  Agreement is asked within 2 (k + 4) 2^-53, absolute
(eta is a ratio to that denominator).  Healthy steps are gated at ETA_MAX = 1e-12 by test_gpu_step_accuracy.py; here eta_max <= 1e-11 and no flag
at the default limit 1e-10."""
import numpy as np
import pytest

import stepcheck as sc

from conftest import GOLD, INPUTS
from test_gpu_step_accuracy import ETA_MAX, N_BUS, PATH_N, PATH_SEED, _net, _scales

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53
BIT_REPEATED, BIT_STEP_FIRST, BIT_STEP_RESULT = 16, 64, 128


def _model(net, cap, solver="block_tree", options=None, check=True):
    from harmonic_power_flow_amd import api
    dm = api._device_model(net["buses"], net["Y"], net["NE"], net["coupled"], net["st"].HARMONICS, solver=solver, max_scenarios=cap, options=options)
    dm.set_option("step_residual_check", 1 if check else 0)
    return dm


def _seed(dm, net, S_):
    sc_ = _scales(net["n"], S_)
    dm.set_loads(net["buses"]["P"].to_numpy(float) * sc_, net["buses"]["Q"].to_numpy(float) * sc_)
    dm.set_state(None, None, n_scen=S_)
    dm.fund_pf(1e-6, 30)
    return dm.get_state()


def _agree(tag, dm, c):
    """One step of every scenario from the current state: device eta_last against stepcheck.backward_error -> worst difference in units of the bound."""
    steps = sc.newton_steps(dm, c)
    last, big = dm.step_residuals()
    worst = 0.0
    for s, (J, f, dx) in enumerate(steps):
        k = int(np.diff(J.indptr).max())
        host = sc.backward_error(J, dx, f)
        bound = 2 * (k + 4) * U53
        print("\nSTEPRESIDUAL %-28s scenario %2d: device eta %.3e host %.3e  |diff| %.2e  bound %.2e (k = %d)" % (tag, s, last[s], host, abs(last[s] - host), bound, k))
        assert abs(last[s] - host) <= bound, (tag, s, last[s], host, bound)
        assert big[s] >= last[s]
        worst = max(worst, abs(last[s] - host) / bound)
    return worst


# (tag, buses, H_MAX, generator seed, coupled, ties, solver, options, scenarios)
PATHS = [("radial b=14", PATH_N, 13, PATH_SEED, True, 0, "block_tree", None, 3),
         ("radial b=30", PATH_N, 29, PATH_SEED, True, 0, "block_tree", None, 1),
         ("radial b=52", PATH_N, 51, PATH_SEED, True, 0, "block_tree", None, 33),
         ("radial b=100", PATH_N, 99, PATH_SEED, True, 0, "block_tree", None, 3),
         ("meshed k=3 b=30", N_BUS, 29, 0, True, 3, "block_tree", None, 3),
         ("uncoupled b=30", N_BUS, 29, 0, False, 0, "block_tree", None, 3),
         ("dense b=14", N_BUS, 13, 0, True, 0, "dense", None, 3),
         ("HPF_GJ_MODE=0 b=28", N_BUS, 27, 0, True, 0, "block_tree", "HPF_GJ_MODE=0", 3)]


@pytest.mark.parametrize("path", [p[0] for p in PATHS])
def test_device_eta_agrees_with_host_and_check_is_inert_when_healthy(path, tmp_path):
    tag, n, hmax, seed, coupled, ties, solver, options, S_ = next(p for p in PATHS if p[0] == path)
    net = _net(tmp_path, n, hmax, seed=seed, coupled=coupled, ties=ties)
    dm = _model(net, S_, solver, options)
    try:
        assert dm.solver == solver
        start = _seed(dm, net, S_)
        last, big = dm.step_residuals()
        assert np.isnan(last).all() and np.isnan(big).all()            # no step taken yet
        # 1. agreement with the host yardstick at the pf seed and after 3 iterations
        _agree(tag + " seed", dm, net["c"])
        dm.mismatch(want_f=False)
        dm.iterate(2)
        _agree(tag + " iter3", dm, net["c"])
        # 2. inert when healthy: a whole solve with the check on and off
        res = {}
        for on in (1, 0):
            dm.set_option("step_residual_check", on)
            dm.set_state(*start)
            n_iter, err, _ = dm.solve(1e-4, 50)
            res[on] = (n_iter.copy(), dm.get_state(), dm.stats()["flags"].copy())
            if on:
                eta_max = dm.step_residuals()[1]
                print("\nSTEPRESIDUAL %-28s solve: eta_max %.3e, n_iter %s" % (tag, np.nanmax(eta_max), n_iter))
                assert (eta_max[n_iter > 0] <= 1e-11).all(), eta_max
            else:
                with pytest.raises(Exception):
                    dm.step_residuals()                                 # HPF_E_STATE with the check off
        assert np.array_equal(res[1][0], res[0][0])
        assert res[1][1][0].tobytes() == res[0][1][0].tobytes() and res[1][1][1].tobytes() == res[0][1][1].tobytes()
        assert np.array_equal(res[1][2], res[0][2]) and not (res[1][2] & (BIT_STEP_FIRST | BIT_STEP_RESULT)).any(), res[1][2]
    finally:
        dm.close()


GOLDEN_ROWS = ["net1_H11_c", "net1_H11_uc", "net1_H51_c", "net2_H11_c", "net2_H51_uc", "net3_H11_c", "net3_H51_c", "lin4_H11_c"]


@pytest.mark.parametrize("name", GOLDEN_ROWS + ["syn50_H11_c", "syn100_H11_c"])
def test_golden_rows_are_unchanged_by_the_check(name, tmp_path):
    """hpf() of a golden parity row with check_steps on and off: byte-identical voltages and n_iter; the row's largest eta is printed."""
    import os
    import harmonic_power_flow_amd as hp
    from harmonic_power_flow_amd import synth
    net_name, hs, cs = name.split("_")
    st = hp.Settings(H_MAX=int(hs[1:]))
    if net_name.startswith("syn"):
        fb, fl = synth.gen(int(net_name[3:]), seed=0, outdir=str(tmp_path))
    else:
        fb, fl = os.path.join(INPUTS, net_name + "_buses.csv"), os.path.join(INPUTS, net_name + "_lines.csv")
    buses, lines, m, n, c = hp.init_network(fb, fl, settings=st)
    out = {}
    for on in (True, False):
        det = {}
        V, err_h, n_iter_h, _ = hp.hpf(buses, lines, cs == "c", settings=st, ne_dir=INPUTS, verbose=False, return_jacobian=False, details=det,
                                       check_steps=on)
        out[on] = (n_iter_h, det["Vm_raw"].tobytes(), det["Va_raw"].tobytes(), det)
    det = out[True][3]
    print("\nSTEPRESIDUAL golden row %-14s solver %-10s n_iter %2d eta_max %.3e flagged %s" % (name, det["solver"], out[True][0], det["step_eta_max"], det["step_flagged"]))
    assert out[False][3]["step_eta_max"] is None and out[False][3]["step_flagged"] is False
    assert out[True][:3] == out[False][:3]
    assert not det["step_flagged"] and det["step_eta_max"] <= 1e-11


def _ablated(tmp_path):
    return _net(tmp_path, N_BUS, 27), "HPF_DEBUG_ABLATE=2 HPF_GJ_MODE=0"


def test_positive_control_finite_wrong_step_is_flagged(tmp_path):
    """HPF_DEBUG_ABLATE=2 on the pivoted variant (test_gpu_step_accuracy.py's control: finite wrong step, host eta >= 1e-9): the device sees the
    same eta (it judges against the true J), hpf_solve(max_iter=1) sets bits 6 and 7 and no bit 4 (that handle has no repeat); check off: no bit."""
    net, options = _ablated(tmp_path)
    dm = _model(net, 1, options=options)
    try:
        start = _seed(dm, net, 1)
        J, f, dx = sc.newton_steps(dm, net["c"])[0]
        host = sc.backward_error(J, dx, f)
        dev = dm.step_residuals()[0][0]
        k = int(np.diff(J.indptr).max())
        print("\nSTEPRESIDUAL positive control: device eta %.6e host %.6e |diff| %.2e bound %.2e" % (dev, host, abs(dev - host), 2 * (k + 4) * U53))
        assert host >= 1e-9 and np.isfinite(dx).all()
        assert abs(dev - host) <= 2 * (k + 4) * U53
        for on in (1, 0):
            dm.set_option("step_residual_check", on)
            dm.set_state(*start)
            dm.solve(1e-4, 1)
            flags = int(dm.stats()["flags"][0])
            want = (BIT_STEP_FIRST | BIT_STEP_RESULT) if on else 0
            assert flags & (BIT_STEP_FIRST | BIT_STEP_RESULT | BIT_REPEATED) == want, (on, flags)
    finally:
        dm.close()


def _case38(tmp_path):
    return _net(tmp_path, 286, 15, seed=441135, frac_nl=0.85, n_pv=2)


def test_open_item_fuzz_case_38_is_flagged_and_repeated(tmp_path):
    """Fuzz case 38, built exactly as test_gpu_step_accuracy.py's case g builds it (unmonitored nested bordered core: the fused step loses
    ~2e-6 of the step, flags bit 3 stays clear).  With the check on, hpf_solve(max_iter=1) flags the first pass (bit 6), repeats the scenario
    with partial pivoting (bit 4), the repeat's own step passes (bit 7 clear), and x0 - x1 of that call meets ETA_MAX against J and f at the seed."""
    net = _case38(tmp_path)
    dm = _model(net, 1)
    try:
        start = _seed(dm, net, 1)
        f, _ = dm.mismatch()
        J = dm.jacobian_csr(0)
        dm.solve(1e-4, 1)
        flags = int(dm.stats()["flags"][0])
        Vm1, Va1 = dm.get_state()
        dx = sc.stacked(start[0][0], start[1][0], net["c"]) - sc.stacked(Vm1[0], Va1[0], net["c"])
        eta = sc.backward_error(J, dx, f[0])
        last, big = dm.step_residuals()
        print("\nSTEPRESIDUAL fuzz case 38: flags %d, returned step: host eta %.3e device eta %.3e" % (flags, eta, last[0]))
        assert flags & BIT_STEP_FIRST and flags & BIT_REPEATED and not flags & BIT_STEP_RESULT, flags
        assert eta <= ETA_MAX
    finally:
        dm.close()


def test_queue_reports_and_sweep_resolves_the_flagged_scenario(tmp_path):
    """A batch of case 38's feeder: scenario 0 carries the loads of the open item (synth.scenario_scale(n, 0)), the others scaled-down loads.
    hpf_solve_queue reports bit 6 for the scenario whose steps miss the limit and does not repeat; sweep.solve_scenarios returns it re-solved
    (bit 4 set, bit 7 clear) and summarize counts it."""
    from harmonic_power_flow_amd import sweep
    net = _case38(tmp_path)
    n = net["n"]
    P0, Q0 = net["buses"]["P"].to_numpy(float), net["buses"]["Q"].to_numpy(float)
    scale = np.ones((4, n))
    scale[0] = _scales(n, 1)[0]
    scale[1:] *= np.array([0.05, 0.1, 0.02])[:, None]
    P, Q = P0 * scale, Q0 * scale
    dm = _model(net, 4)
    try:
        rec = dm.solve_queue(P, Q, max_iter=1)
        print("\nSTEPRESIDUAL queue flags %s" % rec["flags"])
        assert rec["flags"][0] & BIT_STEP_FIRST and not (rec["flags"] & BIT_REPEATED).any()
        assert not (rec["flags"][1:] & BIT_STEP_FIRST).any(), rec["flags"]
        out = sweep.solve_scenarios(dm, P, Q, max_iter_h=1)
        print("STEPRESIDUAL sweep flags %s" % out["flags"])
        assert out["flags"][0] & BIT_STEP_FIRST and out["flags"][0] & BIT_REPEATED and not out["flags"][0] & BIT_STEP_RESULT
        assert not (out["flags"][1:] & (BIT_STEP_FIRST | BIT_REPEATED)).any()
        summ = sweep.summarize(out.view(np.uint8).reshape(4, 24))
        assert summ["step_flagged"] == 1
    finally:
        dm.close()


def test_option_ranges_and_state_errors(tmp_path):
    from harmonic_power_flow_amd import _lib
    net = _net(tmp_path, 40, 5)
    dm = _model(net, 1, check=False)
    try:
        for name, value in (("step_residual_check", 2), ("step_residual_check", -1), ("step_residual_limit_log10", 1), ("step_residual_limit_log10", -17),
                            ("step_residual", 1)):
            with pytest.raises(_lib.HpfError) as e:
                dm.set_option(name, value)
            assert e.value.code == -1, (name, value)                    # HPF_E_ARG
        for value in (0, -16, -10):
            dm.set_option("step_residual_limit_log10", value)
        _seed(dm, net, 1)
        with pytest.raises(_lib.HpfError) as e:
            dm.step_residuals()
        assert e.value.code == -2                                       # HPF_E_STATE: check off
        dm.set_option("step_residual_check", 1)
        assert np.isnan(dm.step_residuals()[0]).all()
        by, fl, ln = dm.kernel_model("step_residual")
        assert by > 0 and fl > 0 and ln == 2
        dm.timing(True)
        dm.mismatch(want_f=False)
        dm.iterate(1)
        ms, cnt = dm.timing_get()["step_residual"]
        dm.timing(False)
        assert cnt == 1 and ms > 0
        assert np.isfinite(dm.step_residuals()[0]).all()
    finally:
        dm.close()
