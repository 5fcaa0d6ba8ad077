"""Warm start of a sweep from a solved base case (hpf_start_*, include/hpf.h "Start state"; run with -m gpu on an MI355X).

Shapes, the smallest that reach every path: syn100 x harmonics to 11, coupled -- radial block tree, the fast queue -- with 8 slots and 24
synth.scenario_scale scenarios, so that slots refill; the same feeder with 2 loop-closing lines (meshed waves); net2 with its golden inputs
(fewer than 32 buses: DENSE waves).  The base case is the feeder at its nominal loads, solved cold to 1e-9.

Bounds.  Bit-for-bit wherever the library promises it (unset = untouched, apply_start = set_state, a scenario's result independent of slots /
queue_chunk / scenario_groups and equal to its solve alone, a cold re-solve equal to the sweep without a start).  Warm against cold: both sweeps
stop at thresh_h = 1e-9, and |dU| <= 1e-8 is the project's fixed-point gate (the oracle: 2.4e-12, tests/test_warm_start_oracle.py).  The
iteration cap -- the warm total at most HALF the cold total -- keeps the test from passing on a start that did nothing; the oracle's figures
are 3 against 19..25 per scenario."""
import numpy as np
import pytest

from conftest import INPUTS

pytestmark = pytest.mark.gpu
TH = 1e-9
S_SCEN = 24
NONSUM_D = ("x_max", "x_arg", "x_over", "thd_max", "thd_arg", "thd_over", "thd_hist")
NONSUM_B = ("irms_max", "irms_arg", "irms_over", "loss_max", "loss_arg", "lossh_max", "lossh_arg")


def _hp():
    import harmonic_power_flow_amd as hp
    return hp


def _net(kind, outdir):
    """-> (settings, buses, Y, NE, solver)"""
    import os
    hp = _hp()
    from harmonic_power_flow_amd import synth
    st = hp.Settings(H_MAX=11)
    if kind == "dense":
        fb, fl = os.path.join(INPUTS, "net2_buses.csv"), os.path.join(INPUTS, "net2_lines.csv")
    else:
        fb, fl = synth.gen(100, seed=0, outdir=str(outdir))
        if kind == "meshed":
            synth.add_ties(fl, 100, 2)
    buses, lines, m, n, c = hp.init_network(fb, fl, settings=st)
    Y = hp.build_admittance_matrices(buses, lines, st.HARMONICS)
    NE = hp.import_Norton_Equivalents(buses, True, st, INPUTS)
    return st, buses, Y, NE, "dense" if kind == "dense" else "block_tree"


def _model(net, slots):
    from harmonic_power_flow_amd import api
    st, buses, Y, NE, solver = net
    return api._device_model(buses, Y, NE, True, st.HARMONICS, solver=solver, max_scenarios=slots)


def _loads(buses, S):
    from harmonic_power_flow_amd import synth
    n = len(buses)
    scale = np.stack([synth.scenario_scale(n, s) for s in range(S)])
    return buses["P"].to_numpy(float) * scale, buses["Q"].to_numpy(float) * scale


def _nominal(buses):
    return buses["P"].to_numpy(float), buses["Q"].to_numpy(float)


def _flat(n, Hn):
    Vm = np.full(n * Hn, 0.1)
    Vm[:n] = 1.0
    return Vm, np.zeros(n * Hn)


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _du(a, b):
    return float(np.abs(a[1] * np.exp(1j * a[2]) - b[1] * np.exp(1j * b[2])).max())


@pytest.fixture(scope="module")
def radial(tmp_path_factory):
    """the radial feeder: base state, the cold queue and the warm queue of the 24 scenarios through 8 slots (thresh_h 1e-9, voltages kept)"""
    net = _net("radial", tmp_path_factory.mktemp("syn100"))
    n, Hn = len(net[1]), len(net[0].HARMONICS)
    P, Q = _loads(net[1], S_SCEN)
    dm = _model(net, 8)
    try:
        assert dm.solver == "block_tree" and dm.tree_census()["ties"] == 0
        cold = dm.solve_queue(P, Q, thresh=TH, want_voltages=True)
        P0, Q0 = _nominal(net[1])
        dm.set_loads(P0, Q0)
        dm.set_state(None, None, n_scen=1)
        dm.fund_pf(1e-6, 30)
        dm.solve(TH, 50)
        assert dm.stats()["flags"][0] == 1
        base = tuple(a[0].copy() for a in dm.get_state())
        dm.capture_start(0)
        captured = dm.get_start()
        warm = dm.solve_queue(P, Q, thresh=TH, want_voltages=True)
        dm.clear_start()
    finally:
        dm.close()
    return dict(net=net, n=n, Hn=Hn, P=P, Q=Q, cold=cold, warm=warm, base=base, captured=captured)


def test_unset_means_untouched(radial):
    r = radial
    dm = _model(r["net"], 8)
    try:
        dm.set_start(*r["base"])
        dm.clear_start()
        dm.clear_start()                                      # (already unset: HPF_OK)
        again = dm.solve_queue(r["P"], r["Q"], thresh=TH, want_voltages=True)
    finally:
        dm.close()
    assert _same(again, r["cold"]) and not (r["cold"][0]["flags"] & 256).any()


def test_apply_start_equals_set_state_and_capture_equals_the_scenario(radial):
    r = radial
    Vm0, Va0 = r["base"]
    Va0 = Va0 + 0.0
    Vm0 = Vm0.copy()
    Vm0[3] = -Vm0[3]                                          # (raw states may carry signed magnitudes and un-wrapped angles)
    Va0[5] += 7.0
    dm = _model(r["net"], 8)
    try:
        dm.set_start(Vm0, Va0)
        got = dm.get_start()
        dm.apply_start(5)
        a = dm.get_state()
        dm.set_loads(r["P"][:5], r["Q"][:5])
        _, err_a = dm.mismatch(want_f=False)
        dm.set_state(np.tile(Vm0, (5, 1)), np.tile(Va0, (5, 1)))
        b = dm.get_state()
        _, err_b = dm.mismatch(want_f=False)
        dm.set_state(None, None, n_scen=5)                    # a batch of five different states: capture scenario 3 of it
        dm.fund_pf(1e-6, 30)
        dm.solve(1e-4, 50)
        st = dm.get_state()
        dm.capture_start(3)
        cap = dm.get_start()
        with pytest.raises(Exception) as out_of_range:
            dm.capture_start(5)
    finally:
        dm.close()
    assert _same(got, (Vm0, Va0)) and a[0].shape == (5, r["n"] * r["Hn"])
    assert _same(a, b) and err_a.tobytes() == err_b.tobytes()
    assert _same(cap, (st[0][3], st[1][3])) and not np.array_equal(st[0][3], st[0][2])
    assert out_of_range.value.code == -1
    assert _same(r["captured"], r["base"])                    # capture of the solved base case = its get_state


def test_warm_queue_converges_in_a_fraction_of_the_iterations(radial):
    cold, warm = radial["cold"][0], radial["warm"][0]
    du = _du(radial["warm"], radial["cold"])
    print("\nWARM START radial: cold iterations %s (total %d), warm %s (total %d), |dU| %.3e"
          % (cold["n_iter"].tolist(), cold["n_iter"].sum(), warm["n_iter"].tolist(), warm["n_iter"].sum(), du))
    assert ((cold["flags"] & (1 | 256)) == 1).all()
    assert ((warm["flags"] & (1 | 256)) == (1 | 256)).all()
    assert (warm["n_iter"] <= cold["n_iter"]).all()
    assert 2 * int(warm["n_iter"].sum()) <= int(cold["n_iter"].sum())
    assert du <= 1e-8


@pytest.mark.parametrize("variant", ["alone", "three_slots", "chunk_1", "one_group"])
def test_a_warm_scenario_does_not_depend_on_its_company(radial, variant):
    r = radial
    dm = _model(r["net"], 3 if variant == "three_slots" else 8)
    try:
        dm.set_start(*r["base"])
        if variant == "alone":
            rec, Vm, Va = r["warm"][0].copy(), np.empty_like(r["warm"][1]), np.empty_like(r["warm"][2])
            for s in range(S_SCEN):
                dm.apply_start(1)
                dm.set_loads(r["P"][s], r["Q"][s])
                dm.solve(TH, 50)
                rec[s] = dm.stats()[0]
                Vm[s], Va[s] = (a[0] for a in dm.get_state())
            got = (rec, Vm, Va)
        else:
            if variant == "chunk_1":
                dm.set_option("queue_chunk", 1)
            if variant == "one_group":
                dm.set_option("scenario_groups", 1)
            got = dm.solve_queue(r["P"], r["Q"], thresh=TH, want_voltages=True)
    finally:
        dm.close()
    assert _same(got, r["warm"]), variant


def test_scenario_groups_do_not_change_a_warm_scenario(radial):
    """(8 slots never split into groups: a group needs 32 running scenarios) 72 scenarios through 64 slots, 4 groups against 1; the first 24
    are the scenarios of the 8-slot queue"""
    r = radial
    P, Q = _loads(r["net"][1], 72)
    res = []
    for groups in (4, 1):
        dm = _model(r["net"], 64)
        try:
            dm.set_option("scenario_groups", groups)
            if groups == 4:
                assert dm.scenario_groups(64) == 2
            dm.set_start(*r["base"])
            res.append(dm.solve_queue(P, Q, thresh=TH, want_voltages=True))
        finally:
            dm.close()
    assert _same(res[0], res[1])
    assert _same([a[:S_SCEN] for a in res[0]], r["warm"])


def _open_accumulators(dm):
    dm.distortion_begin(None, 0.05, 1.0, 16)
    dm.branch_stats_begin(None)


def test_a_bad_start_is_reported_and_deferred(radial):
    """the reference's flat state WITHOUT pf and max_iter_h = 2: non-convergence by construction (the oracle's mismatch after two iterations
    from it stays above 1e2 on this feeder)"""
    r = radial
    dm = _model(r["net"], 8)
    try:
        dm.set_start(*_flat(r["n"], r["Hn"]))
        _open_accumulators(dm)
        rec = dm.solve_queue(r["P"], r["Q"], max_iter=2)
        dist, br = dm.distortion_get(), dm.branch_stats_get()
    finally:
        dm.close()
    print("\nWARM START bad start: mismatch after 2 iterations %.3e .. %.3e" % (rec["err"].min(), rec["err"].max()))
    assert ((rec["flags"] & (256 | 2 | 1)) == (256 | 2)).all() and (rec["n_iter"] == 2).all()
    assert dist.counts.tolist() == [0, 0, S_SCEN] and br.counts.tolist() == [0, 0, S_SCEN]


def _overflow(n, Hn):
    """a start no Newton iteration can leave: magnitudes of 1e200 are finite and non-zero (hpf_start_set takes them), but the first mismatch
    forms their squares -- inf - inf, non-finite, flags bit 2: plain IEEE arithmetic, no fault of any kind"""
    return np.full(n * Hn, 1e200), np.zeros(n * Hn)


@pytest.mark.parametrize("case", ["flat_50", "flat_18", "flat_8", "overflow_50"])
def test_what_does_not_converge_warm_is_solved_cold_as_without_a_start(radial, case):
    """solve_scenarios from a bad start against solve_scenarios(start=None) with the same settings, both accumulators open.  Wherever a
    scenario's final record lacks bit 8 it was solved again cold: record and voltages are those of the sweep without a start, bit for bit.
    Where that holds for EVERY scenario the accumulators must agree too, bit for bit: counts (added, skipped), maxima, args, over counts and
    the histogram.  (The deferred counter is the one field that cannot agree: it counts the scenarios that were solved twice, 24 here and
    none in the sweep without a start; the sums depend on the order of arrival by rounding, include/hpf.h.)
    flat_50: the reference's flat state without pf, the normal cap: the oracle converges from it in 17..27 iterations, nothing may need a
      re-solve;  flat_18 cuts into that range (the oracle: scenarios 0, 1 and 4 need 21, 27 and 20): a mixed sweep;
    flat_8: far below it (the oracle's mismatch from this start is still above 1e2 after 13 iterations): EVERY scenario goes the cold way --
      where the cap of 8 lets none converge either (cold: 16..29), so both sweeps skip all 24;
    overflow_50: a start whose first mismatch is not finite: every scenario is reported with bit 2, repeated from the start state through
      apply_start + solve, still not finite, and solved cold under the normal cap, where all 24 converge: the accumulators are full, and
      everything in them was added by the cold re-solves."""
    from harmonic_power_flow_amd import sweep
    r = radial
    kind, max_iter_h = case.split("_")[0], int(case.split("_")[1])
    bad = (_flat if kind == "flat" else _overflow)(r["n"], r["Hn"])
    cfg = {"limit": None, "thd_limit": 0.05, "hist_max": 1.0, "bins": 16}
    res = []
    for start in (None, bad):
        dm = _model(r["net"], 8)
        try:
            res.append(sweep.solve_scenarios(dm, r["P"], r["Q"], max_iter_h=max_iter_h, want_voltages=True, distortion=cfg,
                                             branches={"rating": None}, start=start))
            assert not dm.has_start()
        finally:
            dm.close()
    cold, warm = res
    again = (warm[0]["flags"] & 256) == 0
    print("\nWARM START %s: %d of %d scenarios solved again cold; counts distortion %s / %s, branches %s / %s (with / without the start)"
          % (case, again.sum(), S_SCEN, warm[3].counts.tolist(), cold[3].counts.tolist(), warm[4].counts.tolist(), cold[4].counts.tolist()))
    assert not (cold[0]["flags"] & 256).any()
    assert ((warm[0]["flags"][~again] & 1) == 1).all()        # what kept bit 8 did converge from the start state
    assert _same([a[again] for a in warm[:3]], [a[again] for a in cold[:3]])
    for k in (3, 4):
        assert warm[k].counts[2] >= again.sum() and cold[k].counts[2] == 0
        assert warm[k].counts[0] == int((warm[0]["flags"] & 1).sum())
    if case == "flat_18":
        assert again.any()
    if case in ("flat_8", "overflow_50"):
        assert again.all()
        assert warm[3].counts.tolist() == ([S_SCEN, 0, S_SCEN] if kind == "overflow" else [0, S_SCEN, S_SCEN])
        for k, names in ((3, NONSUM_D), (4, NONSUM_B)):
            assert warm[k].counts[:2].tolist() == cold[k].counts[:2].tolist()
            for f in names:
                assert np.array_equal(getattr(warm[k], f), getattr(cold[k], f)), f
        if kind == "overflow":
            assert (warm[3].thd_arg >= 0).all() and len(set(warm[3].thd_arg.tolist())) > 1 and warm[4].irms_max.max() > 0


def test_the_start_argument_is_checked(radial):
    from harmonic_power_flow_amd import sweep
    r = radial
    P, Q = r["P"][:3], r["Q"][:3]
    dm = _model(r["net"], 8)
    try:
        as_list = sweep.solve_scenarios(dm, P, Q, thresh_h=TH, want_voltages=True, start=[r["base"][0], r["base"][1]])
        for bad in ("median", 3.0, {"P": P[0]}, (r["base"][0],)):
            with pytest.raises(ValueError):
                sweep.solve_scenarios(dm, P, Q, start=bad)
        dm.set_start(*r["base"])                              # a start state of the caller's own and start=None: refused, not run warm
        with pytest.raises(ValueError):
            sweep.solve_scenarios(dm, P, Q)
        assert dm.has_start()
    finally:
        dm.close()
    assert _same(as_list, [a[:3] for a in r["warm"]])


@pytest.mark.parametrize("kind", ["meshed", "dense"])
@pytest.mark.parametrize("refill", [True, False])
def test_meshed_and_dense_handles_start_warm_through_their_waves(tmp_path, kind, refill):
    from harmonic_power_flow_amd import sweep
    net = _net(kind, tmp_path)
    P, Q = _loads(net[1], 9)
    P0, Q0 = _nominal(net[1])
    dm = _model(net, 4)
    try:
        assert dm.solver == net[4] and (kind == "dense" or dm.tree_census()["ties"] == 2)
        cold = sweep.solve_scenarios(dm, P, Q, thresh_h=TH, want_voltages=True, refill=refill)
        warm = sweep.solve_scenarios(dm, P, Q, thresh_h=TH, want_voltages=True, refill=refill, start={"P": P0, "Q": Q0})
        mean = sweep.solve_scenarios(dm, P, Q, thresh_h=TH, refill=refill, start="mean")
    finally:
        dm.close()
    du = _du(warm, cold)
    print("\nWARM START %s (refill=%s): cold iterations %s, warm %s, from the mean loads %s, |dU| %.3e"
          % (kind, refill, cold[0]["n_iter"].tolist(), warm[0]["n_iter"].tolist(), mean["n_iter"].tolist(), du))
    assert ((cold[0]["flags"] & (1 | 256)) == 1).all()
    for rec in (warm[0], mean):
        assert ((rec["flags"] & (1 | 256)) == (1 | 256)).all()
        assert (rec["n_iter"] <= cold[0]["n_iter"]).all()
        assert 2 * int(rec["n_iter"].sum()) <= int(cold[0]["n_iter"].sum())
    assert du <= 1e-8


def test_argument_checks_without_a_device_fault(radial):
    r = radial
    Vm0, Va0 = r["base"]
    dm = _model(r["net"], 8)
    codes = {}

    def code(name, fn, *a):
        with pytest.raises(Exception) as e:
            fn(*a)
        codes[name] = e.value.code

    try:
        code("apply_unset", dm.apply_start, 1)
        code("get_unset", dm.get_start)
        code("capture_no_batch", dm.capture_start, 0)
        for name, k, v in (("nan", 7, np.nan), ("inf", 7, np.inf), ("zero", 11, 0.0)):
            bad = Vm0.copy()
            bad[k] = v
            code(name, dm.set_start, bad, Va0)
        bad = Va0.copy()
        bad[2] = np.nan
        code("nan_angle", dm.set_start, Vm0, bad)
        code("get_still_unset", dm.get_start)
        assert dm.lib.hpf_start_set(None, None, None) == -1 and dm.lib.hpf_start_apply(None, 1) == -1
        assert dm.lib.hpf_start_clear(None) == -1 and dm.lib.hpf_start_capture(None, 0) == -1 and dm.lib.hpf_start_get(None, None, None) == -1
        dm.set_start(Vm0, Va0)
        code("apply_too_many", dm.apply_start, 9)
        dm.solve_queue(r["P"][:2], r["Q"][:2])
        code("capture_after_queue", dm.capture_start, 0)
        bad = np.tile(Vm0, (2, 1))                            # a batch whose scenario 1 holds what set_start refuses: not captured, and the
        bad[1, 4] = np.nan                                    # start that was being overwritten is gone
        dm.set_state(bad, np.tile(Va0, (2, 1)))
        code("capture_nan", dm.capture_start, 1)
        assert not dm.has_start()
        dm.clear_start()
        dm.capture_start(0)
        assert _same(dm.get_start(), (Vm0, Va0))
    finally:
        dm.close()
    assert codes == {"apply_unset": -2, "get_unset": -2, "capture_no_batch": -2, "nan": -1, "inf": -1, "zero": -1, "nan_angle": -1,
                     "get_still_unset": -2, "apply_too_many": -1, "capture_after_queue": -2, "capture_nan": -2}, codes
