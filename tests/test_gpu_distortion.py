"""The distortion accumulator on the GPU (hpf_distortion_*, k_distortion_add; run with -m gpu on an MI355X) against the NumPy restatement
tests/distortion_ref.py evaluated on the voltages the SAME sweep returned -- never against the library's own statistics.

The device's sqrt / division may differ from NumPy's in the last bits, so threshold-type fields are bracketed: with d = 2^-49 (8 ulp: at most
2 ulp each for sqrt and the division if they were not correctly rounded, doubled) the device's `over` count lies between the NumPy counts of
x (1 - d) > L and x (1 + d) > L, and a histogram sample sits in the bin of thd (1 - d) or of thd (1 + d).  The bracket must not hide a failure:
the share of (entry, scenario) samples on which its two ends disagree is asserted <= 1 %; the limits are midpoints between adjacent sorted NumPy
samples near the median (counts about half, no sample within d of a limit unless two samples nearly coincide), hist_max = 1.25 x the largest THD,
64 bins.  max: rtol d; arg: exact wherever the NumPy runner-up is more than d below the maximum; counts: exact; sums: within
added x 2^-52 x sum|x| + d sum|x| (the order of arrival + the last bits of the samples)."""
import numpy as np
import pytest

from conftest import INPUTS

import distortion_emul as de
import distortion_ref as ref

pytestmark = pytest.mark.gpu
D = 2.0 ** -49
NONSUM = ("counts", "x_max", "x_arg", "x_over", "thd_max", "thd_arg", "thd_over", "thd_hist")


def _hp():
    import harmonic_power_flow_amd as hp
    return hp


def _feeder(n, hmax, outdir, seed=0, ties=0):
    hp = _hp()
    from harmonic_power_flow_amd import synth
    fb, fl = synth.gen(n, seed=seed, outdir=str(outdir))
    if ties:
        synth.add_ties(fl, n, ties)
    st = hp.Settings(H_MAX=hmax)
    buses, lines, m, nn, c = hp.init_network(fb, fl, settings=st)
    Y = hp.build_admittance_matrices(buses, lines, st.HARMONICS)
    NE = hp.import_Norton_Equivalents(buses, True, st, INPUTS)
    return st, buses, Y, NE


def _loads(buses, S):
    from harmonic_power_flow_amd import synth
    n = len(buses)
    scale = np.stack([synth.scenario_scale(n, s) for s in range(S)])
    return buses["P"].to_numpy(float) * scale, buses["Q"].to_numpy(float) * scale


def _model(net, slots, solver="block_tree"):
    from harmonic_power_flow_amd import api
    st, buses, Y, NE = net
    return api._device_model(buses, Y, NE, True, st.HARMONICS, solver=solver, max_scenarios=slots)


def _check(got, Vm, ids, flags, n, Hn, cfg, deferred=None, label="", counts=None):
    """device statistics `got` (DistortionStats) against NumPy on the voltages Vm [S][Hn*n] -> the reference dict (counts: the expected counters
    where the sweep's differ from the yardstick's, which has no queue)"""
    want = ref.accumulate(Vm, ids, flags, n, Hn, deferred=deferred, **cfg)
    assert got.counts.tolist() == (want["counts"].tolist() if counts is None else counts), (label, got.counts, want["counts"])
    added, x, thd = int(want["counts"][0]), want["x"], want["thd"]
    if added == 0:
        return want
    B = cfg["bins"]
    lim = np.asarray(cfg["limit"])[None, :, None]
    lo_x, hi_x = x * (1 - D) > lim, x * (1 + D) > lim
    lo_t, hi_t = thd * (1 - D) > cfg["thd_limit"], thd * (1 + D) > cfg["thd_limit"]
    lo_b, hi_b = ref.bins_of(thd * (1 - D), cfg["hist_max"], B), ref.bins_of(thd * (1 + D), cfg["hist_max"], B)
    share = [(lo_x != hi_x).mean(), (lo_t != hi_t).mean(), (lo_b != hi_b).mean()]
    print("\nDISTORTION %s: added %d; bracket ends disagree on %.4f %% (x limits) %.4f %% (thd limit) %.4f %% (bins) of the samples; "
          "over counts x %d..%d of %d, thd %d of %d" % (label, added, 100 * share[0], 100 * share[1], 100 * share[2], int(lo_x.sum(0).min()),
                                                         int(hi_x.sum(0).max()), added, int(want["thd_over"].sum()), thd.size))
    assert max(share) <= 0.01, ("vacuous bracket", share)
    assert (lo_x.sum(0) <= got.x_over).all() and (got.x_over <= hi_x.sum(0)).all()
    assert (lo_t.sum(0) <= got.thd_over).all() and (got.thd_over <= hi_t.sum(0)).all()
    assert 0 < want["thd_over"].sum() < thd.size and (want["x_over"].sum(axis=1) > 0).all()       # the limits do cut the samples
    sure, maybe = np.zeros((n, B + 1), np.int64), np.zeros((n, B + 1), np.int64)
    for lb, hb in zip(lo_b, hi_b):
        same = lb == hb
        np.add.at(sure, (np.arange(n)[same], lb[same]), 1)
        for b in (lb, hb):
            np.add.at(maybe, (np.arange(n)[~same], b[~same]), 1)
    assert (got.thd_hist.sum(axis=1) == added).all()
    assert (sure <= got.thd_hist).all() and (got.thd_hist <= sure + maybe).all()
    for g_max, g_arg, v, w_max in ((got.x_max, got.x_arg, x, want["x_max"]), (got.thd_max, got.thd_arg, thd, want["thd_max"])):
        assert (np.abs(g_max - w_max) <= D * np.abs(w_max)).all()
        srt = np.sort(v, axis=0)
        clear = np.ones(w_max.shape, bool) if added == 1 else srt[-2] < srt[-1] * (1 - D)
        w_arg = np.asarray(ids)[want["added_mask"]][np.argmax(v, axis=0)]
        assert clear.mean() > 0.9 and np.array_equal(g_arg[clear], w_arg[clear])
        assert np.isin(g_arg, np.asarray(ids)[want["added_mask"]]).all()
    for f, s in (("x_sum", x.sum(0)), ("x_sumsq", (x * x).sum(0)), ("thd_sum", thd.sum(0)), ("thd_sumsq", (thd * thd).sum(0))):
        miss = np.abs(getattr(got, f) - want[f]) - (ref.sum_bound(s, added) + D * s)
        assert (miss <= 0).all(), (f, float(miss.max()))
    return want


def _cfg_from(Vm, flags, n, Hn):
    return de.settings_for(Vm, flags, n, Hn, bins=64)


@pytest.fixture(scope="module")
def sweep75(tmp_path_factory):
    """200 buses x harmonics to 27, seed 3, scenarios 0..74: a sweep with the accumulator OFF on a fresh 32-slot handle (records, voltages -> the
    limits), then the same sweep with it ON on another fresh 32-slot handle."""
    from harmonic_power_flow_amd import sweep
    net = _feeder(200, 27, tmp_path_factory.mktemp("f200"), seed=3)
    P, Q = _loads(net[1], 75)
    dm = _model(net, 32)
    try:
        off = sweep.solve_scenarios(dm, P, Q, want_voltages=True)
        with pytest.raises(Exception) as closed:
            dm.distortion_get()
    finally:
        dm.close()
    n, Hn = len(net[1]), len(net[0].HARMONICS)
    cfg = _cfg_from(off[1], off[0]["flags"], n, Hn)
    dm = _model(net, 32)
    try:
        on = sweep.solve_scenarios(dm, P, Q, want_voltages=True, distortion=cfg)
    finally:
        dm.close()
    return dict(net=net, P=P, Q=Q, n=n, Hn=Hn, cfg=cfg, off=off, on=on, closed=closed.value)


def test_sweep_statistics_match_numpy_on_the_returned_voltages(sweep75):
    s = sweep75
    rec, Vm, Va, stats = s["on"]
    assert stats.added == 75 and stats.counts.tolist() == [75, 0, 0] and len(set(rec["n_iter"])) > 1
    _check(stats, Vm, np.arange(75), rec["flags"], s["n"], s["Hn"], s["cfg"], label="200 x 14, 75 scenarios, 32 slots")
    assert stats.harmonics == list(s["net"][0].HARMONICS) and stats.bins == 64
    w = stats.worst(1)[0]
    assert w[2] == stats.thd_max.max() and w[2] == rec["thd_max"].max() and w[1] == int(np.argmax(rec["thd_max"]))   # the record's worst bus


@pytest.mark.parametrize("variant", ["waves", "one_slot", "all_slots", "one_group"])
def test_statistics_do_not_depend_on_slots_queue_or_groups(sweep75, variant):
    """refill=False (waves + distortion_add), a 1-slot and a 75-slot handle, one scenario group: every non-sum array bit-identical to the 32-slot
    queue's; the sums within the bound of the order of arrival."""
    from harmonic_power_flow_amd import sweep
    s = sweep75
    dm = _model(s["net"], {"one_slot": 1, "all_slots": 75}.get(variant, 32))
    try:
        if variant == "one_group":
            dm.set_option("scenario_groups", 1)
        rec, Vm, Va, stats = sweep.solve_scenarios(dm, s["P"], s["Q"], want_voltages=True, refill=variant != "waves", distortion=s["cfg"])
    finally:
        dm.close()
    base = s["on"][3]
    assert np.array_equal(Vm, s["on"][1]) and np.array_equal(rec.view(np.uint8), s["on"][0].view(np.uint8))
    for f in NONSUM:
        assert np.array_equal(getattr(stats, f), getattr(base, f)), (variant, f)
    _check(stats, Vm, np.arange(75), rec["flags"], s["n"], s["Hn"], s["cfg"], label=variant)


def test_off_means_off_and_on_only_reads(sweep75):
    s = sweep75
    for a, b in zip(s["off"], s["on"][:3]):
        assert a.tobytes() == b.tobytes()
    assert getattr(s["closed"], "code", None) == -2          # distortion_get on a closed accumulator: HPF_E_STATE


def test_reported_scenarios_are_deferred_and_added_by_their_resolve(tmp_path):
    from harmonic_power_flow_amd import sweep
    net = _feeder(100, 27, tmp_path, seed=1)
    n, Hn = len(net[1]), len(net[0].HARMONICS)
    P, Q = _loads(net[1], 7)
    dm = _model(net, 3)
    try:
        dm.set_option("pivot_growth_limit_log10", 0)
        rec0, Vm0, Va0 = sweep.solve_scenarios(dm, P, Q, want_voltages=True)
        cfg = _cfg_from(Vm0, rec0["flags"], n, Hn)
        dm.distortion_begin(cfg["limit"], cfg["thd_limit"], cfg["hist_max"], cfg["bins"])
        raw = dm.solve_queue(P, Q)
        st_raw = dm.distortion_get()
        dm.distortion_end()
        rec, Vm, Va, stats = sweep.solve_scenarios(dm, P, Q, want_voltages=True, distortion=cfg)
    finally:
        dm.close()
    assert ((raw["flags"] & 8) == 8).all() and st_raw.counts.tolist() == [0, 0, 7] and (st_raw.thd_arg == -1).all()
    assert stats.counts.tolist() == [7, 0, 7] and ((rec["flags"] & (8 | 16 | 1)) == (8 | 16 | 1)).all()
    want = _check(stats, Vm, np.arange(7), rec["flags"], n, Hn, cfg, label="100 x 14, 7 flagged scenarios re-solved pivoted", counts=[7, 0, 7])
    assert want["counts"].tolist() == [7, 0, 0]


def test_unconverged_scenarios_are_skipped(sweep75):
    from harmonic_power_flow_amd import sweep
    s = sweep75
    dm = _model(s["net"], 32)
    try:
        rec, stats = sweep.solve_scenarios(dm, s["P"], s["Q"], max_iter_h=5, distortion=s["cfg"])
    finally:
        dm.close()
    assert ((rec["flags"] & 1) == 0).all() and stats.counts.tolist() == [0, 75, 0]
    assert (stats.x_arg == -1).all() and (stats.thd_arg == -1).all()
    for f in ("x_over", "thd_over", "thd_hist", "x_sum", "x_sumsq", "thd_sum", "thd_sumsq", "x_max", "thd_max"):
        assert not getattr(stats, f).any(), f


@pytest.mark.parametrize("kind", ["dense", "meshed"])
def test_every_solver_path_adds_after_its_waves(tmp_path, kind):
    from harmonic_power_flow_amd import sweep
    net = _feeder(100, 11, tmp_path, seed=1) if kind == "dense" else _feeder(100, 27, tmp_path, seed=3, ties=5)
    n, Hn = len(net[1]), len(net[0].HARMONICS)
    P, Q = _loads(net[1], 9)
    dm = _model(net, 4, solver="dense" if kind == "dense" else "block_tree")
    try:
        if kind == "meshed":
            assert dm.tree_census()["ties"] == 5
        rec0, Vm0, Va0 = sweep.solve_scenarios(dm, P, Q, want_voltages=True)
        cfg = _cfg_from(Vm0, rec0["flags"], n, Hn)
        rec, Vm, Va, stats = sweep.solve_scenarios(dm, P, Q, want_voltages=True, distortion=cfg)
    finally:
        dm.close()
    assert stats.added == int(((rec["flags"] & 1) != 0).sum()) >= 1 and stats.counts[1] == 9 - stats.added
    _check(stats, Vm, np.arange(9), rec["flags"], n, Hn, cfg, label=kind + " handle, 9 scenarios in waves of 4")


def test_explicit_add_after_a_plain_solve(tmp_path):
    net = _feeder(100, 11, tmp_path, seed=1)
    n, Hn = len(net[1]), len(net[0].HARMONICS)
    P, Q = _loads(net[1], 5)
    dm = _model(net, 8)
    try:
        dm.set_loads(P, Q)
        dm.set_state(None, None, n_scen=5)
        dm.fund_pf(1e-6, 30)
        dm.distortion_begin(None, np.inf, 1.0, 4)
        with pytest.raises(Exception) as early:
            dm.distortion_add(0)                              # no finished solve yet
        dm.solve(1e-4, 50)
        Vm, Va = dm.get_state()
        flags = dm.stats()["flags"]
        cfg = _cfg_from(Vm, flags, n, Hn)
        dm.distortion_begin(cfg["limit"], cfg["thd_limit"], cfg["hist_max"], cfg["bins"])       # (reset, other bin count)
        dm.distortion_add(1000)
        stats = dm.distortion_get()
        dm.distortion_add(2000)                               # the same batch once more under other ids: counts double, the smaller ids stay
        twice = dm.distortion_get()
        dm.distortion_end()
        with pytest.raises(Exception) as closed:
            dm.distortion_add(0)
        with pytest.raises(Exception) as bad:
            dm.distortion_begin(None, np.inf, 1.0, 257)
    finally:
        dm.close()
    assert early.value.code == -2 and closed.value.code == -2 and bad.value.code == -1
    assert (flags & 1).all() and stats.counts.tolist() == [5, 0, 0]
    assert ((stats.x_arg >= 1000) & (stats.x_arg <= 1004)).all() and ((stats.thd_arg >= 1000) & (stats.thd_arg <= 1004)).all()
    _check(stats, Vm, 1000 + np.arange(5), flags, n, Hn, cfg, label="explicit add, ids 1000..1004")
    assert twice.counts.tolist() == [10, 0, 0] and np.array_equal(twice.x_arg, stats.x_arg) and np.array_equal(twice.x_max, stats.x_max)
    assert np.array_equal(twice.thd_hist, 2 * stats.thd_hist) and np.array_equal(twice.x_over, 2 * stats.x_over)


def test_headline_shape(tmp_path):
    """1 000 buses x 26 harmonics, 128 Monte-Carlo scenarios through 48 slots."""
    from harmonic_power_flow_amd import sweep
    net = _feeder(1000, 51, tmp_path)
    n, Hn = len(net[1]), len(net[0].HARMONICS)
    assert (n, Hn) == (1000, 26)
    P, Q = _loads(net[1], 128)
    dm = _model(net, 48)
    try:
        rec0, Vm0, Va0 = sweep.solve_scenarios(dm, P, Q, want_voltages=True)
        cfg = _cfg_from(Vm0, rec0["flags"], n, Hn)
        rec, Vm, Va, stats = sweep.solve_scenarios(dm, P, Q, want_voltages=True, distortion=cfg)
    finally:
        dm.close()
    assert np.array_equal(Vm, Vm0) and np.array_equal(rec.view(np.uint8), rec0.view(np.uint8))
    assert stats.added == int(((rec["flags"] & 1) != 0).sum()) == 128
    _check(stats, Vm, np.arange(128), rec["flags"], n, Hn, cfg, label="1000 x 26, 128 scenarios, 48 slots")
    p95 = stats.thd_percentile(95)
    _, thd = ref.samples(Vm, n, Hn)
    exact = np.percentile(thd, 95, axis=0, method="higher")
    w = cfg["hist_max"] / 64
    assert (p95 - exact > -D * exact - 1e-12 * w).all() and (p95 - exact <= w * (1 + 1e-12) + D * exact).all()
