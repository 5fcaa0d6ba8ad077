"""Voltage waveforms and waveform statistics on the GPU (hpf_waveform*, k_wave_peaks, k_wave_add; run with -m gpu on an MI355X).

(a) EXACT: with Va = 0 the device's U is (Vm, +-0) whatever sincos it has, the table is formed on the host, every product, difference and sum is
rounded on its own -- samples, peak, kpeak, crest and slack must equal the host emulation (tests/waveform_emul.py: the header's functions in
the kernel's order) bit for bit.  That pins the lane mapping, the wave reduction and the tie rule.
(b) At a solved state against the NumPy restatement tests/waveform_ref.py on the voltages get_state returned.  Bounds are derived, not tuned.
With D = 2^-49 (the 8-ulp allowance of the distortion and branch tests; here it covers the device's sincos of Va) and e = D + (Hn + 2) 2^-53
(the second term: the Hn roundings of the sequential sum and those of a term):
    samples, peak:  b_v = e sum_q |U_q|            (the maximum is 1-Lipschitz)
    kpeak:          |v_ref[kpeak_dev]| >= peak_ref - 2 b_v
    crest:          (b_v + crest b_r) / (rms - b_r) + 4 x 2^-52 crest,  b_r = e rms
    slack:          (D + (Hn + 4) 2^-53) slack     (linear in the |U_q|: D + 2 roundings each -- squares, sqrt --, the product with h^2, Hn sums,
                                                     the final product)
The bound hides nothing: b_v <= 1e-12 peak_ref at every bus is asserted.
(c) A sweep with per-scenario source shifts (the phases differ between scenarios) against waveform_ref + a NumPy fold on the returned voltages;
device against device across slot counts, queue chunks, waves and scenario groups.  (d) Closed means untouched."""
import os

import numpy as np
import pytest

from conftest import INPUTS

import branch_emul as be
import branch_ref as bref
import waveform_emul as we
import waveform_ref as ref

pytestmark = pytest.mark.gpu
D = 2.0 ** -49


def _hp():
    import harmonic_power_flow_amd as hp
    return hp


def _feeder(n, hmax, outdir, seed=0, ties=0):
    hp = _hp()
    from harmonic_power_flow_amd import synth
    fb, fl = synth.gen(n, seed=seed, outdir=str(outdir))
    if ties:
        synth.add_ties(fl, n, ties)
    return _network(fb, fl, hmax)


def _network(fb, fl, hmax):
    hp = _hp()
    st = hp.Settings(H_MAX=hmax)
    buses, lines, m, nn, c = hp.init_network(fb, fl, settings=st)
    Y = hp.build_admittance_matrices(buses, lines, st.HARMONICS)
    NE = hp.import_Norton_Equivalents(buses, True, st, INPUTS)
    return st, buses, Y, NE, lines


def _net1():
    return _network(os.path.join(INPUTS, "net1_buses.csv"), os.path.join(INPUTS, "net1_lines.csv"), 51)


def _loads(buses, S):
    from harmonic_power_flow_amd import synth
    n = len(buses)
    scale = np.stack([synth.scenario_scale(n, s) for s in range(S)])
    return buses["P"].to_numpy(float) * scale, buses["Q"].to_numpy(float) * scale


def _model(net, slots, solver="block_tree"):
    from harmonic_power_flow_amd import api
    st, buses, Y, NE = net[:4]
    return api._device_model(buses, Y, NE, True, st.HARMONICS, solver=solver, max_scenarios=slots)


def _wave(dm, T, sel, orders=None):
    """dm.waveform with other orders than the handle's harmonics (the C entry point takes them with the call)"""
    keep = dm.harmonics
    dm.harmonics = list(keep if orders is None else orders)
    try:
        return dm.waveform(T, sel)
    finally:
        dm.harmonics = keep


def _signed_state(n, Hn, S):
    """Vm [S][Hn*n] (stacked order): fundamental near 1, harmonics near 0.1, perturbed per scenario and entry, signs of both kinds; Va = 0"""
    k = np.arange(Hn * n)
    s = np.arange(S)[:, None]
    sign = np.where((k >= n) & (np.sin(1.3 * k + 0.9 * s) > 0.2), -1.0, 1.0)
    Vm = np.where(k < n, 1.0, 0.1) * (1.0 + 0.3 * np.sin(0.7 * s + 0.37 * k)) * sign
    return Vm, np.zeros_like(Vm)


CASES = {"syn50": (50, 11, 0, 0, "block_tree"), "dense": (50, 11, 1, 0, "dense"), "mesh5": (100, 11, 3, 5, "block_tree")}


@pytest.mark.parametrize("kind", ["syn50", "net1", "dense", "mesh5", "syn1000"])
def test_exact_against_the_emulator_with_zero_angles(tmp_path, kind):
    if kind == "net1":
        net, solver = _net1(), "dense"
    elif kind == "syn1000":
        net, solver = _feeder(1000, 51, tmp_path), "block_tree"
    else:
        nb, hmax, seed, ties, solver = CASES[kind]
        net = _feeder(nb, hmax, tmp_path, seed=seed, ties=ties)
    n, Hn = len(net[1]), len(net[0].HARMONICS)
    assert (n, Hn) == {"syn50": (50, 6), "net1": (20, 26), "dense": (50, 6), "mesh5": (100, 6), "syn1000": (1000, 26)}[kind]
    big = kind == "syn1000"
    sel = [0, n - 1, n // 3, 0]                                     # bus 0, bus n - 1, a repeat
    dm = _model(net, 3 if big else 37, solver=solver)
    checked = 0
    try:
        for S in ((3,) if big else (1, 37)):
            Vm, Va = _signed_state(n, Hn, S)
            dm.set_state(Vm, Va)
            U = ref.rect(Vm, Va, n, Hn)
            assert (U.imag == 0).all() and (U.real < 0).any()
            for T in ((64, 1024) if big else (64, 256, 4096)):
                tab = ref.lib_table(T)
                for orders in ((list(net[0].HARMONICS),) if big else (list(net[0].HARMONICS), list(range(1, Hn + 1)))):
                    got = _wave(dm, T, sel, orders)
                    want = we.waveform(U, orders, T, tab[0], tab[1], sel)
                    for k in ("v", "peak", "kpeak", "crest", "slack"):
                        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (kind, S, T, orders[:3], k)
                    assert np.isfinite(got["crest"]).all() and len(set(got["kpeak"].ravel().tolist())) > 1
                    checked += 1
            # per-bus outputs alone, samples alone
            alone = dm.waveform(64, None)
            assert alone["v"] is None and np.array_equal(alone["peak"], _wave(dm, 64, sel)["peak"])
    finally:
        dm.close()
    assert checked == (2 if big else 12)


def _bounds(w, Hn):
    e = D + (Hn + 2) * 2.0 ** -53
    b_v = e * w["sum_abs"]
    b_r = e * w["rms"]
    return {"v": b_v[..., None], "peak": b_v, "crest": (b_v + w["crest"] * b_r) / (w["rms"] - b_r) + 4 * 2.0 ** -52 * w["crest"],
            "slack": (D + (Hn + 4) * 2.0 ** -53) * w["slack"]}


def _check(got, Vm, Va, n, Hn, orders, T, sel, label):
    """the device's dict `got` against NumPy on the voltages Vm, Va [S][Hn*n] -> the reference dict and its bounds"""
    U = ref.rect(Vm, Va, n, Hn)
    w = ref.waveform(U, orders, T, *ref.lib_table(T))
    b = _bounds(w, Hn)
    assert (b["peak"] <= 1e-12 * w["peak"]).all(), "vacuous bound"
    worst = {}
    for k in ("peak", "crest", "slack"):
        worst[k] = float((np.abs(got[k] - w[k]) / b[k]).max())
    if got["v"] is not None:
        worst["v"] = float((np.abs(got["v"] - w["v"][:, sel]) / b["v"][:, sel]).max())
    at_dev = np.take_along_axis(np.abs(w["v"]), got["kpeak"][..., None].astype(np.int64), axis=-1)[..., 0]
    worst["kpeak"] = float(((w["peak"] - at_dev) / (2 * b["peak"])).max())
    print("\nWAVEFORM %s: %d scenarios x %d buses x %d harmonics, T = %d; largest error / bound: %s; largest bound / peak %.3g"
          % (label, U.shape[0], n, Hn, T, ", ".join("%s %.3g" % kv for kv in worst.items()), float((b["peak"] / w["peak"]).max())))
    assert max(worst.values()) <= 1.0, worst
    assert ((got["kpeak"] >= 0) & (got["kpeak"] < T)).all()
    return w, b


@pytest.mark.parametrize("kind", ["syn50", "net1", "syn1000"])
def test_solved_state_within_the_derived_bound_and_set_state_alone(tmp_path, kind):
    net = _net1() if kind == "net1" else _feeder(*{"syn50": (50, 11), "syn1000": (1000, 51)}[kind], tmp_path)
    n, Hn, orders = len(net[1]), len(net[0].HARMONICS), list(net[0].HARMONICS)
    big = kind == "syn1000"
    dm = _model(net, 3 if big else 37, solver="dense" if kind == "net1" else "block_tree")
    sel = [0, n - 1, n // 2]
    try:
        with pytest.raises(Exception) as nobatch:
            dm.waveform()
        for S in ((3,) if big else (1, 37)):
            P, Q = _loads(net[1], S)
            dm.set_loads(P, Q)
            dm.set_state(None, None, n_scen=S)
            dm.fund_pf(1e-6, 30)
            dm.solve(1e-4, 50)
            assert (dm.stats()["flags"] & 1).all()
            Vm, Va = dm.get_state()
            got = dm.waveform(1024, sel)
            w, b = _check(got, Vm, Va, n, Hn, orders, 1024, sel, "%s, after solve, S = %d" % (kind, S))
            assert (w["crest"] > 1.41).all() and (got["peak"] <= w["peak"] + w["slack"] + b["peak"]).all()
            k = np.arange(Vm.shape[1])
            s = np.arange(S)[:, None]
            Vm2, Va2 = Vm * (1.0 + 0.02 * np.sin(0.7 * s + 0.37 * k)), Va + 0.3 * np.cos(0.3 * s + 0.11 * k)
            dm.set_state(Vm2, Va2)
            got2 = dm.waveform(256, sel)
            _check(got2, Vm2, Va2, n, Hn, orders, 256, sel, "%s, after set_state alone, S = %d" % (kind, S))
            assert np.abs(got2["peak"] - w["peak"]).max() > 1e3 * b["peak"].max()          # (not the solved state's waveforms)
    finally:
        dm.close()
    assert nobatch.value.code == -2


def test_bad_orders_and_selections_are_refused_before_any_launch(tmp_path):
    """HPF_E_ARG from the host checks of hpf_waveform and hpf_waveform_stats_begin, with a real handle and a batch in it: an order of 0, -3 or
    32768, a selected bus of n or -1, a bad T.  Nothing may be written (the outputs keep their fill) and the accumulator stays closed."""
    from harmonic_power_flow_amd import _lib, device
    net = _feeder(50, 11, tmp_path)
    n, Hn, good = len(net[1]), len(net[0].HARMONICS), list(net[0].HARMONICS)
    dm = _model(net, 2)
    codes = {}

    def code(f, *a):
        try:
            f(*a)
        except _lib.HpfError as e:
            return e.code
        return 0

    def raw(orders, T, sel):
        """hpf_waveform itself on pre-filled outputs -> (code, outputs untouched)"""
        S = dm.S
        o = np.ascontiguousarray(orders, dtype=np.int32)
        sl = np.ascontiguousarray(sel, dtype=np.int32)
        f = [np.full((S, n), -7.0) for _ in range(3)]
        k = np.full((S, n), -7, dtype=np.int32)
        v = np.full((S, max(len(sl), 1), max(T, 1)), -7.0)
        rc = dm.lib.hpf_waveform(dm._h, o.ctypes.data_as(_lib.c_int_p), int(T), len(sl), sl.ctypes.data_as(_lib.c_int_p) if len(sl) else None,
                                 v.ctypes.data_as(_lib.c_dbl_p), f[0].ctypes.data_as(_lib.c_dbl_p), k.ctypes.data_as(_lib.c_int_p),
                                 f[1].ctypes.data_as(_lib.c_dbl_p), f[2].ctypes.data_as(_lib.c_dbl_p))
        return rc, all((a == -7).all() for a in f + [k, v])

    try:
        Vm, Va = _signed_state(n, Hn, 2)
        dm.set_state(Vm, Va)
        assert raw(good, 64, [0, n - 1])[0] == 0                                  # (the same call with good arguments runs)
        for name, bad in (("zero", 0), ("negative", -3), ("too_large", 32768)):
            for pos in (0, Hn - 1):
                orders = list(good)
                orders[pos] = bad
                codes["order_%s_%d" % (name, pos)] = raw(orders, 64, [0])
                assert code(_wave, dm, 64, None, orders) == -1
                mem = device.device_memory()
                keep = dm.harmonics
                dm.harmonics = orders
                try:
                    assert code(dm.waveform_stats_begin, 64) == -1
                finally:
                    dm.harmonics = keep
                assert device.device_memory() == mem and code(dm.waveform_stats_get) == -2          # nothing allocated, still closed
        for name, sel in (("sel_n", [n]), ("sel_minus_one", [-1]), ("sel_last_bad", [0, n - 1, n])):
            codes[name] = raw(good, 64, sel)
            assert code(dm.waveform, 64, sel) == -1
        for T in (0, 63, 100, 8192):
            codes["T_%d" % T] = raw(good, T, [0])
        assert raw(list(good[:-1]) + [32767], 64, [n - 1])[0] == 0                # (the largest order and the last bus are fine)
    finally:
        dm.close()
    assert all(v == (-1, True) for v in codes.values()), codes


# ---- (c), (d): the sweep ---------------------------------------------------------------------------------------------------------------------
N_SCEN, T_SWEEP = 40, 1024


def _reference(Vm, Va, rec, n, Hn, orders, lim, climit, deferred=None):
    U = ref.rect(Vm, Va, n, Hn)
    w = ref.waveform(U, orders, T_SWEEP, *ref.lib_table(T_SWEEP))
    b = _bounds(w, Hn)
    want = ref.accumulate(w["peak"], w["crest"], np.arange(len(Vm)), rec["flags"], bref.thd_ok(Vm, n, Hn), lim, climit, deferred=deferred)
    return w, b, want


def _check_stats(got, w, b, want, label):
    assert got.counts.tolist() == want["counts"].tolist(), (label, got.counts, want["counts"])
    ok = want["added_mask"]
    added = int(ok.sum())
    worst = {}
    for pre in ref.QUANT:
        v, bv = w[pre][ok], b[pre][ok]
        err = np.abs(getattr(got, pre + "_max") - want[pre + "_max"])
        assert (err <= bv.max(axis=0)).all(), pre
        worst[pre + "_max"] = float((err / bv.max(axis=0)).max())
        srt = np.sort(v, axis=0)
        clear = np.ones(v.shape[1], bool) if added == 1 else srt[-2] + 2 * bv.max(axis=0) < srt[-1]
        assert clear.mean() > 0.9 and np.array_equal(getattr(got, pre + "_arg")[clear], want[pre + "_arg"][clear]), pre
        for f, s, bs in ((pre + "_sum", v.sum(0), bv.sum(0)), (pre + "_sumsq", (v * v).sum(0), (2 * v * bv + bv * bv).sum(0))):
            miss = np.abs(getattr(got, f) - want[f]) - (bref.sum_bound(s, added) + bs)
            assert (miss <= 0).all(), (f, float(miss.max()))
        assert np.array_equal(getattr(got, pre + "_over"), want[pre + "_over"]), pre
        assert 0 < getattr(got, pre + "_over").sum() < v.size                       # the limits do cut the samples
    print("\nWAVESTATS %s: added %d; largest |max - numpy| / bound: %s" % (label, added, worst))


@pytest.fixture(scope="module")
def sweep40(tmp_path_factory):
    """50 buses x harmonics to 11, scenarios 0..39 with per-scenario source shifts through 16 slots: everything closed BEFORE any waveform call
    (records, voltages -> the limits), the waveform statistics open, closed again, all three accumulators open."""
    from harmonic_power_flow_amd import device, sweep
    net = _feeder(50, 11, tmp_path_factory.mktemp("w50"))
    n, Hn, orders = len(net[1]), len(net[0].HARMONICS), list(net[0].HARMONICS)
    P, Q = _loads(net[1], N_SCEN)
    dm = _model(net, 16)
    out = dict(net=net, n=n, Hn=Hn, orders=orders, P=P, Q=Q)
    try:
        nnl = dm.n - dm.m
        src = {"shift": np.random.default_rng(20261).uniform(-0.075, 0.075, size=(N_SCEN, nnl))}
        out["src"] = src
        out["off"] = sweep.solve_scenarios(dm, P, Q, want_voltages=True, sources=src)
        rec, Vm, Va = out["off"]
        w, b, _ = _reference(Vm, Va, rec, n, Hn, orders, None, np.inf)
        good = (rec["flags"] & 1) != 0
        lim = np.array([be.midpoint_limit(w["peak"][good, i]) for i in range(n)])
        climit = float(be.midpoint_limit(w["crest"][good]))
        out["cfg"] = {"samples": T_SWEEP, "peak_limit": lim, "crest_limit": climit}
        out["good"] = good
        with pytest.raises(Exception) as closed_get:
            dm.waveform_stats_get()
        out["closed_get"] = closed_get.value
        out["mem0"] = device.device_memory()
        dm.waveform_stats_begin(T_SWEEP, lim, climit)
        out["mem_open"] = device.device_memory()
        dm.waveform_stats_begin(256, None)                                         # (on an open one: reset)
        dm.waveform_stats_end()
        dm.waveform_stats_end()                                                     # (closed already: fine)
        out["mem1"] = device.device_memory()
        with pytest.raises(Exception) as closed_add:
            dm.waveform_stats_add(0)
        out["closed_add"] = closed_add.value
        out["on"] = sweep.solve_scenarios(dm, P, Q, want_voltages=True, sources=src, waveform=out["cfg"])
        out["off2"] = sweep.solve_scenarios(dm, P, Q, want_voltages=True, sources=src)
        out["all"] = sweep.solve_scenarios(dm, P, Q, want_voltages=True, sources=src, distortion={}, branches={}, waveform=out["cfg"])
        out["one"] = sweep.solve_scenarios(dm, P[:1], Q[:1], max_iter_h=2, sources={"shift": src["shift"][:1]}, distortion={}, waveform=out["cfg"])
        bad = lim.copy()
        bad[0] = np.nan
        with pytest.raises(Exception) as nan:
            dm.waveform_stats_begin(T_SWEEP, bad)
        out["nan"] = nan.value
        with pytest.raises(Exception) as badT:
            dm.waveform_stats_begin(1000)
        out["badT"] = badT.value
    finally:
        dm.close()
    return out


def test_sweep_statistics_match_numpy_on_the_returned_voltages(sweep40):
    s = sweep40
    rec, Vm, Va, stats = s["on"]
    n, Hn = s["n"], s["Hn"]
    assert stats.samples == T_SWEEP and stats.counts.tolist() == [N_SCEN, 0, 0] and len(set(rec["n_iter"])) >= 1
    w, b, want = _reference(Vm, Va, rec, n, Hn, s["orders"], s["cfg"]["peak_limit"], s["cfg"]["crest_limit"])
    # the limits sit in gaps of the reference samples wider than twice the bound: the over counts are then exact
    good = s["good"]
    for i in range(n):
        srt = np.sort(w["peak"][good, i])
        k = len(srt) // 2
        assert srt[k] - srt[k - 1] > 2 * b["peak"][good, i].max(), i
    srt = np.sort(w["crest"][good].ravel())
    k = len(srt) // 2
    assert srt[k] - srt[k - 1] > 2 * b["crest"][good].max()
    # the phases do differ between the scenarios: the crest factor of a bus moves by far more than its bound
    assert (np.ptp(w["crest"], axis=0) > 1e6 * b["crest"].max(axis=0)).all()
    _check_stats(stats, w, b, want, "50 x 6, 40 scenarios with source shifts, 16 slots")


def test_closed_means_untouched(sweep40):
    s = sweep40
    for a, b, c in zip(s["off"], s["on"][:3], s["off2"]):
        assert a.tobytes() == b.tobytes() == c.tobytes()                            # open only reads; closed again: as before any waveform call
    for a, b in zip(s["off"], s["all"][:3]):
        assert a.tobytes() == b.tobytes()
    assert s["mem0"] == s["mem1"] and s["mem_open"][0] == s["mem0"][0] + 10 and s["mem_open"][1] > s["mem0"][1]
    assert s["closed_get"].code == -2 and s["closed_add"].code == -2 and s["nan"].code == -1 and s["badT"].code == -1


def test_all_three_accumulators_open_and_an_unconverged_scenario(sweep40):
    from harmonic_power_flow_amd import sweep
    s = sweep40
    assert len(s["all"]) == 6 and isinstance(s["all"][3], sweep.DistortionStats) and isinstance(s["all"][4], sweep.BranchStats)
    assert isinstance(s["all"][5], sweep.WaveformStats)
    for f in sweep.WaveformStats.ARRAYS:                                            # bit for bit, sums included: the same order of arrival
        assert np.array_equal(getattr(s["all"][5], f), getattr(s["on"][3], f)), f
    assert s["all"][3].counts.tolist() == s["all"][5].counts.tolist() == s["all"][4].counts.tolist()
    rec, dist, wst = s["one"]
    assert not (rec["flags"][0] & 1) and wst.counts.tolist() == dist.counts.tolist() and wst.counts[0] == 0 and wst.counts.sum() >= 1
    assert (wst.peak_arg == -1).all() and (wst.crest_over == 0).all()


@pytest.mark.parametrize("variant", ["all_slots", "chunk1", "chunk4", "waves", "one_group", "four_groups"])
def test_statistics_do_not_depend_on_slots_queue_chunk_waves_or_groups(sweep40, variant):
    from harmonic_power_flow_amd import sweep
    s = sweep40
    dm = _model(s["net"], N_SCEN if variant == "all_slots" else 16)
    try:
        if variant.startswith("chunk"):
            dm.set_option("queue_chunk", int(variant[5:]))
        if variant.endswith("group") or variant.endswith("groups"):
            dm.set_option("scenario_groups", 1 if variant == "one_group" else 4)
        rec, Vm, Va, stats = sweep.solve_scenarios(dm, s["P"], s["Q"], want_voltages=True, refill=variant != "waves", sources=s["src"],
                                                   waveform=s["cfg"])
    finally:
        dm.close()
    base = s["on"][3]
    assert np.array_equal(Vm, s["on"][1]) and np.array_equal(rec.view(np.uint8), s["on"][0].view(np.uint8))
    for f in ref.EXACT:
        assert np.array_equal(getattr(stats, f), getattr(base, f)), (variant, f)
    w, b, want = _reference(Vm, Va, rec, s["n"], s["Hn"], s["orders"], s["cfg"]["peak_limit"], s["cfg"]["crest_limit"])
    _check_stats(stats, w, b, want, variant)


def test_explicit_add_and_the_reference_shaped_calls(tmp_path):
    """waveform_stats_add after a plain solve on a dense handle (ids from first_id; a second add doubles the counts and keeps the smaller ids), and
    hp.waveforms / hp.solve(waveforms=True) on a reference network."""
    hp = _hp()
    net = _net1()
    n, Hn, orders = len(net[1]), len(net[0].HARMONICS), list(net[0].HARMONICS)
    P, Q = _loads(net[1], 4)
    dm = _model(net, 4, solver="dense")
    try:
        dm.set_loads(P, Q)
        dm.set_state(None, None, n_scen=4)
        dm.fund_pf(1e-6, 30)
        dm.waveform_stats_begin(T_SWEEP)
        with pytest.raises(Exception) as early:
            dm.waveform_stats_add(0)
        dm.solve(1e-4, 50)
        Vm, Va = dm.get_state()
        rec = dm.stats()
        dm.waveform_stats_add(1000)
        once = dm.waveform_stats_get()
        dm.waveform_stats_add(2000)
        twice = dm.waveform_stats_get()
        dm.waveform_stats_end()
    finally:
        dm.close()
    assert early.value.code == -2 and (rec["flags"] & 1).all()
    U = ref.rect(Vm, Va, n, Hn)
    w = ref.waveform(U, orders, T_SWEEP, *ref.lib_table(T_SWEEP))
    b = _bounds(w, Hn)
    assert once.counts.tolist() == [4, 0, 0] and (np.abs(once.peak_max - w["peak"].max(axis=0)) <= b["peak"].max(axis=0)).all()
    assert set(once.peak_arg.tolist()) <= set(range(1000, 1004)) and (once.peak_over == 0).all()
    assert twice.counts.tolist() == [8, 0, 0] and np.array_equal(twice.peak_arg, once.peak_arg) and np.array_equal(twice.peak_max, once.peak_max)
    st = hp.Settings(H_MAX=11)
    fb, fl = os.path.join(INPUTS, "net1_buses.csv"), os.path.join(INPUTS, "net1_lines.csv")
    plain = hp.solve(fb, fl, coupled=True, settings=st, ne_dir=INPUTS)
    res = hp.solve(fb, fl, coupled=True, settings=st, ne_dir=INPUTS, waveforms=True)
    assert set(res) - set(plain) == {"waveforms"} and res["V"].equals(plain["V"])
    buses = hp.init_network(fb, fl, settings=st)[0]
    table, v = hp.waveforms(res["V"], buses, st.HARMONICS, samples=256, at=[0, len(buses) - 1])
    table2, none = hp.waveforms(res["V"], buses, samples=1024)
    assert none is None and table2.equals(res["waveforms"]) and list(table.columns) == ["peak", "kpeak", "crest", "slack"]
    assert v.shape == (2, 256) and np.array_equal(np.abs(v.to_numpy()).max(axis=1), table["peak"].to_numpy()[[0, -1]])
    V = res["V"]
    nn, H = len(buses), len(st.HARMONICS)
    got = {k: table[k].to_numpy()[None] for k in table.columns}
    got["v"] = v.to_numpy()[None]
    _check(got, V["V_m"].to_numpy()[None], V["V_a"].to_numpy()[None], nn, H, list(st.HARMONICS), 256, [0, nn - 1], "hp.waveforms, net1 H11")
