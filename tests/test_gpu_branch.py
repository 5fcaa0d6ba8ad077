"""Branch flows and branch statistics on the GPU (hpf_branch_*, k_branch_flows, k_branch_add; run with -m gpu on an MI355X) against the NumPy
restatement tests/branch_ref.py evaluated on the voltages the SAME run returned (get_state, or the sweep's Vm, Va) -- never against the
library's own numbers.

Tolerances are derived, not tuned.  The device forms U = Vm exp(j Va) with its own sincos, NumPy with the host's; the difference U[i] - U[j]
cancels (voltage drops are 1e-4 of |U|, |y| reaches 1.1e4 p.u.), so the bound is absolute.  With D = 2^-49 (the 8-ulp allowance of
tests/test_gpu_distortion.py) and d = U[i] - U[j]:
    |d_dev - d_np| <= bd = D (|U_i| + |U_j|)
    |I_dev - I_np| <= bI = D (|y| (|U_i| + |U_j|) + |I|)
    irms:  | ||a|| - ||b|| | <= ||a - b||  ->  sqrt(sum_q bI^2) + (Hn + 2) 2^-53 irms        (the second term: the rounding of the sum and the sqrt)
    loss[q][e] = Re(y) |d|^2  ->  bl = Re(y) (2 |d| bd + bd^2) + 4 x 2^-53 loss;  loss_e, loss_harm: sum_q bl + Hn 2^-53 sum_q loss;
    loss_h: sum_e bl + nb 2^-53 sum_e loss
    thd_i = ||I_harm|| / |I_0|  ->  (bH + thd_i bI_0) / (|I_0| - bI_0) + 4 x 2^-52 thd_i, checked where |I_0| > 2 bI_0 (elsewhere it is
    inf, NaN or rounding noise by definition)
Every test prints the largest observed ratio to its bound.  The bound must not hide a failure: on the headline feeder the irms bound is below
1e-9 irms for at least 75 % of the branches (NumPy on the golden: irms quartile 0.287 p.u., bound at most 7.4e-11)."""
import hashlib

import numpy as np
import pytest

from conftest import INPUTS

import branch_emul as be
import branch_ref as ref

pytestmark = pytest.mark.gpu
D = 2.0 ** -49
EXACT = ("counts", "irms_max", "irms_arg", "irms_over", "loss_max", "loss_arg", "lossh_max", "lossh_arg")


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
    return st, buses, Y, NE, lines


def _loads(buses, S):
    from harmonic_power_flow_amd import synth
    n = len(buses)
    scale = np.stack([synth.scenario_scale(n, s) for s in range(S)])
    return buses["P"].to_numpy(float) * scale, buses["Q"].to_numpy(float) * scale


def _model(net, slots, solver="block_tree"):
    from harmonic_power_flow_amd import api
    st, buses, Y, NE = net[:4]
    return api._device_model(buses, Y, NE, True, st.HARMONICS, solver=solver, max_scenarios=slots)


def _bounds(fr, to, y, U, w):
    """the derived bounds of the module docstring for the NumPy flows w of U [S][Hn][n]"""
    Hn, nb = y.shape
    aU = np.abs(U)
    bd = D * (aU[:, :, fr] + aU[:, :, to])
    bI = D * (np.abs(y)[None] * (aU[:, :, fr] + aU[:, :, to]) + np.abs(w["I"]))
    b = {"I": bI, "irms": np.sqrt((bI * bI).sum(axis=1)) + (Hn + 2) * 2.0 ** -53 * w["irms"]}
    bl = y.real[None] * (2 * np.abs(w["d"]) * bd + bd * bd) + 4 * 2.0 ** -53 * w["loss_q"]
    b["loss"] = bl.sum(axis=1) + Hn * 2.0 ** -53 * w["loss"]
    b["loss_harm"] = bl[:, 1:].sum(axis=1) + Hn * 2.0 ** -53 * w["loss_harm"]
    b["loss_h"] = bl.sum(axis=2) + nb * 2.0 ** -53 * w["loss_q"].sum(axis=2)
    b["I0"], b["IH"] = bI[:, 0], np.sqrt((bI[:, 1:] ** 2).sum(axis=1))
    return b


def _check_flows(got, fr, to, y, Vm, Va, n, Hn, label):
    U = ref.rect(Vm, Va, n, Hn)
    w = ref.flows(fr, to, y, U)
    b = _bounds(fr, to, y, U, w)
    worst = {}
    for k in ("I", "irms", "loss", "loss_harm", "loss_h"):
        assert got[k].shape == w[k].shape, k
        err = np.abs(got[k] - w[k])
        with np.errstate(invalid="ignore", divide="ignore"):
            worst[k] = float(np.nanmax(np.where(b[k] > 0, err / b[k], np.where(err > 0, np.inf, 0.0))))
    i0 = np.abs(w["I"][:, 0])
    sure = i0 > 2 * b["I0"]
    with np.errstate(all="ignore"):
        bt = (b["IH"] + w["thd_i"] * b["I0"]) / (i0 - b["I0"]) + 4 * 2.0 ** -52 * w["thd_i"]
        worst["thd_i"] = float((np.abs(got["thd_i"] - w["thd_i"])[sure] / bt[sure]).max()) if sure.any() else 0.0
    print("\nBRANCH %s: %d scenarios x %d branches x %d harmonics; largest error / bound: %s; thd_i checked on %.1f %% of the branches"
          % (label, U.shape[0], len(fr), Hn, ", ".join("%s %.3g" % kv for kv in worst.items()), 100 * sure.mean()))
    assert max(worst.values()) <= 1.0, worst
    assert (got["loss"] >= 0).all() and (got["irms"] >= 0).all()
    return w, b


def _perturbed(Vm, Va):
    k = np.arange(Vm.shape[1])
    s = np.arange(Vm.shape[0])[:, None]
    return Vm * (1.0 + 0.02 * np.sin(0.7 * s + 0.37 * k)), Va + 1e-3 * np.cos(0.3 * s + 0.11 * k)


@pytest.mark.parametrize("kind", ["radial", "mesh5", "mesh20", "dense"])
def test_branch_flows_after_a_solve_and_after_set_state_alone(tmp_path, kind):
    """S = 1 and S = 37 through one handle: flows at the solved state, then hpf_set_state with OTHER voltages and nothing else -- the flows must be
    those of the new state (the rectangular voltages the kernels read are refreshed), on the block tree (radial, 5 and 20 loop-closing lines: ties
    are branches too) and on the dense solver.  The radial case is the headline feeder: 1 000 buses x 26 harmonics."""
    if kind == "dense":
        net = _feeder(100, 11, tmp_path, seed=1)
    else:
        net = _feeder(1000, 51, tmp_path, ties={"radial": 0, "mesh5": 5, "mesh20": 20}[kind])
    n, Hn = len(net[1]), len(net[0].HARMONICS)
    fr, to, ypos = ref.branches(net[2].rowptr, net[2].col)
    y = ref.series(net[2].Yval, ypos)
    dm = _model(net, 37, solver="dense" if kind == "dense" else "block_tree")
    try:
        assert dm.nb == len(fr) == n - 1 + {"mesh5": 5, "mesh20": 20}.get(kind, 0)
        if kind.startswith("mesh"):
            assert dm.tree_census()["ties"] == int(kind[4:])
        for a, b in zip(dm.branches(), (fr, to, ypos)):
            assert np.array_equal(a, b)
        with pytest.raises(Exception) as nobatch:
            dm.branch_flows()
        for S in (1, 37):
            P, Q = _loads(net[1], S)
            dm.set_loads(P, Q)
            dm.set_state(None, None, n_scen=S)
            dm.fund_pf(1e-6, 30)
            dm.solve(1e-4, 50)
            assert (dm.stats()["flags"] & 1).all()
            Vm, Va = dm.get_state()
            w, b = _check_flows(dm.branch_flows(), fr, to, y, Vm, Va, n, Hn, "%s, after solve, S = %d" % (kind, S))
            if kind == "radial":
                tight = (b["irms"] < 1e-9 * w["irms"]).mean(axis=1)
                print("BRANCH headline: irms bound below 1e-9 irms on %.1f %% of the branches (worst scenario)" % (100 * tight.min()))
                assert (tight >= 0.75).all()
            Vm2, Va2 = _perturbed(Vm, Va)
            dm.set_state(Vm2, Va2)
            got = dm.branch_flows()
            _check_flows(got, fr, to, y, Vm2, Va2, n, Hn, "%s, after set_state alone, S = %d" % (kind, S))
            assert np.abs(got["I"] - w["I"]).max() > 1e3 * b["I"].max()          # (not the solved state's flows)
            assert dm.branch_flows(want_I=False)["I"] is None
    finally:
        dm.close()
    assert nobatch.value.code == -2


@pytest.mark.parametrize("net", ["net1", "net2", "net3"])
def test_line_flows_and_summary_of_the_reference_networks(net):
    import os
    hp = _hp()
    st = hp.Settings(H_MAX=11)
    fb, fl = os.path.join(INPUTS, net + "_buses.csv"), os.path.join(INPUTS, net + "_lines.csv")
    plain = hp.solve(fb, fl, coupled=True, settings=st, ne_dir=INPUTS)
    res = hp.solve(fb, fl, coupled=True, settings=st, ne_dir=INPUTS, line_flows=True)
    assert set(res) - set(plain) == {"line_flows", "line_summary"} and res["V"].equals(plain["V"])
    buses, lines, m, n, c = hp.init_network(fb, fl, settings=st)
    V = res["V"]
    lf, ls = hp.line_flows(V, lines, buses, st), hp.line_summary(V, lines, buses, st)
    assert lf.equals(res["line_flows"]) and ls.equals(res["line_summary"])
    Hn, L = len(st.HARMONICS), len(lines)
    assert list(lf.columns) == ["fromID", "toID", "I_m", "I_a", "loss"] and lf.index.names == ["harmonic", "line"] and len(lf) == Hn * L
    assert list(ls.columns) == ["fromID", "toID", "I_rms", "THD_I", "loss", "loss_harm"] and ls.index.equals(lines.index)
    Y = hp.build_admittance_matrices(buses, lines, st.HARMONICS)
    fr, to, ypos = ref.branches(Y.rowptr, Y.col)
    y = ref.series(Y.Yval, ypos)
    U = ref.rect(V["V_m"].to_numpy()[None], V["V_a"].to_numpy()[None], n, Hn)
    w = ref.flows(fr, to, y, U)
    b = _bounds(fr, to, y, U, w)
    # the lines' own orientation: the branch of the line's bus pair, the sign of its from -> to
    f0, t0 = lines.fromID.to_numpy() - 1, lines.toID.to_numpy() - 1
    e = np.array([int(np.nonzero((fr == min(a, c_)) & (to == max(a, c_)))[0][0]) for a, c_ in zip(f0, t0)])
    sign = np.where(f0 < t0, 1.0, -1.0)
    I_line = w["I"][0][:, e] * sign
    I_got = (lf["I_m"].to_numpy() * np.exp(1j * lf["I_a"].to_numpy())).reshape(Hn, L)
    r_I = np.abs(I_got - I_line) / (b["I"][0][:, e] + 4 * 2.0 ** -52 * np.abs(I_line))          # (+ abs / angle / exp round trip)
    # line_flows forms loss = R |I_dev|^2 with R = Re(y) / |y|^2 on the host: R (2 |I| bI + bI^2) + 8 x 2^-52 loss
    R = y.real / (y.real ** 2 + y.imag ** 2)
    bl = R[None] * (2 * np.abs(w["I"]) * b["I"] + b["I"] ** 2) + 8 * 2.0 ** -52 * w["loss_q"]
    r_l = np.abs(lf["loss"].to_numpy().reshape(Hn, L) - w["loss_q"][0][:, e]) / np.maximum(bl[0][:, e], 1e-300)
    r_s = [np.abs(ls[a].to_numpy() - w[k][0][e]) / b[k][0][e] for a, k in (("I_rms", "irms"), ("loss", "loss"), ("loss_harm", "loss_harm"))]
    print("\nLINES %s: largest error / bound: I %.3g, loss %.3g, I_rms %.3g, loss %.3g, loss_harm %.3g"
          % (net, r_I.max(), r_l.max(), r_s[0].max(), r_s[1].max(), r_s[2].max()))
    assert r_I.max() <= 1 and r_l.max() <= 1 and max(r.max() for r in r_s) <= 1
    assert np.array_equal(lf["fromID"].to_numpy()[:L], lines.fromID.to_numpy()) and (lf["loss"] >= 0).all()
    assert (I_line != 0).any()


def _check_stats(got, Vm, Va, ids, flags, net, rating, label, counts=None, deferred=None):
    """device statistics `got` (BranchStats) against NumPy on the returned voltages"""
    n, Hn = len(net[1]), len(net[0].HARMONICS)
    fr, to, ypos = ref.branches(net[2].rowptr, net[2].col)
    y = ref.series(net[2].Yval, ypos)
    U = ref.rect(Vm, Va, n, Hn)
    fl = ref.flows(fr, to, y, U)
    b = _bounds(fr, to, y, U, fl)
    want = ref.accumulate(fl, ids, flags, ref.thd_ok(Vm, n, Hn), rating, deferred=deferred)
    assert got.counts.tolist() == (want["counts"].tolist() if counts is None else counts), (label, got.counts, want["counts"])
    ok = want["added_mask"]
    added = int(ok.sum())
    if added == 0:
        return want
    x, bx = fl["irms"][ok], b["irms"][ok]
    lo, hi = (x - bx) > rating, (x + bx) > rating                                  # irms (1 -+ D'): D' = the propagated bound
    share = (lo != hi).mean()
    print("\nBRANCHSTATS %s: added %d; over counts %d..%d of %d per branch; bracket ends disagree on %.4f %% of the samples"
          % (label, added, int(lo.sum(0).min()), int(hi.sum(0).max()), added, 100 * share))
    assert share <= 0.01, ("vacuous bracket", share)
    assert (lo.sum(0) <= got.irms_over).all() and (got.irms_over <= hi.sum(0)).all()
    assert 0 < got.irms_over.sum() < x.size                                        # the ratings do cut the samples
    aid = np.asarray(ids)[ok]
    worst = {}
    for pre, key in zip(ref.QUANT, ("irms", "loss", "loss_harm")):
        v, bv = fl[key][ok], b[key][ok]
        g_max, g_arg = getattr(got, pre + "_max"), getattr(got, pre + "_arg")
        top = np.argmax(v, axis=0)
        cols = np.arange(v.shape[1])
        worst[pre + "_max"] = float((np.abs(g_max - want[pre + "_max"]) / np.maximum(bv.max(axis=0), 1e-300)).max())
        assert (np.abs(g_max - want[pre + "_max"]) <= bv.max(axis=0)).all(), pre
        srt = np.sort(v, axis=0)
        clear = np.ones(v.shape[1], bool) if added == 1 else srt[-2] + 2 * bv.max(axis=0) < srt[-1]
        assert np.array_equal(g_arg[clear], aid[top][clear]) and np.isin(g_arg, aid).all(), pre
        if pre == "irms":
            assert clear.mean() > 0.5
        for f, s, bs in ((pre + "_sum", v.sum(0), bv.sum(0)), (pre + "_sumsq", (v * v).sum(0), (2 * v * bv + bv * bv).sum(0))):
            miss = np.abs(getattr(got, f) - want[f]) - (ref.sum_bound(s, added) + bs)
            assert (miss <= 0).all(), (f, float(miss.max()))
    print("BRANCHSTATS %s: largest |max - numpy| / bound: %s" % (label, worst))
    return want


def _rating(Vm, Va, flags, net):
    n, Hn = len(net[1]), len(net[0].HARMONICS)
    fr, to, ypos = ref.branches(net[2].rowptr, net[2].col)
    y = ref.series(net[2].Yval, ypos)
    U = ref.rect(Vm, Va, n, Hn)
    fl = ref.flows(fr, to, y, U)
    good = (np.asarray(flags) & 1) != 0
    mid = np.array([be.midpoint_limit(fl["irms"][good, e]) for e in range(len(fr))])
    # a branch below a no-load subtree carries no current in any scenario (its two buses sit at one potential): its samples are 0 or rounding
    # noise below their own error bound, no rating can cut them and any rating in their range would put every one of them inside the bracket --
    # such a branch (median sample within 1e3 x its bound) gets no rating
    noise = _bounds(fr, to, y, U, fl)["irms"][good].max(axis=0)
    rating = np.where(mid > 1e3 * noise, mid, np.inf)
    assert np.isinf(rating).mean() < 0.15
    return rating


@pytest.fixture(scope="module")
def sweep75(tmp_path_factory):
    """200 buses x harmonics to 27, seed 3, scenarios 0..74 through 32 slots: everything closed (records, voltages -> the ratings), the branch
    statistics open, the distortion accumulator open, both open."""
    from harmonic_power_flow_amd import sweep
    import distortion_emul as de
    net = _feeder(200, 27, tmp_path_factory.mktemp("b200"), seed=3)
    P, Q = _loads(net[1], 75)
    n, Hn = len(net[1]), len(net[0].HARMONICS)
    out = dict(net=net, P=P, Q=Q, n=n, Hn=Hn)
    dm = _model(net, 32)
    try:
        out["off"] = sweep.solve_scenarios(dm, P, Q, want_voltages=True)
        with pytest.raises(Exception) as closed:
            dm.branch_stats_get()
        out["closed"] = closed.value
        out["rating"] = _rating(out["off"][1], out["off"][2], out["off"][0]["flags"], net)
        out["dcfg"] = de.settings_for(out["off"][1], out["off"][0]["flags"], n, Hn, bins=64)
        out["on"] = sweep.solve_scenarios(dm, P, Q, want_voltages=True, branches={"rating": out["rating"]})
        out["dist"] = sweep.solve_scenarios(dm, P, Q, want_voltages=True, distortion=out["dcfg"])
        out["both"] = sweep.solve_scenarios(dm, P, Q, want_voltages=True, distortion=out["dcfg"], branches={"rating": out["rating"]})
    finally:
        dm.close()
    return out


def test_sweep_statistics_match_numpy_on_the_returned_voltages(sweep75):
    s = sweep75
    rec, Vm, Va, stats = s["on"]
    assert stats.added == 75 and stats.counts.tolist() == [75, 0, 0] and len(set(rec["n_iter"])) > 1
    _check_stats(stats, Vm, Va, np.arange(75), rec["flags"], s["net"], s["rating"], "200 x 14, 75 scenarios, 32 slots")
    for a, b in zip(s["off"], s["on"][:3]):
        assert a.tobytes() == b.tobytes()                                          # open only reads
    assert getattr(s["closed"], "code", None) == -2


def test_both_accumulators_open_change_neither(sweep75):
    from harmonic_power_flow_amd import sweep
    s = sweep75
    assert len(s["both"]) == 5 and isinstance(s["both"][3], sweep.DistortionStats) and isinstance(s["both"][4], sweep.BranchStats)
    for a, b in zip(s["off"], s["both"][:3]):
        assert a.tobytes() == b.tobytes()
    for f in sweep.DistortionStats.ARRAYS:                                         # bit for bit, sums included: the same order of arrival
        assert np.array_equal(getattr(s["both"][3], f), getattr(s["dist"][3], f)), f
    for f in sweep.BranchStats.ARRAYS:
        assert np.array_equal(getattr(s["both"][4], f), getattr(s["on"][3], f)), f


@pytest.mark.parametrize("variant", ["waves", "one_slot", "all_slots", "one_group", "chunk2"])
def test_statistics_do_not_depend_on_slots_queue_chunk_or_groups(sweep75, variant):
    from harmonic_power_flow_amd import sweep
    s = sweep75
    dm = _model(s["net"], {"one_slot": 1, "all_slots": 75}.get(variant, 32))
    try:
        if variant == "one_group":
            dm.set_option("scenario_groups", 1)
        if variant == "chunk2":
            dm.set_option("queue_chunk", 2)
        rec, Vm, Va, stats = sweep.solve_scenarios(dm, s["P"], s["Q"], want_voltages=True, refill=variant != "waves",
                                                   branches={"rating": s["rating"]})
    finally:
        dm.close()
    base = s["on"][3]
    assert np.array_equal(Vm, s["on"][1]) and np.array_equal(rec.view(np.uint8), s["on"][0].view(np.uint8))
    for f in EXACT:
        assert np.array_equal(getattr(stats, f), getattr(base, f)), (variant, f)
    _check_stats(stats, Vm, Va, np.arange(75), rec["flags"], s["net"], s["rating"], variant)


def test_reported_scenarios_are_added_exactly_once_by_their_resolve(tmp_path):
    from harmonic_power_flow_amd import sweep
    net = _feeder(100, 27, tmp_path, seed=1)
    P, Q = _loads(net[1], 7)
    dm = _model(net, 3)
    try:
        dm.set_option("pivot_growth_limit_log10", 0)
        rec0, Vm0, Va0 = sweep.solve_scenarios(dm, P, Q, want_voltages=True)
        rating = _rating(Vm0, Va0, rec0["flags"], net)
        dm.branch_stats_begin(rating)
        raw = dm.solve_queue(P, Q)
        st_raw = dm.branch_stats_get()
        dm.branch_stats_end()
        rec, Vm, Va, stats = sweep.solve_scenarios(dm, P, Q, want_voltages=True, branches={"rating": rating})
    finally:
        dm.close()
    assert ((raw["flags"] & 8) == 8).all() and st_raw.counts.tolist() == [0, 0, 7] and (st_raw.irms_arg == -1).all()
    assert stats.counts.tolist() == [7, 0, 7] and ((rec["flags"] & (8 | 16 | 1)) == (8 | 16 | 1)).all()
    want = _check_stats(stats, Vm, Va, np.arange(7), rec["flags"], net, rating, "100 x 14, 7 flagged scenarios re-solved pivoted", counts=[7, 0, 7])
    assert want["counts"].tolist() == [7, 0, 0]


@pytest.mark.parametrize("kind", ["dense", "meshed"])
def test_every_solver_path_adds_after_its_waves_and_the_explicit_add(tmp_path, kind):
    from harmonic_power_flow_amd import sweep
    net = _feeder(100, 11, tmp_path, seed=1) if kind == "dense" else _feeder(100, 27, tmp_path, seed=3, ties=5)
    P, Q = _loads(net[1], 9)
    dm = _model(net, 4, solver="dense" if kind == "dense" else "block_tree")
    try:
        rec0, Vm0, Va0 = sweep.solve_scenarios(dm, P, Q, want_voltages=True)
        rating = _rating(Vm0, Va0, rec0["flags"], net)
        rec, Vm, Va, stats = sweep.solve_scenarios(dm, P, Q, want_voltages=True, branches={"rating": rating})
        # explicit add after a plain solve: ids from first_id, a second add doubles the counts and keeps the smaller ids
        dm.set_loads(P[:4], Q[:4])
        dm.set_state(None, None, n_scen=4)
        dm.fund_pf(1e-6, 30)
        dm.branch_stats_begin(rating)
        with pytest.raises(Exception) as early:
            dm.branch_stats_add(0)
        dm.solve(1e-4, 50)
        sVm, sVa = dm.get_state()
        sfl = dm.stats()["flags"]
        dm.branch_stats_add(1000)
        once = dm.branch_stats_get()
        dm.branch_stats_add(2000)
        twice = dm.branch_stats_get()
        dm.branch_stats_end()
        with pytest.raises(Exception) as closed:
            dm.branch_stats_add(0)
        bad = rating.copy()
        bad[0] = np.nan
        with pytest.raises(Exception) as nan:
            dm.branch_stats_begin(bad)
    finally:
        dm.close()
    assert stats.added == int(((rec["flags"] & 1) != 0).sum()) >= 1 and stats.counts[1] == 9 - stats.added
    _check_stats(stats, Vm, Va, np.arange(9), rec["flags"], net, rating, kind + " handle, 9 scenarios in waves of 4")
    assert early.value.code == -2 and closed.value.code == -2 and nan.value.code == -1
    _check_stats(once, sVm, sVa, 1000 + np.arange(4), sfl, net, rating, kind + ", explicit add, ids 1000..1003")
    assert twice.counts.tolist() == [2 * c for c in once.counts.tolist()] and np.array_equal(twice.irms_arg, once.irms_arg)
    assert np.array_equal(twice.irms_max, once.irms_max) and np.array_equal(twice.irms_over, 2 * once.irms_over)


def test_closed_is_free_a_handle_that_opened_and_closed_equals_a_fresh_one(tmp_path):
    """Records and voltages of a 64-scenario queue run: a fresh handle against one that built its branch table, opened and closed the branch
    statistics and asked for branch flows first -- hash-equal.  (That no branch kernel is launched while closed is shown by the kernel trace of
    tools/sweep_accumulators.py.)"""
    net = _feeder(200, 27, tmp_path, seed=3)
    P, Q = _loads(net[1], 64)

    def run(touch):
        dm = _model(net, 16)
        try:
            if touch:
                dm.branch_stats_begin(None)
                dm.branch_stats_end()
                dm.set_loads(P[:2], Q[:2])
                dm.set_state(None, None, n_scen=2)
                dm.branch_flows()
            rec, Vm, Va = dm.solve_queue(P, Q, want_voltages=True)
        finally:
            dm.close()
        return hashlib.sha256(rec.tobytes() + Vm.tobytes() + Va.tobytes()).hexdigest()
    assert run(False) == run(True)
