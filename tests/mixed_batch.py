"""Batches whose scenarios end differently from each other (tests/test_gpu_mixed_batches.py): the compositions and the comparison helpers.
Test infrastructure only.

A batch is a string of scenario kinds, one letter per slot.  Scenario s has the loads P0 * synth.scenario_scale(n, s) (times gscale[s]) and
  B  enters at its own converged state (a default solve of the same loads + two more Newton iterations): under thresh at the first mismatch, so
     the first k_finalize never activates it -- n_iter 0, flags bit 0 only, err_hist = [e0, NaN, ...], state untouched, eta NaN;
  A  enters at the pf seed and is run on a handle with pivot_growth_limit_log10 = 0, where every scenario that takes a step is flagged;
  C  enters at the pf seed (iters[s] > 0: at the state after that many default iterations) under the default limit;
  N  enters at the pf seed of the clean loads with P[s][i] = NaN at one load bus i: its first mismatch is NaN, it is inactive from the first
     k_finalize of every pass and no factorisation ever sees it.
A and C are the same scenario; what differs is the handle they run on."""
import numpy as np

from conftest import INPUTS

import branch_ref as bref
import distortion_ref as dref

THRESH, MAX_ITER = 1e-4, 50
N_BUS, SEED, H_MAX = 90, 0, 27
MODE_BITS = 256 | 512 | 1024                 # start state, rectangular update, per-scenario sources: how a record was made, not how it ended
D = 2.0 ** -49                               # the 8-ulp allowance of tests/test_gpu_distortion.py for the device's sqrt / division / sincos


def feeder(outdir, ties=0):
    import harmonic_power_flow_amd as hp
    from harmonic_power_flow_amd import synth
    fb, fl = synth.gen(N_BUS, seed=SEED, outdir=str(outdir))
    if ties:
        synth.add_ties(fl, N_BUS, ties)
    st = hp.Settings(H_MAX=H_MAX)
    buses, lines, m, n, c = hp.init_network(fb, fl, settings=st)
    Y = hp.build_admittance_matrices(buses, lines, st.HARMONICS)
    NE = hp.import_Norton_Equivalents(buses, True, st, INPUTS)
    return dict(st=st, buses=buses, Y=Y, NE=NE, n=n, Hn=len(st.HARMONICS), P0=buses["P"].to_numpy(float), Q0=buses["Q"].to_numpy(float),
                cache={})


def model(net, slots, solver="block_tree", opts=()):
    from harmonic_power_flow_amd import api
    dm = api._device_model(net["buses"], net["Y"], net["NE"], True, net["st"].HARMONICS, solver=solver, max_scenarios=slots)
    try:
        for k, v in opts:
            dm.set_option(k, v)
    except Exception:
        dm.close()
        raise
    return dm


def nan_bus(net, m):
    """the first load bus behind the slack: a linear bus (index < m) with P0 != 0"""
    return 1 + int(np.nonzero(net["P0"][1:m])[0][0])


def compose(net, kinds, solver="block_tree", iters=None, gscale=None):
    """-> the batch: P, Q [S][n] (NaN already placed), entering state Vm, Va [S][Hn*n], kinds [S].  One default handle of `solver` prepares the
    states; cached per feeder."""
    from harmonic_power_flow_amd import synth
    key = (kinds, solver, None if iters is None else tuple(iters), None if gscale is None else tuple(gscale))
    if key in net["cache"]:
        return net["cache"][key]
    k = np.array(list(kinds))
    S, n = len(k), net["n"]
    scale = np.stack([synth.scenario_scale(n, s) for s in range(S)])
    if gscale is not None:
        scale = scale * np.asarray(gscale, dtype=np.float64)[:, None]
    P, Q = net["P0"] * scale, net["Q0"] * scale
    dm = model(net, S, solver)
    try:
        dm.set_loads(P, Q)
        dm.set_state(None, None, n_scen=S)
        dm.fund_pf(1e-6, 30)
        states = [dm.get_state()]
        if iters is not None and max(iters) > 0:
            dm.mismatch(want_f=False)
            for _ in range(max(iters)):
                dm.iterate(1)
                dm.sync()
                states.append(dm.get_state())
            dm.set_state(*states[0])
        conv = None
        if (k == "B").any():
            _, err, _ = dm.solve(THRESH, MAX_ITER)
            assert (err[k == "B"] <= THRESH).all(), ("the feeder does not converge", err)
            dm.mismatch(want_f=False)
            dm.iterate(2)
            dm.sync()
            conv = dm.get_state()
        bus = nan_bus(net, dm.m)
    finally:
        dm.close()
    Vm, Va = states[0][0].copy(), states[0][1].copy()
    for s in range(S):
        if k[s] == "B":
            Vm[s], Va[s] = conv[0][s], conv[1][s]
        elif iters is not None:
            Vm[s], Va[s] = states[iters[s]][0][s], states[iters[s]][1][s]
    P[k == "N", bus] = np.nan
    b = dict(P=P, Q=Q, Vm=Vm, Va=Va, kinds=k, S=S, bus=bus)
    net["cache"][key] = b
    return b


def where(b, kind):
    return np.nonzero(b["kinds"] == kind)[0]


def solve_on(dm, b, idx=None, max_iter=MAX_ITER, trace=False, eta=False, jac_of=(), accum=False):
    """scenarios idx of batch b on handle dm: loads, entering state, first mismatch e0, hpf_solve -> every output as a dict (a non-zero return
    code of hpf_solve, HPF_E_SINGULAR included, raises)"""
    idx = np.arange(b["S"]) if idx is None else np.asarray(idx)
    dm.set_loads(b["P"][idx], b["Q"][idx])
    dm.set_state(b["Vm"][idx], b["Va"][idx])
    _, e0 = dm.mismatch(want_f=False)
    if accum:
        dm.distortion_begin()
        dm.branch_stats_begin()
    res = dm.solve(THRESH, max_iter, trace=trace)
    out = dict(it=res[0], err=res[1], hist=res[2], e0=e0, stats=dm.stats())
    if trace:
        out["Vt"], out["At"] = res[3], res[4]
    if accum:
        dm.distortion_add(0)
        dm.branch_stats_add(0)
        out["dist"], out["br"] = dm.distortion_get(), dm.branch_stats_get()
        dm.distortion_end()
        dm.branch_stats_end()
    out["Vm"], out["Va"] = dm.get_state()
    if eta:
        out["eta_last"], out["eta_max"] = dm.step_residuals()
    out["jac"] = {int(s): dm.jacobian_csr(int(s), last=True).data.copy() for s in jac_of}
    return out


def run(net, b, opts=(), solver="block_tree", **kw):
    dm = model(net, b["S"], solver, opts)
    try:
        return solve_on(dm, b, **kw)
    finally:
        dm.close()


def run_alone(net, b, idx, opts=(), solver="block_tree", **kw):
    """each scenario of idx alone on ONE handle of one slot -> {s: outputs}"""
    dm = model(net, 1, solver, opts)
    try:
        return {int(s): solve_on(dm, b, [int(s)], **kw) for s in idx}
    finally:
        dm.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(-1).view(np.uint64)


def assert_same(x, y, s, t=None, what=""):
    """scenario s of run x and scenario t of run y: n_iter, err, the whole err_hist row (NaN tail), Vm, Va, thd_max -- bit for bit"""
    t = s if t is None else t
    assert x["it"][s] == y["it"][t], (what, s, x["it"][s], y["it"][t])
    assert x["stats"]["n_iter"][s] == y["stats"]["n_iter"][t] == x["it"][s], (what, s)
    for k in ("err", "hist", "Vm", "Va"):
        assert np.array_equal(bits(x[k][s]), bits(y[k][t])), (what, k, s)
    assert np.array_equal(bits(x["stats"]["thd_max"][s]), bits(y["stats"]["thd_max"][t])), (what, "thd_max", s)
    assert np.array_equal(bits(x["stats"]["err"][s]), bits(x["err"][s])), (what, "record err", s)


def assert_untouched(r, b, s, t=None):
    t = s if t is None else t
    assert np.array_equal(bits(r["Vm"][t]), bits(b["Vm"][s])) and np.array_equal(bits(r["Va"][t]), bits(b["Va"][s])), ("state moved", s)


def check_B(r, b, s, t=None, eta=False):
    """enters converged: never activated"""
    t = s if t is None else t
    assert r["e0"][t] <= THRESH, ("B does not enter converged", s, r["e0"][t])
    assert r["it"][t] == 0 and r["stats"]["n_iter"][t] == 0, (s, r["it"][t])
    assert (r["stats"]["flags"][t] & ~MODE_BITS) == 1, (s, r["stats"]["flags"][t])
    assert bits(r["err"][t])[0] == bits(r["e0"][t])[0] == bits(r["hist"][t, 0])[0], (s, r["err"][t], r["e0"][t], r["hist"][t, 0])
    assert np.isnan(r["hist"][t, 1:]).all(), (s, r["hist"][t])
    assert_untouched(r, b, s, t)
    if eta:
        assert np.isnan(r["eta_last"][t]) and np.isnan(r["eta_max"][t]), (s, r["eta_last"][t], r["eta_max"][t])


def check_N(r, b, s, repeated, t=None):
    """non-finite from the first mismatch: reported with bit 2 (and bit 4 where hpf_solve repeats), never activated"""
    t = s if t is None else t
    assert np.isnan(r["e0"][t]) and np.isnan(r["err"][t]) and np.isnan(r["stats"]["err"][t]), (s, r["e0"][t], r["err"][t])
    assert r["it"][t] == 0 and r["stats"]["n_iter"][t] == 0, (s, r["it"][t])
    assert (r["stats"]["flags"][t] & ~MODE_BITS) == (4 | (16 if repeated else 0)), (s, r["stats"]["flags"][t])
    assert np.isnan(r["hist"][t]).all(), (s, r["hist"][t])
    assert_untouched(r, b, s, t)
    assert np.isfinite(r["stats"]["thd_max"][t])


# ---- the accumulators against tests/distortion_ref.py / tests/branch_ref.py on the returned voltages, under the rules of tests/test_gpu_distortion.py
# and tests/test_gpu_branch.py: counts exact; max within the allowance for the device's last bits; arg exact wherever the yardstick's runner-up
# is clearly below its maximum, and always the id of an added scenario (no limits are set here: every `over` array stays zero)

def _check_max_arg(g_max, g_arg, v, bound, aid, label):
    assert (np.abs(g_max - v.max(axis=0)) <= bound).all(), label
    srt = np.sort(v, axis=0)
    clear = np.ones(g_max.shape, bool) if v.shape[0] == 1 else srt[-2] + 2 * bound < srt[-1]
    want = aid[np.argmax(v, axis=0)]
    assert np.array_equal(g_arg[clear], want[clear]) and np.isin(g_arg, aid).all(), label
    return float(clear.mean())


def check_distortion(got, Vm, ids, flags, n, Hn, counts=None, deferred=None):
    want = dref.accumulate(Vm, ids, flags, n, Hn, deferred=deferred)
    if counts is not None:
        assert got.counts.tolist() == list(counts), (got.counts, counts)
    ok = want["added_mask"]
    assert got.counts[0] == ok.sum(), (got.counts, ok.sum())
    if not ok.any():
        assert (got.x_arg == -1).all() and (got.thd_arg == -1).all()
        return
    aid = np.asarray(ids)[ok]
    cx = _check_max_arg(got.x_max, got.x_arg, want["x"], D * want["x"].max(axis=0), aid, "x")
    ct = _check_max_arg(got.thd_max, got.thd_arg, want["thd"], D * want["thd"].max(axis=0), aid, "thd")
    print("\nMIXED distortion: added %d, arg compared exactly on %.3f (x) %.3f (thd) of the entries" % (ok.sum(), cx, ct))
    assert (got.thd_hist.sum(axis=1) == ok.sum()).all() and not got.x_over.any() and not got.thd_over.any()


def check_branches(got, dm_arrays, Vm, Va, ids, flags, n, Hn, counts=None, deferred=None):
    rowptr, col, Yval = dm_arrays
    fr, to, ypos = bref.branches(rowptr, col)
    y = bref.series(np.asarray(Yval).reshape(Hn, -1), ypos)
    U = bref.rect(Vm, Va, n, Hn)
    fl = bref.flows(fr, to, y, U)
    want = bref.accumulate(fl, ids, flags, bref.thd_ok(Vm, n, Hn), deferred=deferred)
    if counts is not None:
        assert got.counts.tolist() == list(counts), (got.counts, counts)
    ok = want["added_mask"]
    assert got.counts[0] == ok.sum(), (got.counts, ok.sum())
    if not ok.any():
        assert (got.irms_arg == -1).all()
        return
    # the derived bounds of tests/test_gpu_branch.py (its module docstring)
    aU = np.abs(U)
    bd = D * (aU[:, :, fr] + aU[:, :, to])
    bI = D * (np.abs(y)[None] * (aU[:, :, fr] + aU[:, :, to]) + np.abs(fl["I"]))
    bl = y.real[None] * (2 * np.abs(fl["d"]) * bd + bd * bd) + 4 * 2.0 ** -53 * fl["loss_q"]
    bound = {"irms": np.sqrt((bI * bI).sum(axis=1)) + (Hn + 2) * 2.0 ** -53 * fl["irms"],
             "loss": bl.sum(axis=1) + Hn * 2.0 ** -53 * fl["loss"],
             "loss_harm": bl[:, 1:].sum(axis=1) + Hn * 2.0 ** -53 * fl["loss_harm"]}
    aid = np.asarray(ids)[ok]
    for pre, key in zip(bref.QUANT, ("irms", "loss", "loss_harm")):
        _check_max_arg(getattr(got, pre + "_max"), getattr(got, pre + "_arg"), fl[key][ok], bound[key][ok].max(axis=0), aid, pre)
    assert not got.irms_over.any()
