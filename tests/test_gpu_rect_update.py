"""Rectangular state update of the harmonic Newton loop (option "rectangular_update", include/hpf.h; run with -m gpu on an MI355X).

Shapes: syn100 x harmonics to 11, coupled (6 harmonics, blocks of 12: the smallest the tree kernels instantiate) -- as a radial block tree
(the fast queue), with 2 loop-closing lines (meshed: bordered step, step in the stacked layout) and on the dense solver; 24
synth.scenario_scale scenarios through 8 / 3 slots so that slots refill; one S = 1 solve of the headline feeder syn1000 x harmonics to 51.

Bounds.
One step (test 1): the device's new state, as U = vm' e^(j va'), against tests/update_ref.rect_update applied to the same start x0 and the step
dx recovered from the polar run of the same handle (dx = x0 - x1).  Per entry, in units of eps = 2^-52, relative to |u| + |dU| (>= |U'|):
  4 on u and 4 on dU: the restatement forms u = vm e^(j va) and e = u / vm with NumPy's sin / cos, the device with its own (each within 1 - 2
    ulp, + the products' rounding): both enter U' = u - dU, e through dU = e (dV + j vm dtheta);
  2 + 2: b, two products and a sum per component of dU, rounded on their own on each side (4 x 2^-53 each side);
  1: the subtraction u - dU on each side (2^-53 each);
  1 + 1: vm' = sqrt(re^2 + im^2) on each side (two squares, a sum, a root: 2.5 x 2^-53);
  4 + 2: va' = atan2 within 2 ulp of pi (= 2^-51 each) on the device and 1 ulp in NumPy, turned into |U'| dva' of displacement;
  2 + 2: the test's own vm' e^(j va') of both states (sin / cos 1 ulp, one product);
  = 25, taken as 32.  Added to it, from the operands: the recovered step carries the rounding of x1 = x0 - dx and of x0 - x1,
  |ddV| <= 2^-53 (|vm1| + |dV|), |ddtheta| <= 2^-53 (|va1| + |dtheta|), which moves dU by at most |ddV| + |vm| |ddtheta|.
Everything else is bit for bit (entries with k < c against the polar run, stored U / E against hpf_set_state of the returned state, a scenario
against its solve alone, off against a fresh handle, the polar re-solves against update="polar"), or the project's fixed-point gate 1e-8 on
complex voltages of two solves that both stop at thresh 1e-9, or the iteration bounds of the issue (at most half of the reference update's
iterations; at most 6 for the headline feeder at thresh 1e-4, where the oracle needs 3)."""
import os
import time

import numpy as np
import pytest

from conftest import INPUTS

import update_ref as ref

pytestmark = pytest.mark.gpu
TH = 1e-9
S_SCEN = 24
EPS = 2.0 ** -52
NONSUM_D = ("x_max", "x_arg", "x_over", "thd_max", "thd_arg", "thd_over", "thd_hist")
NONSUM_B = ("irms_max", "irms_arg", "irms_over", "loss_max", "loss_arg", "lossh_max", "lossh_arg")


def _hp():
    import harmonic_power_flow_amd as hp
    return hp


def _net(kind, outdir, n_bus=100, hmax=11):
    """-> (settings, buses, Y, NE, solver, lines)"""
    hp = _hp()
    from harmonic_power_flow_amd import synth
    st = hp.Settings(H_MAX=hmax)
    fb, fl = synth.gen(n_bus, seed=0, outdir=str(outdir))
    if kind == "meshed":
        synth.add_ties(fl, n_bus, 2)
    buses, lines, m, n, c = hp.init_network(fb, fl, settings=st)
    Y = hp.build_admittance_matrices(buses, lines, st.HARMONICS)
    NE = hp.import_Norton_Equivalents(buses, True, st, INPUTS)
    return st, buses, Y, NE, "dense" if kind == "dense" else "block_tree", lines


def _model(net, slots):
    from harmonic_power_flow_amd import api
    st, buses, Y, NE, solver = net[:5]
    return api._device_model(buses, Y, NE, True, st.HARMONICS, solver=solver, max_scenarios=slots)


def _loads(buses, S):
    from harmonic_power_flow_amd import synth
    n = len(buses)
    scale = np.stack([synth.scenario_scale(n, s) for s in range(S)])
    return buses["P"].to_numpy(float) * scale, buses["Q"].to_numpy(float) * scale


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _u(Vm, Va):
    return Vm * np.exp(1j * Va)


def _seed(dm, P, Q):
    """flat start + pf of the scenarios P, Q -> (Vm, Va) of the batch"""
    dm.set_loads(P, Q)
    dm.set_state(None, None, n_scen=np.atleast_2d(P).shape[0])
    dm.fund_pf(1e-6, 30)
    return dm.get_state()


@pytest.fixture(scope="module")
def radial(tmp_path_factory):
    """the radial feeder and its 24 scenarios through 8 slots, option on (thresh 1e-9, voltages kept), and the same sweep with the option off"""
    net = _net("radial", tmp_path_factory.mktemp("syn100"))
    P, Q = _loads(net[1], S_SCEN)
    dm = _model(net, 8)
    try:
        assert dm.solver == "block_tree" and dm.tree_census()["ties"] == 0
        polar = dm.solve_queue(P, Q, thresh=TH, want_voltages=True)
        dm.set_option("rectangular_update", 1)
        rect = dm.solve_queue(P, Q, thresh=TH, want_voltages=True)
    finally:
        dm.close()
    return dict(net=net, n=len(net[1]), Hn=len(net[0].HARMONICS), P=P, Q=Q, polar=polar, rect=rect)


# ---- 1. one step -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["dense", "radial", "meshed"])
def test_one_step_is_the_restatement_of_the_polar_step(tmp_path, kind):
    net = _net(kind, tmp_path)
    n, Hn = len(net[1]), len(net[0].HARMONICS)
    P, Q = _loads(net[1], 2)
    dm = _model(net, 2)
    try:
        assert dm.solver == net[4] and (kind != "meshed" or dm.tree_census()["ties"] == 2)
        c = dm.c
        x0 = _seed(dm, P, Q)
        dm.solve(TH, 1)
        x1, st_p = dm.get_state(), dm.stats()
        dm.set_option("rectangular_update", 1)
        dm.set_state(*x0)
        dm.solve(TH, 1)
        xr, st_r = dm.get_state(), dm.stats()
        # stored U, E = those of hpf_set_state(returned state): the second step of a two-step solve (which reads the stored ones) against a
        # one-step solve from the returned state (which forms them anew)
        dm.set_state(*x0)
        dm.solve(TH, 2)
        two = dm.get_state()
        dm.set_state(*xr)
        dm.solve(TH, 1)
        split = dm.get_state()
    finally:
        dm.close()
    assert (st_p["n_iter"] == 1).all() and (st_r["n_iter"] == 1).all()
    assert not (st_p["flags"] & 512).any() and (st_r["flags"] & 512).all()
    k = np.arange(n * Hn)
    worst = 0.0
    for s in range(2):
        vm, va = x0[0][s], x0[1][s]
        dth = np.where(k >= 1, va - x1[1][s], 0.0)
        dv = np.where(k >= c, vm - x1[0][s], 0.0)
        u = vm * np.cos(va) + 1j * (vm * np.sin(va))
        e = u * (1.0 / vm)
        vm_r, va_r, tre, tim = ref.rect_update(vm, va, u, e, k, c, dth, dv)
        low = k < c
        assert xr[0][s][low].tobytes() == x1[0][s][low].tobytes() and xr[1][s][low].tobytes() == x1[1][s][low].tobytes()
        assert (xr[0][s][~low] >= 0).all()
        dU = np.hypot(dv, vm * dth)
        step_err = 2.0 ** -53 * ((np.abs(x1[0][s]) + np.abs(dv)) + np.abs(vm) * (np.abs(x1[1][s]) + np.abs(dth)))
        bound = 32 * EPS * (np.abs(u) + dU) + step_err
        got = np.abs(_u(xr[0][s], xr[1][s]) - _u(vm_r, va_r))
        worst = max(worst, float((got[~low] / bound[~low]).max()))
        assert (got[~low] <= bound[~low]).all(), (kind, s, float((got[~low] / bound[~low]).max()))
    print("\nRECT UPDATE one step, %s: largest observed / bound %.3f (largest harmonic |dtheta| of the step %.2f rad)"
          % (kind, worst, float(np.abs(dth[n:]).max())))
    assert _same(two, split)


# ---- 2. convergence ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["radial", "dense"])
def test_converges_in_at_most_half_the_iterations_to_the_same_voltages(tmp_path, kind):
    net = _net(kind, tmp_path)
    P, Q = _loads(net[1], 4)
    dm = _model(net, 4)
    res = {}
    try:
        assert dm.solver == net[4]
        for on in (0, 1):
            dm.set_option("rectangular_update", on)
            _seed(dm, P, Q)
            dm.solve(TH, 50)
            res[on] = (dm.stats(), ) + dm.get_state()
    finally:
        dm.close()
    du = float(np.abs(_u(*res[1][1:]) - _u(*res[0][1:])).max())
    print("\nRECT UPDATE %s: iterations off %s, on %s, |dU| %.3e" % (kind, res[0][0]["n_iter"].tolist(), res[1][0]["n_iter"].tolist(), du))
    assert ((res[0][0]["flags"] & (1 | 512)) == 1).all()
    assert ((res[1][0]["flags"] & (1 | 512)) == (1 | 512)).all()
    assert (2 * res[1][0]["n_iter"] <= res[0][0]["n_iter"]).all()
    assert du <= 1e-8


def test_the_headline_feeder_converges_in_a_handful_of_iterations(tmp_path):
    """syn1000 x harmonics to 51, one scenario (scenario_scale 127, the oracle's case: 3 iterations), thresh 1e-4: at most 6"""
    from harmonic_power_flow_amd import synth
    t0 = time.perf_counter()
    net = _net("radial", tmp_path, n_bus=1000, hmax=51)
    n = len(net[1])
    scale = synth.scenario_scale(n, 127)
    dm = _model(net, 1)
    t_build = time.perf_counter() - t0
    try:
        dm.set_option("rectangular_update", 1)
        _seed(dm, net[1]["P"].to_numpy(float) * scale, net[1]["Q"].to_numpy(float) * scale)
        _, _, hist = dm.solve(1e-4, 50)
        st = dm.stats()[0]
    finally:
        dm.close()
    print("\nRECT UPDATE syn1000 H51 scenario 127: %d iterations (%s), fixture + handle %.2f s"
          % (st["n_iter"], " -> ".join("%.1e" % e for e in hist[0][:st["n_iter"] + 1]), t_build))
    assert (st["flags"] & (1 | 512)) == (1 | 512)
    assert st["n_iter"] <= 6


# ---- 3. slot independence ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["alone", "slots3_chunk4_groups2", "slots8_chunk1_groups1", "slots3_chunk1_groups1", "slots8_chunk4_groups2"])
def test_a_scenario_does_not_depend_on_its_company(radial, variant):
    r = radial
    slots = 3 if "slots3" in variant else 8
    dm = _model(r["net"], slots)
    try:
        dm.set_option("rectangular_update", 1)
        if variant == "alone":
            rec, Vm, Va = r["rect"][0].copy(), np.empty_like(r["rect"][1]), np.empty_like(r["rect"][2])
            for s in range(S_SCEN):
                _seed(dm, r["P"][s], r["Q"][s])
                dm.solve(TH, 50)
                rec[s] = dm.stats()[0]
                Vm[s], Va[s] = (a[0] for a in dm.get_state())
            got = (rec, Vm, Va)
        else:
            dm.set_option("queue_chunk", 1 if "chunk1" in variant else 4)
            dm.set_option("scenario_groups", 1 if "groups1" in variant else 2)
            got = dm.solve_queue(r["P"], r["Q"], thresh=TH, want_voltages=True)
    finally:
        dm.close()
    assert ((got[0]["flags"] & (1 | 512)) == (1 | 512)).all()
    assert _same(got, r["rect"]), variant


def test_the_queue_converges_in_at_most_half_the_iterations(radial):
    polar, rect = radial["polar"], radial["rect"]
    du = float(np.abs(_u(*rect[1:]) - _u(*polar[1:])).max())
    print("\nRECT UPDATE queue: iterations off %s (total %d), on %s (total %d), |dU| %.3e"
          % (polar[0]["n_iter"].tolist(), polar[0]["n_iter"].sum(), rect[0]["n_iter"].tolist(), rect[0]["n_iter"].sum(), du))
    assert (2 * rect[0]["n_iter"] <= polar[0]["n_iter"]).all() and du <= 1e-8


# ---- 4. off is off ---------------------------------------------------------------------------------------------------------------------------
def test_off_is_off(radial):
    r = radial
    dm = _model(r["net"], 8)
    try:
        dm.set_option("rectangular_update", 1)
        dm.set_option("rectangular_update", 0)
        again = dm.solve_queue(r["P"], r["Q"], thresh=TH, want_voltages=True)
        _seed(dm, r["P"][:3], r["Q"][:3])
        dm.solve(TH, 50)
        batch = (dm.stats(), ) + dm.get_state()
    finally:
        dm.close()
    assert _same(again, r["polar"]) and not (again[0]["flags"] & 512).any()
    assert not (batch[0]["flags"] & 512).any()
    for j in range(3):
        assert all(batch[i][j].tobytes() == r["polar"][i][j].tobytes() for i in range(3))


def test_a_cached_handle_does_not_keep_the_mode(tmp_path):
    """hp.hpf of the golden row syn100_H11_c, then solve_scenarios(update="rectangular") and hp.hpf(update="rectangular") on the SAME cached
    handle, then hp.hpf again: byte-identical to the first call, and the golden row's iteration count"""
    hp = _hp()
    from harmonic_power_flow_amd import api, sweep, synth
    g = np.load(os.path.join(os.path.dirname(INPUTS), "syn100_H11_c.npz"), allow_pickle=True)
    st = hp.Settings(H_MAX=11)
    fb, fl = synth.gen(100, seed=0, outdir=str(tmp_path))
    buses, lines, m, n, c = hp.init_network(fb, fl, settings=st)

    def row(**kw):
        det = {}
        _, err_h, n_iter_h, _ = hp.hpf(buses, lines, True, settings=st, ne_dir=INPUTS, verbose=False, return_jacobian=False, details=det, **kw)
        return n_iter_h, err_h, det["Vm_raw"].tobytes(), det["Va_raw"].tobytes(), int(det["stats"]["flags"][0])

    hp.handle_cache(4)
    before = row()
    s0 = hp.handle_cache()
    Y = hp.build_admittance_matrices(buses, lines, st.HARMONICS)
    NE = hp.import_Norton_Equivalents(buses, True, st, INPUTS)
    P, Q = _loads(buses, 3)
    with api._borrow_model(buses, Y, NE, True, st.HARMONICS) as dm:
        rec = sweep.solve_scenarios(dm, P, Q, thresh_h=TH, update="rectangular")
    rect = row(update="rectangular")
    after = row()
    assert hp.handle_cache()["hits"] - s0["hits"] == 3            # the same handle all along
    assert ((rec["flags"] & (1 | 512)) == (1 | 512)).all()
    assert (rect[4] & (1 | 512)) == (1 | 512) and 2 * rect[0] <= before[0]
    assert before[0] == int(g["n_iter_h"]) and not (before[4] & 512)
    assert after == before


# ---- 5. fallback ---------------------------------------------------------------------------------------------------------------------------
def test_what_does_not_converge_is_deferred_and_solved_again_with_the_polar_update(radial):
    """max_iter_h = 1: nothing converges in one step from the flat start.  The queue with the option on reports every scenario with bits 9
    and 1 and both accumulators defer all 24; solve_scenarios(update="rectangular") then solves each again with the reference's update, and
    its records, voltages and accumulators are those of solve_scenarios(update="polar") with the same cap, bit for bit, without bit 9.  (The
    deferred counter is the one field that cannot agree: it counts the scenarios that were solved twice, 24 here and none in the polar sweep.
    Neither sweep adds a scenario -- one iteration converges nothing --, so both skip all 24.)"""
    from harmonic_power_flow_amd import sweep
    r = radial
    cfg = {"limit": None, "thd_limit": 0.05, "hist_max": 1.0, "bins": 16}
    dm = _model(r["net"], 8)
    try:
        dm.set_option("rectangular_update", 1)
        dm.distortion_begin(None, 0.05, 1.0, 16)
        dm.branch_stats_begin(None)
        first = dm.solve_queue(r["P"], r["Q"], max_iter=1)
        dist, br = dm.distortion_get(), dm.branch_stats_get()
        dm.distortion_end()
        dm.branch_stats_end()
        dm.set_option("rectangular_update", 0)
        res = [sweep.solve_scenarios(dm, r["P"], r["Q"], max_iter_h=1, want_voltages=True, distortion=cfg, branches={"rating": None}, update=u)
               for u in ("polar", "rectangular")]
    finally:
        dm.close()
    assert ((first["flags"] & (512 | 2 | 1)) == (512 | 2)).all() and (first["n_iter"] == 1).all()
    assert dist.counts.tolist() == [0, 0, S_SCEN] and br.counts.tolist() == [0, 0, S_SCEN]
    polar, rect = res
    assert not (rect[0]["flags"] & 512).any() and ((rect[0]["flags"] & 3) == 2).all()
    assert _same(rect[:3], polar[:3])
    for k, names in ((3, NONSUM_D), (4, NONSUM_B)):
        assert polar[k].counts.tolist() == [0, S_SCEN, 0] and rect[k].counts.tolist() == [0, S_SCEN, S_SCEN]
        for f in names:
            assert np.array_equal(getattr(rect[k], f), getattr(polar[k], f)), f


# ---- 6. with a start -------------------------------------------------------------------------------------------------------------------------
def test_with_a_start_state(radial):
    from harmonic_power_flow_amd import sweep
    r = radial
    dm = _model(r["net"], 8)
    try:
        warm = sweep.solve_scenarios(dm, r["P"], r["Q"], thresh_h=TH, want_voltages=True, start="mean", update="rectangular")
        assert not dm.has_start()
        off = dm.solve_queue(r["P"][:2], r["Q"][:2], thresh=TH)       # (the option is back to off)
    finally:
        dm.close()
    du = float(np.abs(_u(*warm[1:]) - _u(*r["polar"][1:])).max())
    print("\nRECT UPDATE warm: iterations %s, |dU| against the cold polar sweep %.3e" % (warm[0]["n_iter"].tolist(), du))
    assert ((warm[0]["flags"] & (1 | 256 | 512)) == (1 | 256 | 512)).all()
    assert du <= 1e-8
    assert off.tobytes() == r["polar"][0][:2].tobytes()


# ---- 7. bad values ---------------------------------------------------------------------------------------------------------------------------
def test_bad_values_are_refused(radial):
    hp = _hp()
    from harmonic_power_flow_amd import sweep
    r = radial
    dm = _model(r["net"], 2)
    try:
        for bad in (2, -1):
            assert dm.lib.hpf_set_option(dm._h, b"rectangular_update", bad) == -1
        assert dm.lib.hpf_set_option(dm._h, b"rectangular_update", 1) == 0 and dm.lib.hpf_set_option(dm._h, b"rectangular_update", 0) == 0
        for bad in ("cartesian", None, 1):
            with pytest.raises(ValueError):
                sweep.solve_scenarios(dm, r["P"][:2], r["Q"][:2], update=bad)
        st, buses, lines = r["net"][0], r["net"][1], r["net"][5]
        with pytest.raises(ValueError):
            hp.hpf(buses, lines, True, settings=st, ne_dir=INPUTS, verbose=False, update="Rectangular")
        rec = dm.solve_queue(r["P"][:2], r["Q"][:2], thresh=TH)
    finally:
        dm.close()
    assert rec.tobytes() == r["polar"][0][:2].tobytes()            # nothing of the refused calls stuck
    assert dm.lib.hpf_version() >= 101
