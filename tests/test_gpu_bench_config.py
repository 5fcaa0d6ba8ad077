"""GPU parity tests AT THE BENCHMARK CONFIGURATIONS (run with -m gpu on an MI355X).

BASELINE config 4, one GPU's share: gen(1000, seed 0) x harmonics 1..51, coupled, 128 Monte-Carlo load scenarios in ONE handle
-> scenario groups on their own HIP streams (four groups of 32 by default, tile-aligned; three before round 4: the fixture's scenarios
0 / 15 / 16 / 42 / 43 / 85 / 127 sit at tile and group boundaries of both splits), full and ragged 16-scenario tiles in k_leaf_batch / k_sleaf_batch / k_*_back_batch.  Checked
  (i)   bit for bit against single-scenario handles (one group, one scenario per tile) for scenarios at every tile / group
        boundary, and against the same batch run as ONE group;
  (ii)  against oracle fixtures (tests/golden/syn1000_H51_scen.npz, oracle/make_golden_bench.py): the iterate where the
        reference's stop rule (err <= 1e-4) ends is within 1e-6 of the oracle's (what the stop rule itself guarantees, the
        trajectory being solver sensitive: DESIGN.md §1), and the FIXED POINT -- which does not depend on the linear solver --
        within 1e-8 p.u. per harmonic (north_star tolerance), on complex U and on V_m;
  (iii) ragged tiles and the 1 -> 2 -> 3 group boundaries on a smaller feeder with the same block size (S = 17, 24, 40, 56).
BASELINE config 5 (10 000 buses x 49 harmonics, N = 999 998): full size against the oracle fixture
(tests/golden/syn10000_H99_c.npz)."""
import os

import numpy as np
import pytest

from conftest import GOLD, INPUTS, REPO

pytestmark = pytest.mark.gpu
TOL_V = 1e-8


def _hp():
    import harmonic_power_flow_amd as hp
    return hp


def _feeder(hp, n, hmax, tmp_path, seed=0):
    from harmonic_power_flow_amd import synth
    fb, fl = synth.gen(n, seed=seed, outdir=str(tmp_path))
    st = hp.Settings(H_MAX=hmax)
    buses, lines, m, nn, c = hp.init_network(fb, fl, settings=st)
    Y = hp.build_admittance_matrices(buses, lines, st.HARMONICS)
    NE = hp.import_Norton_Equivalents(buses, True, st, INPUTS)
    return st, buses, Y, NE


def _run(hp, st, buses, Y, NE, ids, groups=None, polish=0):
    """pf + hpf_solve of the scenarios `ids` in one handle -> (n_iter, err, Vm, Va[, Vm, Va after `polish` more iterations])"""
    from harmonic_power_flow_amd import api, synth
    n = len(buses)
    P0, Q0 = buses["P"].to_numpy(float), buses["Q"].to_numpy(float)
    dm = api._device_model(buses, Y, NE, True, st.HARMONICS, solver="block_tree", max_scenarios=len(ids))
    try:
        if groups is not None:
            dm.set_option("scenario_groups", groups)
        scale = np.stack([np.ones(n) if s is None else synth.scenario_scale(n, int(s)) for s in ids])   # None: the CSV loads
        dm.set_loads(P0 * scale, Q0 * scale)
        dm.set_state(None, None, n_scen=len(ids))
        dm.fund_pf(1e-6, 30)
        seed = dm.get_state()
        it, err, _ = dm.solve(1e-4, 50)
        Vm, Va = dm.get_state()
        stats = dm.stats()
        out = [it.copy(), err.copy(), Vm, Va, seed, stats]
        if polish:
            dm.mismatch(want_f=False)
            dm.iterate(polish)
            dm.sync()
            out += list(dm.get_state())
    finally:
        dm.close()
    return out


def _U(V):
    return V[:, 0] * np.exp(1j * V[:, 1])


def test_benchmark_configuration_128_scenarios_three_groups(tmp_path):
    hp = _hp()
    g = np.load(os.path.join(GOLD, "syn1000_H51_scen.npz"))
    scen = [int(s) for s in g["scen"]]
    assert scen == [0, 15, 16, 42, 43, 85, 127]
    st, buses, Y, NE = _feeder(hp, 1000, 51, tmp_path)
    S = 128
    it, err, Vm, Va, seed, stats, Vm2, Va2 = _run(hp, st, buses, Y, NE, list(range(S)), polish=3)
    assert (err <= 1e-4).all() and (it < 50).all()
    assert ((stats["flags"] & 1) == 1).all() and (stats["n_iter"] == it).all()
    # (i) bit-identical to single-scenario handles and to the one-group run of the same batch
    for s in scen:
        it1, err1, Vm1, Va1, seed1, _ = _run(hp, st, buses, Y, NE, [s])
        assert it1[0] == it[s], (s, it1[0], it[s])
        assert np.array_equal(seed1[0][0], seed[0][s]) and np.array_equal(seed1[1][0], seed[1][s])
        assert np.array_equal(Vm1[0], Vm[s]) and np.array_equal(Va1[0], Va[s]), "scenario %d differs from its single-scenario solve" % s
    itg, errg, Vmg, Vag, _, _ = _run(hp, st, buses, Y, NE, list(range(S)), groups=1)
    assert np.array_equal(itg, it) and np.array_equal(Vmg, Vm) and np.array_equal(Vag, Va)
    # (ii) oracle fixtures
    worst_stop = worst_fix = 0.0
    for s in scen:
        np.testing.assert_allclose(np.stack([seed[0][s][:1000], seed[1][s][:1000]], 1), g["seed_fund_%d" % s], rtol=0, atol=1e-12)
        assert (seed[0][s][1000:] == 0.1).all() and (seed[1][s][1000:] == 0.0).all()
        eh = g["err_hist_%d" % s]
        d_stop = np.abs(Vm[s] * np.exp(1j * Va[s]) - _U(g["V_stop_%d" % s])).max()
        Uf = _U(g["V_fix_%d" % s])
        d_fix = np.abs(Vm2[s] * np.exp(1j * Va2[s]) - Uf).max()
        # V_m after the HG:545-549 normalisation (|V_m|)
        d_vm = np.abs(np.abs(Vm2[s]) - np.abs(g["V_fix_%d" % s][:, 0])).max()
        print("\nscenario %3d: %d it (oracle %d), err %.2e (oracle %.2e); |dU| at the stop rule %.2e, at the fixed point %.2e, |dVm| %.2e"
              % (s, it[s], int(g["n_iter_%d" % s]), err[s], eh[-1], d_stop, d_fix, d_vm))
        worst_stop, worst_fix = max(worst_stop, d_stop), max(worst_fix, d_fix)
        assert d_stop < 1e-6
        assert d_fix < TOL_V and d_vm < TOL_V
    print("\nS=128, default groups: max|dU| vs oracle at the stop rule %.2e, at the fixed point %.2e" % (worst_stop, worst_fix))
    # (iii) the REFERENCE ITSELF on scenarios 0 and 127 (oracle/make_golden.py scenref<s>: the unmodified hcne_generalized.py with the
    # scenario's loads, 32 / 30 iterations): its final voltages lie 3.7e-10 / 2.7e-10 from the fixed point (it stops at err 4e-7), so
    # the product's fixed point must agree with the reference's own printed result within the north-star tolerance
    for s in (0, 127):
        r = np.load(os.path.join(GOLD, "syn1000_H51_scenref%d.npz" % s), allow_pickle=True)
        np.testing.assert_allclose(np.stack([seed[0][s][:1000], seed[1][s][:1000]], 1), r["V_pf"][:1000], rtol=0, atol=1e-12)
        from harmonic_power_flow_amd.api import _postprocess
        Vm_p, Va_p = _postprocess(Vm2[s], Va2[s])
        d_ref = np.abs(Vm_p * np.exp(1j * Va_p) - _U(r["V_final"])).max()
        d_vm = np.abs(Vm_p - r["V_final"][:, 0]).max()
        print("scenario %3d vs the reference's own run (%d it, err %.2e): %d it here, |dU| %.2e, |dVm| %.2e at the fixed point"
              % (s, int(r["n_iter_h"]), float(r["err_h"]), it[s], d_ref, d_vm))
        assert d_ref < TOL_V and d_vm < TOL_V
        assert abs(it[s] - int(r["n_iter_h"])) <= 6              # (solver-sensitive count: reported, bounded)


@pytest.mark.parametrize("S", [17, 24, 40, 56])
def test_ragged_tiles_and_group_boundaries(S, tmp_path):
    """S = 17: 2 groups (8 + 9); 24: 3 x 8; 40: 13 + 13 + 14 (ragged tiles only); 56: 18 + 19 + 19 (one full + one ragged
    tile per group) on a 300-bus feeder with b = 52 blocks (same kernels as the headline feeder)."""
    hp = _hp()
    st, buses, Y, NE = _feeder(hp, 300, 51, tmp_path, seed=2)
    ids = list(range(S))
    it, err, Vm, Va, seed, stats = _run(hp, st, buses, Y, NE, ids)
    it1, err1, Vm1, Va1, _, _ = _run(hp, st, buses, Y, NE, ids, groups=1)
    assert np.array_equal(it, it1) and np.array_equal(Vm, Vm1) and np.array_equal(Va, Va1)
    for s in sorted({0, 7, 8, 15, 16, S // 3, S // 3 + 1, 2 * S // 3, S - 1}):
        its, errs, Vms, Vas, _, _ = _run(hp, st, buses, Y, NE, [s])
        assert its[0] == it[s]
        assert np.array_equal(Vms[0], Vm[s]) and np.array_equal(Vas[0], Va[s]), "scenario %d of %d" % (s, S)


def test_config5_full_size_vs_oracle_fixture(tmp_path):
    """BASELINE config 5: gen(10000, seed 0), harmonics 1..99 (K = 49, b = 100), coupled, one scenario, against the oracle
    (SuperLU on the 999 998 x 999 998 Jacobian, 45 min on one core; the reference cannot run this size)."""
    path = os.path.join(GOLD, "syn10000_H99_c.npz")
    if not os.path.exists(path):
        pytest.skip("config-5 oracle fixture not generated (oracle/make_golden_bench.py cfg5)")
    hp = _hp()
    g = np.load(path)
    st, buses, Y, NE = _feeder(hp, 10000, 99, tmp_path)
    it, err, Vm, Va, seed, stats, Vm2, Va2 = _run(hp, st, buses, Y, NE, [None], polish=2)
    n, Hn = 10000, 50
    assert Vm.shape[1] == n * Hn == int(g["n"]) * Hn
    assert err[0] <= 1e-4 and it[0] < 50 and (stats["flags"][0] & 1)
    idx = g["idx"]
    np.testing.assert_allclose(np.stack([seed[0][0][idx], seed[1][0][idx]], 1), g["seed_sample"], rtol=0, atol=1e-11)
    U, U2 = Vm[0] * np.exp(1j * Va[0]), Vm2[0] * np.exp(1j * Va2[0])
    d_stop = np.abs(U[idx] - _U(g["V_stop_sample"])).max()
    d_fix = np.abs(U2[idx] - _U(g["V_fix_sample"])).max()
    d_vm = np.abs(np.abs(Vm2[0][idx]) - np.abs(g["V_fix_sample"][:, 0])).max()
    # every entry, in aggregate: per-harmonic sums of |U| at the fixed point (10 000 terms each)
    d_sum = np.abs(np.abs(U2).reshape(Hn, n).sum(1) - g["U_fix_abs_per_harmonic"]).max()
    print("\nconfig 5: %d it (oracle %d) err %.2e; sampled |dU| at the stop rule %.2e, at the fixed point %.2e, |dVm| %.2e; "
          "per-harmonic sum |U| deviation %.2e" % (it[0], int(g["n_iter"]), err[0], d_stop, d_fix, d_vm, d_sum))
    assert d_stop < 1e-6
    assert d_fix < TOL_V and d_vm < TOL_V
    assert d_sum < n * TOL_V * 1e-2


@pytest.mark.parametrize("refill", [True, False])
def test_sweep_in_waves_equals_single_scenario_solves(tmp_path, refill):
    """sweep.solve_scenarios: 75 scenarios through a model sized for 32 live scenarios -- refill=True: hpf_solve_queue (finished scenarios
    harvested between chunks of iterations, their slots refilled from the queue until it drains); refill=False: waves of 32 + 32 + 11 --
    every record and every voltage bit-identical to the scenario solved alone."""
    hp = _hp()
    from harmonic_power_flow_amd import api, sweep, synth
    st, buses, Y, NE = _feeder(hp, 200, 27, tmp_path, seed=3)
    n = len(buses)
    P0, Q0 = buses["P"].to_numpy(float), buses["Q"].to_numpy(float)
    scale = np.stack([synth.scenario_scale(n, s) for s in range(75)])
    dm = api._device_model(buses, Y, NE, True, st.HARMONICS, solver="block_tree", max_scenarios=32)
    try:
        rec, Vm, Va = sweep.solve_scenarios(dm, P0 * scale, Q0 * scale, want_voltages=True, refill=refill)
        rec_nv = sweep.solve_scenarios(dm, P0 * scale, Q0 * scale, refill=refill)                 # records only, same handle again
        few, Vm_few, Va_few = sweep.solve_scenarios(dm, (P0 * scale)[40:45], (Q0 * scale)[40:45], want_voltages=True, refill=refill)   # fewer scenarios than slots
    finally:
        dm.close()
    assert rec.shape == (75,) and ((rec["flags"] & 1) == 1).all()
    assert np.array_equal(rec.view(np.uint8), rec_nv.view(np.uint8))
    assert np.array_equal(few.view(np.uint8), rec[40:45].view(np.uint8)) and np.array_equal(Vm_few, Vm[40:45]) and np.array_equal(Va_few, Va[40:45])
    summ = sweep.summarize(rec.view(np.uint8).reshape(75, 24))
    assert summ["scenarios"] == 75 and summ["converged"] == 75 and summ["iters_total"] == int(rec["n_iter"].sum())
    assert len(set(rec["n_iter"])) > 1                       # (the scenarios do finish at different times: slots are refilled mid-sweep)
    for s in (0, 31, 32, 40, 63, 64, 74):
        it1, err1, Vm1, Va1, _, st1 = _run(hp, st, buses, Y, NE, [s])
        assert rec["n_iter"][s] == it1[0] and rec["err"][s] == err1[0] and rec["thd_max"][s] == st1["thd_max"][0]
        assert rec["flags"][s] == st1["flags"][0]
        assert np.array_equal(Vm[s], Vm1[0]) and np.array_equal(Va[s], Va1[0])


def test_solve_queue_edge_cases(tmp_path):
    """hpf_solve_queue: one scenario in a one-slot handle, a scenario that hits max_iter (reported, its slot is refilled), a queue through a
    DENSE handle (waves), and the handle's per-batch entry points after a queued sweep."""
    hp = _hp()
    from harmonic_power_flow_amd import api, synth
    st, buses, Y, NE = _feeder(hp, 100, 11, tmp_path, seed=1)
    n = len(buses)
    P0, Q0 = buses["P"].to_numpy(float), buses["Q"].to_numpy(float)
    scale = np.stack([synth.scenario_scale(n, s) for s in range(9)])
    ref = {}
    for solver, S_max in (("block_tree", 1), ("block_tree", 4), ("dense", 4)):
        dm = api._device_model(buses, Y, NE, True, st.HARMONICS, solver=solver, max_scenarios=S_max)
        try:
            rec, Vm, Va = dm.solve_queue(P0 * scale, Q0 * scale, want_voltages=True)
            short = dm.solve_queue(P0 * scale, Q0 * scale, max_iter=5)
            with pytest.raises(Exception):
                dm.solve(1e-4, 50)                           # no batch in the handle after a queued sweep
            dm.set_loads(P0 * scale[:1], Q0 * scale[:1])     # ... and the per-batch path works again
            dm.set_state(None, None, n_scen=1)
            dm.fund_pf(1e-6, 30)
            it1, err1, _ = dm.solve(1e-4, 50)
        finally:
            dm.close()
        assert ((rec["flags"] & 1) == 1).all() and it1[0] == rec["n_iter"][0]
        if solver == "block_tree":                           # (DENSE: rocSOLVER's batched and single LU round differently)
            assert err1[0] == rec["err"][0]
        assert (short["n_iter"] == 5).all() and ((short["flags"] & 2) == 2).all() and ((short["flags"] & 1) == 0).all()
        ref[(solver, S_max)] = (rec, Vm, Va)
    a, b, d = ref[("block_tree", 1)], ref[("block_tree", 4)], ref[("dense", 4)]
    assert np.array_equal(a[0].view(np.uint8), b[0].view(np.uint8)) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert np.abs(a[0]["n_iter"] - d[0]["n_iter"]).max() <= 4                                # (solver-sensitive counts on this feeder)
    assert np.abs(a[1] * np.exp(1j * a[2]) - d[1] * np.exp(1j * d[2])).max() < 5e-5        # (dense vs block tree, each at ITS stop: the stop rule is 1e-4)


def test_queue_at_the_benchmark_configuration_equals_the_batch_solve(tmp_path):
    """BASELINE config 4's per-GPU share through hpf_solve_queue: the 128 Monte-Carlo scenarios of the 1 000-bus x 25-harmonic feeder through a
    handle of 48 slots (three scenario groups, slots refilled as scenarios converge) -- every record and every voltage bit-identical to the same
    scenarios solved together in one 128-scenario handle (hpf_solve)."""
    hp = _hp()
    from harmonic_power_flow_amd import api, sweep, synth
    st, buses, Y, NE = _feeder(hp, 1000, 51, tmp_path)
    n, S = len(buses), 128
    P0, Q0 = buses["P"].to_numpy(float), buses["Q"].to_numpy(float)
    scale = np.stack([synth.scenario_scale(n, s) for s in range(S)])
    it, err, Vm, Va, seed, stats = _run(hp, st, buses, Y, NE, list(range(S)))
    dm = api._device_model(buses, Y, NE, True, st.HARMONICS, solver="block_tree", max_scenarios=48)
    try:
        rec, Vq, Aq = sweep.solve_scenarios(dm, P0 * scale, Q0 * scale, want_voltages=True)
    finally:
        dm.close()
    assert np.array_equal(rec["n_iter"], it) and np.array_equal(rec["err"], err)
    assert np.array_equal(rec["flags"], stats["flags"]) and np.array_equal(rec["thd_max"], stats["thd_max"])
    assert np.array_equal(Vq, Vm) and np.array_equal(Aq, Va)


def test_queue_reports_flagged_scenarios_and_the_sweep_resolves_them_with_pivoting(tmp_path):
    """With the pivot-growth limit at 10^0 every scenario is flagged by the static-pivot monitor: hpf_solve_queue reports it (flags bit 3, not
    repeated), sweep.solve_scenarios then solves each flagged scenario alone through hpf_solve, which repeats it with partial pivoting (bit 4) --
    the results equal an explicit block_pivoting = 1 solve bit for bit."""
    hp = _hp()
    from harmonic_power_flow_amd import api, sweep, synth
    st, buses, Y, NE = _feeder(hp, 100, 27, tmp_path, seed=1)
    n, S = len(buses), 7
    P0, Q0 = buses["P"].to_numpy(float), buses["Q"].to_numpy(float)
    scale = np.stack([synth.scenario_scale(n, s) for s in range(S)])
    dm = api._device_model(buses, Y, NE, True, st.HARMONICS, solver="block_tree", max_scenarios=3)
    try:
        dm.set_option("pivot_growth_limit_log10", 0)
        raw = dm.solve_queue(P0 * scale, Q0 * scale)
        rec, Vq, Aq = sweep.solve_scenarios(dm, P0 * scale, Q0 * scale, want_voltages=True)
    finally:
        dm.close()
    assert ((raw["flags"] & 8) == 8).all() and ((raw["flags"] & 16) == 0).all()
    assert ((rec["flags"] & (8 | 16)) == (8 | 16)).all() and ((rec["flags"] & 1) == 1).all()
    for s in (0, 3, 6):
        dm1 = api._device_model(buses, Y, NE, True, st.HARMONICS, solver="block_tree", max_scenarios=1)
        try:
            dm1.set_option("block_pivoting", 1)
            dm1.set_loads(P0 * scale[s], Q0 * scale[s])
            dm1.set_state(None, None, n_scen=1)
            dm1.fund_pf(1e-6, 30)
            it1, err1, _ = dm1.solve(1e-4, 50)
            Vm1, Va1 = dm1.get_state()
        finally:
            dm1.close()
        assert it1[0] == rec["n_iter"][s] and err1[0] == rec["err"][s]
        assert np.array_equal(Vm1[0], Vq[s]) and np.array_equal(Va1[0], Aq[s])


def test_plain_bench_run_times_the_steps_and_dumps_the_state_of_the_last_one(tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR` (a fresh process): ONE timed block of K steps, the headline keys only, and
    DIR/{Vm,Va,err}.npy = the state after W + K Newton iterations from the pf seed, bit for bit what the same iterations give in a handle here."""
    import json
    import subprocess
    import sys
    from harmonic_power_flow_amd import api, synth
    n, hmax, S, K, W = 200, 11, 4, 3, 2
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(K), "--warmup", str(W), "--buses", str(n),
                        "--hmax", str(hmax), "--scenarios", str(S), "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    j = json.loads(r.stdout.strip().splitlines()[-1])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in j, k
    assert j["steps"] == K and j["repeats"] == 1 and len(j["repeat_ms_per_step"]) == 1 and j["ms_per_step"] > 0
    assert abs(j["value"] - S * K / (j["ms_per_step"] * K * 1e-3)) <= 1e-9 * j["value"]
    assert "roofline" not in j and "cpu_baseline" not in j and "sweep" not in j
    hp = _hp()
    st, buses, Y, NE = _feeder(hp, n, hmax, tmp_path)
    P0, Q0 = buses["P"].to_numpy(float), buses["Q"].to_numpy(float)
    scale = np.stack([synth.scenario_scale(n, s) for s in range(S)])
    dm = api._device_model(buses, Y, NE, True, st.HARMONICS, solver="block_tree", max_scenarios=S)
    try:
        dm.set_loads(P0 * scale, Q0 * scale)
        dm.set_state(None, None, n_scen=S)
        dm.fund_pf(st.thresh_f, st.max_iter_f)
        dm.mismatch(want_f=False)
        dm.iterate(W + K)
        dm.sync()
        Vm, Va = dm.get_state()
        _, err = dm.mismatch(want_f=False)
    finally:
        dm.close()
    for name, ref in (("Vm", Vm), ("Va", Va), ("err", err)):
        a = np.load(out / (name + ".npy"))
        assert a.dtype == np.float64 and np.array_equal(a, ref), name
