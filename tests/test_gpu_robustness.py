"""Robustness of the block-tree path (run with -m gpu): the static-pivot monitor and the automatic repeat with partial
pivoting, the per-iteration state dump, the tree-build variants behind the diagnostic environment switches, and a randomised
feeder sweep with the north-star criterion (converged voltages within 1e-8 p.u. of the dense rocSOLVER path / the oracle)."""
import os

import numpy as np
import pytest

import hpf_oracle as o
from conftest import GOLD, INPUTS

pytestmark = pytest.mark.gpu
TOL_V = 1e-8


def _hp():
    import harmonic_power_flow_amd as hp
    return hp


def _feeder(hp, n, hmax, tmp_path, seed=0, frac_nl=0.35, n_pv=0):
    from harmonic_power_flow_amd import synth
    fb, fl = synth.gen(n, seed=seed, frac_nl=frac_nl, outdir=str(tmp_path))
    if n_pv:
        rows = open(fb).read().splitlines()
        for bid in range(2, 2 + n_pv):
            cols = rows[bid].split(";")
            cols[1], cols[2], cols[4], cols[5] = "PV", "gen_%d" % bid, "-120", "0"
            rows[bid] = ";".join(cols)
        open(fb, "w").write("\n".join(rows) + "\n")
    st = hp.Settings(H_MAX=hmax)
    buses, lines, m, nn, c = hp.init_network(fb, fl, settings=st)
    Y = hp.build_admittance_matrices(buses, lines, st.HARMONICS)
    NE = hp.import_Norton_Equivalents(buses, True, st, INPUTS)
    return st, buses, Y, NE, (fb, fl)


def _solve(hp, st, buses, Y, NE, solver="block_tree", S=1, options=(), seed_state=None, polish=0, thresh=1e-4):
    from harmonic_power_flow_amd import api, synth
    n = len(buses)
    dm = api._device_model(buses, Y, NE, True, st.HARMONICS, solver=solver, max_scenarios=S)
    try:
        for k, v in options:
            dm.set_option(k, v)
        P0, Q0 = buses["P"].to_numpy(float), buses["Q"].to_numpy(float)
        scale = np.stack([np.ones(n)] + [synth.scenario_scale(n, s) for s in range(1, S)])
        dm.set_loads(P0 * scale, Q0 * scale)
        dm.set_state(None, None, n_scen=S)
        dm.fund_pf(1e-6, 30)
        if seed_state is not None:
            dm.set_state(*seed_state)
        seed = dm.get_state()
        it, err, hist = dm.solve(thresh, 50)
        st_ = dm.stats()
        if polish:
            dm.mismatch(want_f=False)
            dm.iterate(polish)
            dm.sync()
        Vm, Va = dm.get_state()
        census = dm.tree_census() if solver == "block_tree" else None
    finally:
        dm.close()
    return dict(it=it, err=err, Vm=Vm, Va=Va, seed=seed, stats=st_, hist=hist, census=census)


def _first_step(hp, st, buses, Y, NE, S):
    """state after ONE Newton iteration from the fundamental power-flow seed (block-tree path)"""
    from harmonic_power_flow_amd import api, synth
    n = len(buses)
    dm = api._device_model(buses, Y, NE, True, st.HARMONICS, solver="block_tree", max_scenarios=S)
    try:
        P0, Q0 = buses["P"].to_numpy(float), buses["Q"].to_numpy(float)
        scale = np.stack([np.ones(n)] + [synth.scenario_scale(n, s) for s in range(1, S)])
        dm.set_loads(P0 * scale, Q0 * scale)
        dm.set_state(None, None, n_scen=S)
        dm.fund_pf(1e-6, 30)
        dm.mismatch(want_f=False)
        dm.iterate(1)
        dm.sync()
        return dm.get_state()
    finally:
        dm.close()


def test_static_pivot_monitor_and_repeat_with_partial_pivoting(tmp_path):
    """With the growth limit at 10^0 every pivot block counts as weak: every scenario is flagged (flags bit 3) and repeated with
    partial pivoting (bit 4) inside hpf_solve; the result must be bit-identical to an explicit block_pivoting = 1 solve.  With
    auto_repivot = 0 the flag is only reported.  At the default limit (10^10) nothing is flagged on this feeder."""
    hp = _hp()
    st, buses, Y, NE, _ = _feeder(hp, 100, 27, tmp_path)                      # b = 28 blocks
    S = 3
    ref = _solve(hp, st, buses, Y, NE, S=S, options=[("block_pivoting", 1)])
    dflt = _solve(hp, st, buses, Y, NE, S=S)
    forced = _solve(hp, st, buses, Y, NE, S=S, options=[("pivot_growth_limit_log10", 0)])
    only_flag = _solve(hp, st, buses, Y, NE, S=S, options=[("pivot_growth_limit_log10", 0), ("auto_repivot", 0)])
    assert ((dflt["stats"]["flags"] & (8 | 16)) == 0).all() and ((dflt["stats"]["flags"] & 1) == 1).all()
    assert ((forced["stats"]["flags"] & (8 | 16)) == (8 | 16)).all()
    assert ((forced["stats"]["flags"] & 1) == 1).all()
    assert np.array_equal(forced["it"], ref["it"])
    assert np.array_equal(forced["Vm"], ref["Vm"]) and np.array_equal(forced["Va"], ref["Va"])
    np.testing.assert_array_equal(forced["hist"], ref["hist"])                # NaN tail included
    assert ((only_flag["stats"]["flags"] & 8) == 8).all() and ((only_flag["stats"]["flags"] & 16) == 0).all()
    assert np.array_equal(only_flag["Vm"], dflt["Vm"])                        # reported, not repeated: the static result
    # both pivot orders end at the same voltages (iterates at the stop rule: within what the stop rule guarantees)
    U0 = dflt["Vm"] * np.exp(1j * dflt["Va"])
    U1 = ref["Vm"] * np.exp(1j * ref["Va"])
    assert np.array_equal(dflt["it"], ref["it"]) and np.abs(U0 - U1).max() < 1e-6


def test_converged_flag_and_api_details(tmp_path):
    """solve()['converged'] follows the stop rule (flags bit 0), not 'the loop ended'."""
    hp = _hp()
    from harmonic_power_flow_amd import synth
    fb, fl = synth.gen(50, seed=0, outdir=str(tmp_path))
    st = hp.Settings(H_MAX=11)
    res = hp.solve(fb, fl, coupled=True, settings=st, ne_dir=INPUTS)
    assert res["converged"] and res["details"]["stats"]["flags"][0] & 1 and not res["details"]["repeated_with_pivoting"]
    assert res["details"]["stats"]["n_iter"][0] == res["n_iter_h"]            # the record of THIS solve (not of a replay)
    assert res["details"]["stats"]["err"][0] == res["err_h"]
    st2 = hp.Settings(H_MAX=11, max_iter_h=3)
    res2 = hp.solve(fb, fl, coupled=True, settings=st2, ne_dir=INPUTS)
    assert not res2["converged"] and res2["n_iter_h"] == 3 and (res2["details"]["stats"]["flags"][0] & 2)


@pytest.mark.parametrize("name,solver", [("net2_H11_c", "dense"), ("net1_H11_c", "dense"), ("syn100_H11_c", "block_tree")])
def test_per_iteration_state_dump_follows_the_reference_trajectory(name, solver, tmp_path):
    """hpf_set_trace: the voltages after every Newton iteration, against the reference's own iterates (golden V_traj) on the
    robust K = 5 cases -- every iterate, not only the last."""
    hp = _hp()
    from harmonic_power_flow_amd import api, synth
    g = np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=True)
    st = hp.Settings(H_MAX=11)
    if name.startswith("syn"):
        fb, fl = synth.gen(100, seed=0, outdir=str(tmp_path))
    else:
        fb, fl = (os.path.join(INPUTS, name.split("_")[0] + s) for s in ("_buses.csv", "_lines.csv"))
    buses, lines, m, n, c = hp.init_network(fb, fl, settings=st)
    Y = hp.build_admittance_matrices(buses, lines, st.HARMONICS)
    NE = hp.import_Norton_Equivalents(buses, True, st, INPUTS)
    dm = api._device_model(buses, Y, NE, True, st.HARMONICS, solver=solver)
    try:
        dm.set_loads(buses["P"].to_numpy(float), buses["Q"].to_numpy(float))
        dm.set_state(None, None, n_scen=1)
        dm.fund_pf(1e-6, 30)
        it, err, hist, Vt, At = dm.solve(1e-4, 50, trace=True)
        Vm, Va = dm.get_state()
    finally:
        dm.close()
    n_it = int(it[0])
    assert n_it == int(g["n_iter_h"])
    if "V_traj" in g.files:
        traj = g["V_traj"]
        assert len(traj) == n_it + 1
        dev = []
        for k in range(n_it + 1):
            Ud = Vt[0, k] * np.exp(1j * At[0, k])
            Ug = traj[k][:, 0] * np.exp(1j * traj[k][:, 1])
            dev.append(np.abs(Ud - Ug).max() / max(1.0, np.abs(Ug).max()))
        print("\n%s: relative deviation from the reference's iterates: %s" % (name, " ".join("%.1e" % d for d in dev)))
        # the first steps are taken from (nearly) identical states; the wandering middle of the trajectory amplifies the rounding
        # differences of the two linear solvers (SuperLU there, rocSOLVER / block elimination here: SURVEY.md §0 trap #2) before
        # both contract onto the same solution
        assert max(dev[:3]) < 1e-9
        assert dev[-1] < 1e-8
        np.testing.assert_allclose(hist[0, :3], g["err_hist"][:3], rtol=1e-9)
    assert np.array_equal(Vt[0, n_it], Vm[0]) and np.array_equal(At[0, n_it], Va[0])      # last recorded iterate = final state
    assert np.isnan(Vt[0, n_it + 1:]).all()


@pytest.mark.parametrize("env", [{"HPF_LAZY": "0"}, {"HPF_LAZY": "1"}, {"HPF_SLEAF": "0"}, {"HPF_SLEAF": "1"},
                                 {"HPF_SLLAZY": "0"}, {"HPF_SLBACK": "0"}, {"HPF_LEAFBATCH": "0"}, {"HPF_GROUPS": "2"},
                                 {"HPF_SLNEST": "0"}, {"HPF_LINTREE": "0"}, {"HPF_FUSELEVEL": "0"}, {"HPF_LINBUNDLE": "0"}, {"HPF_CHAINBUNDLE": "0"},
                                 {"HPF_COMPRESS": "0"}, {"HPF_FUSEBACK": "0"}])
def test_tree_build_variants_take_the_same_newton_steps(env, tmp_path, monkeypatch):
    """Every diagnostic switch of hpf_create (hpf.h) selects a more general path for some class of buses (no lazy leaves, no
    super-leaves, super-leaves that push their Schur complement / store their inverse, leaves one workgroup per scenario): the
    first Newton steps and the converged voltages must agree with the default build at rounding level."""
    hp = _hp()
    st, buses, Y, NE, _ = _feeder(hp, 300, 51, tmp_path, seed=2)
    S = 17
    base = _solve(hp, st, buses, Y, NE, S=S, polish=1)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    var = _solve(hp, st, buses, Y, NE, S=S, polish=1)
    if "HPF_GROUPS" in env or "HPF_LINTREE" in env or "HPF_LINBUNDLE" in env or "HPF_CHAINBUNDLE" in env or "HPF_FUSEBACK" in env:   # same arithmetic, other launch shapes: bit-identical
        assert np.array_equal(var["Vm"], base["Vm"]) and np.array_equal(var["Va"], base["Va"])
    Ub, Uv = base["Vm"] * np.exp(1j * base["Va"]), var["Vm"] * np.exp(1j * var["Va"])
    print("\n%s: iterations %s vs %s, max|dU| after one more iteration %.2e" % (env, var["it"][:4], base["it"][:4], np.abs(Ub - Uv).max()))
    assert (var["err"] <= 1e-4).all()
    assert np.abs(Ub - Uv).max() < TOL_V


@pytest.mark.parametrize("n,hmax", [(1000, 51), (600, 11), (400, 27)])
def test_nested_bordered_buses_match_the_gauss_jordan_path(n, hmax, tmp_path, monkeypatch):
    """Bordered buses below bordered buses (the child's m_c x m_c core T_c sits on the parent's diagonal, total
    border <= 10) replace Gauss-Jordan buses of the upper tree; with HPF_SLNEST=0 the same buses take the general kernel.  Same
    converged voltages (fixed point: one Newton iteration past the stop rule on both sides; the iteration COUNTS of the load
    scenarios of this feeder differ with any change of the rounding, SURVEY.md §0 trap #2) and the census says which path ran."""
    hp = _hp()
    st, buses, Y, NE, _ = _feeder(hp, n, hmax, tmp_path, seed=0)
    S = 19                                                          # one full 16-scenario workgroup and a ragged one
    nest = _solve(hp, st, buses, Y, NE, S=S, polish=1)
    monkeypatch.setenv("HPF_SLNEST", "0")
    flat = _solve(hp, st, buses, Y, NE, S=S, polish=1)
    print("\nn=%d hmax=%d: nested %s\n               flat   %s" % (n, hmax, nest["census"], flat["census"]))
    assert flat["census"]["nested_bordered"] == 0
    assert nest["census"]["gauss_jordan"] + nest["census"]["nested_bordered"] == flat["census"]["gauss_jordan"]
    if (n, hmax) == (1000, 51):                                     # the headline feeder: a quarter of its Gauss-Jordan buses
        assert nest["census"]["nested_bordered"] >= 20
        assert nest["census"]["gauss_jordan"] <= flat["census"]["gauss_jordan"] - 20
    assert (nest["err"] <= 1e-4).all() and (flat["err"] <= 1e-4).all()
    Un, Uf = nest["Vm"] * np.exp(1j * nest["Va"]), flat["Vm"] * np.exp(1j * flat["Va"])
    assert np.abs(Un - Uf).max() < TOL_V


@pytest.mark.parametrize("n,hmax", [(1000, 51), (600, 11), (400, 27)])
def test_compress_steps_shorten_the_level_chain_and_keep_the_newton_step(n, hmax, tmp_path, monkeypatch):
    """Compress steps: Gauss-Jordan buses of the skeleton are eliminated BEFORE their tallest dense child (four pushes,
    dense fill blocks, a dense push and a dense back-substitution term for that child).  Fewer elimination levels than the strictly
    leaf-first order (HPF_COMPRESS=0), the same Newton step at rounding level, the same fixed point."""
    hp = _hp()
    st, buses, Y, NE, _ = _feeder(hp, n, hmax, tmp_path, seed=0)
    S = 5
    comp = _solve(hp, st, buses, Y, NE, S=S, polish=1)
    one_c = _first_step(hp, st, buses, Y, NE, S)
    monkeypatch.setenv("HPF_COMPRESS", "0")
    flat = _solve(hp, st, buses, Y, NE, S=S, polish=1)
    one_f = _first_step(hp, st, buses, Y, NE, S)
    print("\nn=%d hmax=%d: compress %s\n               leaf-first %s" % (n, hmax, comp["census"], flat["census"]))
    assert flat["census"]["compress_steps"] == 0
    assert comp["census"]["compress_steps"] > 0
    assert comp["census"]["levels"] < flat["census"]["levels"]
    assert comp["census"]["gauss_jordan"] == flat["census"]["gauss_jordan"]
    d1 = np.abs(one_c[0] - one_f[0]).max(), np.abs(one_c[1] - one_f[1]).max()
    print("first Newton step: max|dVm| %.2e  max|dVa| %.2e" % d1)
    assert d1[0] < 1e-9 and d1[1] < 1e-8                      # (the first steps of these feeders are tens of radians long)
    assert (comp["err"] <= 1e-4).all() and (flat["err"] <= 1e-4).all()
    Uc, Uf = comp["Vm"] * np.exp(1j * comp["Va"]), flat["Vm"] * np.exp(1j * flat["Va"])
    print("fixed points: max|dU| %.2e" % np.abs(Uc - Uf).max())
    assert np.abs(Uc - Uf).max() < TOL_V


def test_compress_steps_are_the_default_at_every_capacity_and_results_do_not_depend_on_it(tmp_path, monkeypatch):
    """VERDICT r4 parity limit (ii): the iteration count of a solver-sensitive case depended on the capacity a handle was created with (compress
    steps up to 256 scenarios only).  Round 5: the steps are the default at every capacity -- the same scenario solved in handles of capacity 1, 8
    and 300 gives bit-identical voltages and counts --; HPF_COMPRESS=0 (option string) builds the leaf-first tree (5 - 8 % faster per step from
    ~384 live scenarios on)."""
    hp = _hp()
    from harmonic_power_flow_amd import ingest, synth
    from harmonic_power_flow_amd.device import DeviceModel
    st, buses, Y, NE, _ = _feeder(hp, 1000, 51, tmp_path, seed=0)
    monkeypatch.delenv("HPF_COMPRESS", raising=False)
    m, n, c = ingest.network_constants(buses)
    dev, Y_N, I_N, n_dev = ingest.norton_arrays(buses, NE, True, len(st.HARMONICS))
    P0, Q0 = buses["P"].to_numpy(float), buses["Q"].to_numpy(float)
    scale = np.stack([synth.scenario_scale(n, s) for s in (0, 5)])
    got, res = {}, {}
    for S, opt in ((1, None), (8, None), (300, None), (300, "HPF_COMPRESS=0")):
        dm = DeviceModel(n, m, c, st.HARMONICS, Y.rowptr, Y.col, Y.Yval, dev, Y_N, I_N, n_dev, True, solver="block_tree", max_scenarios=S, options=opt)
        try:
            got[(S, opt)] = dm.tree_census()
            k = min(S, 2)
            dm.set_loads((P0 * scale)[:k], (Q0 * scale)[:k])
            dm.set_state(None, None, n_scen=k)
            dm.fund_pf(1e-6, 30)
            it, err, _ = dm.solve(1e-4, 50)
            Vm, Va = dm.get_state()
            res[(S, opt)] = (it.copy(), err.copy(), Vm.copy(), Va.copy())
        finally:
            dm.close()
    assert got[(1, None)] == got[(8, None)] == got[(300, None)] and got[(300, None)]["compress_steps"] > 0
    assert got[(300, "HPF_COMPRESS=0")]["compress_steps"] == 0 and got[(300, None)]["levels"] < got[(300, "HPF_COMPRESS=0")]["levels"]   # 10 vs 15 here
    a, b, d = res[(1, None)], res[(8, None)], res[(300, None)]
    assert b[0][0] == a[0][0] == d[0][0] and np.array_equal(a[2][0], b[2][0]) and np.array_equal(a[3][0], d[3][0]) and np.array_equal(a[2][0], d[2][0])
    assert np.array_equal(b[0], d[0]) and np.array_equal(b[2], d[2]) and np.array_equal(b[3], d[3]) and np.array_equal(b[1], d[1])


# (n, H_MAX, share of nonlinear buses, PV buses, generator seed, iterations of the ORACLE [50 = the reference's own Newton iteration
#  does not converge on this feeder: measured with oracle/hpf_oracle.py, err stays at 1e2..1e4])
FUZZ = [(347, 35, 0.85, 0, 880227, 50), (377, 51, 0.60, 2, 318146, 31), (118, 27, 0.85, 2, 867892, 50), (384, 59, 0.15, 0, 569402, 26),
        (200, 35, 0.60, 2, 422784, 23), (262, 25, 0.85, 0, 438186, 22), (54, 27, 0.15, 0, 657433, 14), (403, 11, 0.35, 2, 522250, 22),
        (296, 25, 0.85, 1, 644436, 28), (161, 19, 0.35, 1, 692459, 50),
        (125, 75, 0.60, 2, 128047, 50)]       # (round 3: the one outlier of 300 fuzz cases, first step 6.5e-6 off -- the reference's iteration diverges here too)


@pytest.mark.parametrize("n,hmax,frac,n_pv,seed,it_oracle", FUZZ)
def test_fuzz_feeders_converged_voltages_block_tree_vs_dense(n, hmax, frac, n_pv, seed, it_oracle, tmp_path):
    """The cases of the round-1 fuzz sweep (tools/fuzz_parity.py) with the north-star criterion: where the reference's algorithm
    converges (oracle), the CONVERGED voltages (fixed point: two Newton iterations past the stop rule on both sides) of the
    block-tree path and of the dense rocSOLVER path agree within 1e-8 p.u.  Seed 880227 -- the worst first-step deviation of that
    sweep, 5e-8 rad -- is a feeder on which the reference's own iteration DIVERGES (85 % nonlinear buses; first steps of tens of
    radians, err 1e2..1e3 after 50 iterations): there, and on the two other such feeders, the product must report the same
    non-convergence (n_iter = max_iter, flags bit 1, not bit 0) on both solver paths instead of a result."""
    hp = _hp()
    st, buses, Y, NE, _ = _feeder(hp, n, hmax, tmp_path, seed=seed, frac_nl=frac, n_pv=n_pv)
    Hn = len(st.HARMONICS)
    bt = _solve(hp, st, buses, Y, NE, S=1, polish=2)
    de = _solve(hp, st, buses, Y, NE, solver="dense", S=1, seed_state=bt["seed"], polish=2)
    print("\nn=%d Hn=%d nl=%.2f pv=%d seed=%d: oracle %d it, block-tree %s it (flags %s), dense %s it (flags %s)"
          % (n, Hn, frac, n_pv, seed, it_oracle, bt["it"], bt["stats"]["flags"], de["it"], de["stats"]["flags"]))
    if it_oracle >= 50:
        for r in (bt, de):
            assert r["it"][0] == 50 and (r["stats"]["flags"][0] & 3) == 2 and not r["err"][0] <= 1e-4
        return
    assert (bt["err"] <= 1e-4).all() and ((bt["stats"]["flags"] & 1) == 1).all()
    assert ((bt["stats"]["flags"] & (8 | 16 | 32)) == 0).all()
    assert (de["err"] <= 1e-4).all()
    Ub, Ud = bt["Vm"] * np.exp(1j * bt["Va"]), de["Vm"] * np.exp(1j * de["Va"])
    print("   fixed points differ by %.2e" % np.abs(Ub - Ud).max())
    assert np.abs(Ub - Ud).max() < TOL_V


@pytest.mark.parametrize("n,hmax", [(400, 27), (600, 11), (300, 51)])
def test_level_kernel_for_every_block_size_matches_separate_launches(n, hmax, tmp_path, monkeypatch):
    """k_level (one launch per elimination level) runs b <= 12, <= 28 and <= 52 blocks alike: the factor body of a smaller block uses
    the first 64 NT threads of the 256-thread workgroup.  Same Newton steps as the separate launches (HPF_FUSELEVEL=0)."""
    hp = _hp()
    st, buses, Y, NE, _ = _feeder(hp, n, hmax, tmp_path, seed=1)
    S = 21
    fused = _solve(hp, st, buses, Y, NE, S=S, polish=1)
    monkeypatch.setenv("HPF_FUSELEVEL", "0")
    plain = _solve(hp, st, buses, Y, NE, S=S, polish=1)
    # census[9] = EVERY elimination level is one k_level launch: always so for blocks of 52; smaller blocks fuse the levels that have
    # scenario-batched workgroups only (the upper levels run k_factor_q's own grid), so the flag is 0 there although k_level runs
    assert plain["census"]["fused_levels"] == 0
    if 2 * ((hmax + 1) // 2) > 28:
        assert fused["census"]["fused_levels"] == 1
    assert (fused["err"] <= 1e-4).all() and (plain["err"] <= 1e-4).all()
    Uf, Up = fused["Vm"] * np.exp(1j * fused["Va"]), plain["Vm"] * np.exp(1j * plain["Va"])
    print("\nn=%d hmax=%d: iterations %s vs %s, max|dU| %.2e" % (n, hmax, fused["it"][:4], plain["it"][:4], np.abs(Uf - Up).max()))
    assert np.abs(Uf - Up).max() < TOL_V


@pytest.mark.parametrize("n,hmax,frac,seed,S", [(150, 51, 0.6, 11, 20), (220, 27, 0.35, 5, 33), (120, 51, 0.85, 3, 17)])
def test_many_scenarios_block_tree_vs_dense_fixed_points(n, hmax, frac, seed, S, tmp_path):
    """The scenario-batched kernels (16 scenarios per workgroup: lazy leaves, bordered and nested bordered buses; full and ragged tiles,
    1..3 stream groups), the level kernel and the bundle kernels against an INDEPENDENT solver on the same scenarios: dense rocSOLVER LU
    of the full Jacobian, batched over the scenarios.  Converged voltages (two Newton iterations past the stop rule on both sides)
    within 1e-8 p.u. for every scenario both paths converge on; the census shows the block-tree classes are all populated."""
    hp = _hp()
    st, buses, Y, NE, _ = _feeder(hp, n, hmax, tmp_path, seed=seed, frac_nl=frac)
    bt = _solve(hp, st, buses, Y, NE, S=S, polish=2)
    de = _solve(hp, st, buses, Y, NE, solver="dense", S=S, seed_state=bt["seed"], polish=2)
    ok = (bt["err"] <= 1e-4) & (de["err"] <= 1e-4)
    print("\nn=%d hmax=%d S=%d: census %s; converged on both paths %d / %d; iterations bt %s dense %s"
          % (n, hmax, S, bt["census"], ok.sum(), S, bt["it"][:5], de["it"][:5]))
    assert bt["census"]["lazy_leaves"] > 0 and bt["census"]["bordered"] > 0
    assert ok.sum() >= S - 2                                            # (a scenario one path leaves at max_iter is not compared)
    assert np.array_equal((bt["stats"]["flags"] & 1) == 1, bt["err"] <= 1e-4)
    Ub, Ud = bt["Vm"] * np.exp(1j * bt["Va"]), de["Vm"] * np.exp(1j * de["Va"])
    dev = np.abs(Ub - Ud).max(axis=1)
    print("   fixed points differ by at most %.2e (scenario %d)" % (dev[ok].max(), int(np.argmax(np.where(ok, dev, 0.0)))))
    assert dev[ok].max() < TOL_V


# ---- meshed networks on the block-tree path (bordered Newton step) ------------------------------------------------------------
def _add_ties(fl, n, k, seed=42):
    import importlib.util
    spec = importlib.util.spec_from_file_location("mgb", os.path.join(os.path.dirname(GOLD), "..", "oracle", "make_golden_bench.py"))
    mgb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mgb)
    return mgb.add_ties(fl, n, k, seed)


@pytest.mark.parametrize("n,hmax,k", [(300, 51, 3), (120, 11, 1), (200, 27, 4), (260, 51, 12), (100, 99, 2)])
def test_meshed_feeder_bordered_block_tree_vs_dense(n, hmax, k, tmp_path):
    """A radial feeder plus k loop-closing lines: BFS spanning tree + bordered system on the block-tree path, in BOTH forms -- factor-once (round 5,
    default: one sweep + selected inversion over the endpoints' root paths) and the m virtual sweeps of rounds 2 - 4 (HPF_MESH_SEL=0: m + 2
    right-hand sides per Newton step in chunks of virtual scenarios) --, m x m border system on rocSOLVER, fundamental pf through the dense LU,
    against the dense rocSOLVER path on the full meshed Jacobian: pf seed, first Newton step, converged voltages (fixed point) within 1e-8.
    (260, 51, 12): m = 1 196 border unknowns; (100, 99, 2): blocks of 100 (the kernels of BASELINE config 5)."""
    hp = _hp()
    from harmonic_power_flow_amd import api, synth
    fb, fl = synth.gen(n, seed=4, outdir=str(tmp_path))
    ties = _add_ties(fl, n, k)
    st = hp.Settings(H_MAX=hmax)
    buses, lines, m, nn, c = hp.init_network(fb, fl, settings=st)
    Y = hp.build_admittance_matrices(buses, lines, st.HARMONICS)
    assert len(Y.col) == n + 2 * (n - 1) + 2 * k
    NE = hp.import_Norton_Equivalents(buses, True, st, INPUTS)
    out = {}
    for solver in ("dense", "block_tree", "virtual"):
        dm = api._device_model(buses, Y, NE, True, st.HARMONICS, solver="dense" if solver == "dense" else "block_tree",
                               options="HPF_MESH_SEL=0" if solver == "virtual" else None)
        try:
            dm.set_loads(buses["P"].to_numpy(float), buses["Q"].to_numpy(float))
            dm.set_state(None, None, n_scen=1)
            nf, _, _ = dm.fund_pf(1e-6, 30)
            v0 = dm.get_state()
            if solver != "dense":
                cs = dm.tree_census()                       # factor-once with the block Gauss-Jordan border solve | virtual sweeps
                assert cs["ties"] == k and cs["bordered_form"] == (2 if solver == "block_tree" else 0) and cs["border_unknowns"] % (2 * len(st.HARMONICS)) == 0
                assert (cs["root_path_buses"] > 0) == (solver == "block_tree")
            if "dense" in out:
                np.testing.assert_allclose(v0[0], out["dense"][0][0], rtol=0, atol=1e-12)
                np.testing.assert_allclose(v0[1], out["dense"][0][1], rtol=0, atol=1e-12)
                dm.set_state(*out["dense"][0])
            dm.mismatch(want_f=False)
            dm.iterate(1)
            dm.sync()
            v1 = dm.get_state()
            dm.set_state(*(out["dense"][0] if "dense" in out else v0))
            n_iter, err, _ = dm.solve(1e-4, 50)
            stt = dm.stats()
            dm.mismatch(want_f=False)
            dm.iterate(2)
            dm.sync()
            out[solver] = (v0, v1, dm.get_state(), int(n_iter[0]), float(err[0]), stt)
        finally:
            dm.close()
    v0d, v1d, vfd, itd, ed, _ = out["dense"]
    step = max(np.abs(v1d[0] - v0d[0]).max(), np.abs(v1d[1] - v0d[1]).max())
    Ud = vfd[0][0] * np.exp(1j * vfd[1][0])
    for form in ("block_tree", "virtual"):
        v0b, v1b, vfb, itb, eb, stb = out[form]
        d1 = max(np.abs(v1d[0] - v1b[0]).max(), np.abs(v1d[1] - v1b[1]).max())
        Ub = vfb[0][0] * np.exp(1j * vfb[1][0])
        print("\nn=%d H_MAX=%d ties %s, %s: first step %.1e (deviation %.1e); dense %d it (err %.1e), bordered block-tree %d it (err %.1e); fixed points differ by %.2e"
              % (n, hmax, ties, "factor-once" if form == "block_tree" else "virtual sweeps", step, d1, itd, ed, itb, eb, np.abs(Ud - Ub).max()))
        assert d1 <= 1e-8 * max(1.0, step)
        assert ed <= 1e-4 and eb <= 1e-4 and (stb["flags"][0] & 1)
        assert np.abs(Ud - Ub).max() < TOL_V


def test_border_system_unpivoted_lu_with_residual_check_vs_pivoted(tmp_path):
    """The m x m border system of a bordered Newton step: unpivoted LU + residual check (default; a failed check repeats it pivoted) against
    option "border_pivoting" = 1 (always rocSOLVER's pivoted LU): same Newton steps to 1e-9 of the step, same fixed point; the census counts the
    systems that went through the pivoted LU."""
    hp = _hp()
    from harmonic_power_flow_amd import api, synth
    n, hmax, k = 260, 51, 6
    fb, fl = synth.gen(n, seed=4, outdir=str(tmp_path))
    _add_ties(fl, n, k)
    st = hp.Settings(H_MAX=hmax)
    buses, lines, m, nn, c = hp.init_network(fb, fl, settings=st)
    Y = hp.build_admittance_matrices(buses, lines, st.HARMONICS)
    NE = hp.import_Norton_Equivalents(buses, True, st, INPUTS)
    out = {}
    for piv in (0, 1):
        dm = api._device_model(buses, Y, NE, True, st.HARMONICS, solver="block_tree")
        try:
            dm.set_option("border_pivoting", piv)
            dm.set_loads(buses["P"].to_numpy(float), buses["Q"].to_numpy(float))
            dm.set_state(None, None, n_scen=1)
            dm.fund_pf(1e-6, 30)
            v0 = dm.get_state()
            dm.mismatch(want_f=False)
            dm.iterate(1)
            dm.sync()
            v1 = dm.get_state()
            dm.set_state(*v0)
            n_iter, err, _ = dm.solve(1e-4, 50)
            dm.mismatch(want_f=False)
            dm.iterate(2)
            dm.sync()
            out[piv] = (v0, v1, dm.get_state(), int(n_iter[0]), float(err[0]), dm.tree_census())
        finally:
            dm.close()
    (v0a, v1a, vfa, ita, ea, ca), (v0b, v1b, vfb, itb, eb, cb) = out[0], out[1]
    step = max(np.abs(v1b[0] - v0b[0]).max(), np.abs(v1b[1] - v0b[1]).max())
    d1 = max(np.abs(v1a[0] - v1b[0]).max(), np.abs(v1a[1] - v1b[1]).max())
    Ua, Ub = vfa[0][0] * np.exp(1j * vfa[1][0]), vfb[0][0] * np.exp(1j * vfb[1][0])
    print("\nborder LU: unpivoted + check %d it (repeated pivoted: %d), always pivoted %d it (%d systems); first step %.1e, deviation %.1e; "
          "fixed points differ by %.2e" % (ita, ca["border_repivots"], itb, cb["border_repivots"], step, d1, np.abs(Ua - Ub).max()))
    assert ca["ties"] == k and cb["border_repivots"] >= itb + 3 and ca["border_repivots"] <= cb["border_repivots"]
    assert d1 <= 1e-9 * max(1.0, step)
    assert ea <= 1e-4 and eb <= 1e-4
    assert np.abs(Ua - Ub).max() < TOL_V


def test_meshed_handle_refuses_the_pivoted_mode(tmp_path):
    """The bordered Newton step of a meshed network exists in the bus-image layout of the static-pivot kernels only: asking such a handle
    for partial pivoting (option block_pivoting = 1) is refused with HPF_E_STATE instead of taking silently wrong steps, and env
    HPF_GJ_MODE=0 does not apply to it."""
    hp = _hp()
    from harmonic_power_flow_amd import _lib, api, synth
    fb, fl = synth.gen(120, seed=4, outdir=str(tmp_path))
    _add_ties(fl, 120, 2)
    st = hp.Settings(H_MAX=11)
    buses, lines, m, nn, c = hp.init_network(fb, fl, settings=st)
    Y = hp.build_admittance_matrices(buses, lines, st.HARMONICS)
    NE = hp.import_Norton_Equivalents(buses, True, st, INPUTS)
    dm = api._device_model(buses, Y, NE, True, st.HARMONICS, solver="block_tree")
    try:
        assert dm.tree_census()["ties"] == 2
        with pytest.raises(_lib.HpfError) as ei:
            dm.set_option("block_pivoting", 1)
        assert ei.value.code == -2
        dm.set_option("block_pivoting", 0)
    finally:
        dm.close()


def test_dense_solver_beyond_32_bit_offsets_matches_the_block_tree_step(tmp_path):
    """N = 51 998 (the headline feeder as ONE dense system, 21.6 GB): beyond rocSOLVER's 32-bit element offsets, refused until round 2;
    now through the 64-bit entry points.  The first Newton step from the same pf seed against the block-tree path (the second one
    already amplifies the rounding difference of two solvers a thousandfold on this feeder: SURVEY.md trap #2)."""
    hp = _hp()
    from harmonic_power_flow_amd import api
    st, buses, Y, NE, _ = _feeder(hp, 1000, 51, tmp_path, seed=0)
    out = {}
    for solver in ("block_tree", "dense"):
        dm = api._device_model(buses, Y, NE, True, st.HARMONICS, solver=solver)
        try:
            assert dm.N == 51998
            dm.set_loads(buses["P"].to_numpy(float), buses["Q"].to_numpy(float))
            dm.set_state(None, None, n_scen=1)
            dm.fund_pf(1e-6, 30)
            if out:
                dm.set_state(*out["block_tree"][0])
            v0 = dm.get_state()
            dm.mismatch(want_f=False)
            dm.iterate(1)
            dm.sync()
            out[solver] = (v0, dm.get_state())
        finally:
            dm.close()
    (v0, vb), (_, vd) = out["block_tree"], out["dense"]
    step = max(np.abs(vb[0] - v0[0]).max(), np.abs(vb[1] - v0[1]).max())
    d = max(np.abs(vb[0] - vd[0]).max(), np.abs(vb[1] - vd[1]).max())
    print("\ndense (64-bit rocSOLVER) vs block tree after one Newton iteration: %.2e (step of %.1e)" % (d, step))
    assert d <= 1e-8 * max(1.0, step)


@pytest.mark.parametrize("k", [5, 20])
def test_meshed_headline_feeder_vs_oracle_fixture(k, tmp_path):
    """gen(1000, seed 0) + k loop-closing lines, harmonics 1..51: N = 51 998 was beyond the dense limit of rounds 1-2 (N*N < 2^31), so
    before the bordered step such a feeder could not be solved on the GPU at all (missing #1); k = 20 (40 endpoint buses,
    m = 2 080 border unknowns, nine chunks of virtual scenarios) was beyond the bordered step's own bound of 1 024 until round 3 (VERDICT
    r02, missing #2).  solver="auto" must take the block-tree path; result against the oracle (SuperLU on the meshed Jacobian;
    tests/golden/syn1000_H51_mesh<k>.npz)."""
    path = os.path.join(GOLD, "syn1000_H51_mesh%d.npz" % k)
    if not os.path.exists(path):
        pytest.skip("fixture not generated (oracle/make_golden_bench.py mesh %d)" % k)
    hp = _hp()
    from harmonic_power_flow_amd import api, synth
    g = np.load(path)
    fb, fl = synth.gen(1000, seed=0, outdir=str(tmp_path))
    ties = _add_ties(fl, 1000, k)
    assert np.array_equal(np.array(ties), g["ties"])
    st = hp.Settings(H_MAX=51)
    buses, lines, m, n, c = hp.init_network(fb, fl, settings=st)
    Y = hp.build_admittance_matrices(buses, lines, st.HARMONICS)
    NE = hp.import_Norton_Equivalents(buses, True, st, INPUTS)
    dm = api._device_model(buses, Y, NE, True, st.HARMONICS, solver="auto")
    try:
        assert dm.solver == "block_tree"
        dm.set_loads(buses["P"].to_numpy(float), buses["Q"].to_numpy(float))
        dm.set_state(None, None, n_scen=1)
        dm.fund_pf(1e-6, 30)
        seed = dm.get_state()
        np.testing.assert_allclose(np.stack([seed[0][0][:1000], seed[1][0][:1000]], 1), g["seed_fund"], rtol=0, atol=1e-11)
        n_iter, err, _ = dm.solve(1e-4, 50)
        Vm, Va = dm.get_state()
        dm.mismatch(want_f=False)
        dm.iterate(2)
        dm.sync()
        Vm2, Va2 = dm.get_state()
    finally:
        dm.close()
    idx = g["idx"]
    U, U2 = Vm[0] * np.exp(1j * Va[0]), Vm2[0] * np.exp(1j * Va2[0])
    Us = g["V_stop_sample"][:, 0] * np.exp(1j * g["V_stop_sample"][:, 1])
    Uf = g["V_fix_sample"][:, 0] * np.exp(1j * g["V_fix_sample"][:, 1])
    d_stop, d_fix = np.abs(U[idx] - Us).max(), np.abs(U2[idx] - Uf).max()
    d_sum = np.abs(np.abs(U2).reshape(26, 1000).sum(1) - g["U_fix_abs_per_harmonic"]).max()
    print("\nmeshed syn1000 + %d ties: %d it (oracle %d) err %.2e; |dU| at the stop rule %.2e, at the fixed point %.2e; per-harmonic sum |U| deviation %.2e"
          % (k, n_iter[0], int(g["n_iter"]), err[0], d_stop, d_fix, d_sum))
    assert err[0] <= 1e-4 and n_iter[0] < 50
    assert d_stop < 1e-6 and d_fix < TOL_V and d_sum < 1000 * TOL_V * 1e-2


def test_meshed_feeder_several_scenarios_and_sweep_api(tmp_path):
    """The bordered step with S > 1 real scenarios in one handle (the virtual slots sit behind them; scenarios that converge
    drop out of the host's walk): every scenario lands on the dense path's fixed point and on its own single-scenario solve
    (not bit for bit: the fundamental pf of a meshed handle goes through rocSOLVER, whose batched and single LU round differently)."""
    hp = _hp()
    from harmonic_power_flow_amd import api, synth
    n, hmax, k, S = 150, 15, 2, 4
    fb, fl = synth.gen(n, seed=9, outdir=str(tmp_path))
    _add_ties(fl, n, k)
    st = hp.Settings(H_MAX=hmax)
    buses, lines, m, nn, c = hp.init_network(fb, fl, settings=st)
    Y = hp.build_admittance_matrices(buses, lines, st.HARMONICS)
    NE = hp.import_Norton_Equivalents(buses, True, st, INPUTS)
    P0, Q0 = buses["P"].to_numpy(float), buses["Q"].to_numpy(float)
    scale = np.stack([synth.scenario_scale(n, s) for s in range(S)])

    def run(solver, ids):
        dm = api._device_model(buses, Y, NE, True, st.HARMONICS, solver=solver, max_scenarios=len(ids))
        try:
            dm.set_loads(P0 * scale[ids], Q0 * scale[ids])
            dm.set_state(None, None, n_scen=len(ids))
            dm.fund_pf(1e-6, 30)
            it, err, _ = dm.solve(1e-4, 50)
            stop = dm.get_state()
            dm.mismatch(want_f=False)
            dm.iterate(2)
            dm.sync()
            return it, err, stop, dm.get_state()
        finally:
            dm.close()
    itb, errb, stopb, fixb = run("block_tree", list(range(S)))
    itd, errd, stopd, fixd = run("dense", list(range(S)))
    assert (errb <= 1e-4).all() and (errd <= 1e-4).all()
    Ub, Ud = fixb[0] * np.exp(1j * fixb[1]), fixd[0] * np.exp(1j * fixd[1])
    print("\nmeshed, %d scenarios: bordered %s it, dense %s it, fixed points differ by %.2e" % (S, itb, itd, np.abs(Ub - Ud).max()))
    assert np.abs(Ub - Ud).max() < TOL_V
    for s in (0, S - 1):
        it1, err1, stop1, fix1 = run("block_tree", [s])
        U1 = fix1[0][0] * np.exp(1j * fix1[1][0])
        assert it1[0] == itb[s] and np.abs(U1 - Ub[s]).max() < 1e-10


def test_auto_takes_the_bordered_block_tree_path_for_meshed_feeders_of_32_buses_and_more(tmp_path):
    """solver="auto" (round 5): a meshed feeder of 100 buses (N = 2 798, far below the N > 8 192 of rounds 2 - 4) runs the bordered block-tree step and lands
    on the dense path's voltages; a 20-bus ring stays on the dense LU."""
    hp = _hp()
    from harmonic_power_flow_amd import synth
    fb, fl = synth.gen(100, seed=3, outdir=str(tmp_path))
    synth.add_ties(fl, 100, 3)
    st = hp.Settings(H_MAX=27)
    buses, lines, m, n, c = hp.init_network(fb, fl, settings=st)
    da, dd = {}, {}
    Va_, ea, ia, _ = hp.hpf(buses, lines, True, settings=st, ne_dir=INPUTS, verbose=False, details=da, extra_iters=2)
    Vd_, ed, idn, _ = hp.hpf(buses, lines, True, settings=st, ne_dir=INPUTS, verbose=False, details=dd, solver="dense", extra_iters=2)
    assert da["solver"] == "block_tree" and da["tree"]["ties"] == 3 and da["tree"]["bordered_form"] == 2 and dd["solver"] == "dense"
    Ua = Va_["V_m"].to_numpy() * np.exp(1j * Va_["V_a"].to_numpy())
    Ud = Vd_["V_m"].to_numpy() * np.exp(1j * Vd_["V_a"].to_numpy())
    print("\nauto on a meshed feeder of 100 buses: %s, %d it (dense %d), fixed points differ by %.2e" % (da["solver"], ia, idn, np.abs(Ua - Ud).max()))
    assert ea <= 1e-4 and ed <= 1e-4 and np.abs(Ua - Ud).max() < TOL_V
    fb2, fl2 = synth.gen(20, seed=3, outdir=str(tmp_path), prefix="small")
    synth.add_ties(fl2, 20, 1)
    buses2, lines2, _, _, _ = hp.init_network(fb2, fl2, settings=st)
    d2 = {}
    hp.hpf(buses2, lines2, True, settings=st, ne_dir=INPUTS, verbose=False, details=d2)
    assert d2["solver"] == "dense"


def test_meshed_batches_of_scenarios_equal_one_scenario_at_a_time(tmp_path):
    """Factor-once bordered step (round 5): the selected inversion and the border solve of a group's running scenarios go through the block-product
    kernels as ONE batch (second grid dimension); with HPF_MESH_BATCH_GB too small for more than one scenario's buffers the same scenarios go one
    after the other, and with HPF_BORDER_GJ=0 the border systems take rocSOLVER's unpivoted LU one by one.  Same seed -> the batched and the serial
    run must agree bit for bit (the same arithmetic per scenario, whatever the batch), scenarios converging at different iterations included;
    the rocSOLVER form agrees at the fixed point."""
    hp = _hp()
    from harmonic_power_flow_amd import api, synth
    n, hmax, k, S = 220, 27, 3, 7
    fb, fl = synth.gen(n, seed=5, outdir=str(tmp_path))
    _add_ties(fl, n, k)
    st = hp.Settings(H_MAX=hmax)
    buses, lines, m, nn, c = hp.init_network(fb, fl, settings=st)
    Y = hp.build_admittance_matrices(buses, lines, st.HARMONICS)
    NE = hp.import_Norton_Equivalents(buses, True, st, INPUTS)
    P0, Q0 = buses["P"].to_numpy(float), buses["Q"].to_numpy(float)
    scale = np.stack([synth.scenario_scale(n, s) for s in range(S)])
    scale[3] *= 0.2                                           # (a light scenario: converges earlier than the others)
    seed = None
    out = {}
    for name, opt in (("batched", None), ("serial", "HPF_MESH_BATCH_GB=0.000001"), ("rocsolver", "HPF_BORDER_GJ=0")):
        dm = api._device_model(buses, Y, NE, True, st.HARMONICS, solver="block_tree", max_scenarios=S, options=opt)
        try:
            dm.set_loads(P0 * scale, Q0 * scale)
            dm.set_state(None, None, n_scen=S)
            dm.fund_pf(1e-6, 30)
            if seed is None:
                seed = dm.get_state()
            dm.set_state(*seed)                               # (the same fundamental seed for every run)
            it, err, hist = dm.solve(1e-4, 50)
            stop = dm.get_state()
            dm.mismatch(want_f=False)
            dm.iterate(2)
            dm.sync()
            out[name] = (it.copy(), err.copy(), stop, dm.get_state(), dm.tree_census())
        finally:
            dm.close()
    itb, errb, stopb, fixb, csb = out["batched"]
    its, errs, stops, fixs, css = out["serial"]
    itr, errr, stopr, fixr, csr = out["rocsolver"]
    print("\nmeshed batch of %d: iterations %s (serial %s, rocSOLVER border %s), forms %d / %d / %d" % (S, itb, its, itr, csb["bordered_form"], css["bordered_form"],
                                                                                                    csr["bordered_form"]))
    assert csb["bordered_form"] == 2 and css["bordered_form"] == 2 and csr["bordered_form"] == 1
    assert (errb <= 1e-4).all() and len(set(itb.tolist())) > 1
    assert np.array_equal(itb, its) and np.array_equal(stopb[0], stops[0]) and np.array_equal(stopb[1], stops[1])
    assert np.array_equal(fixb[0], fixs[0]) and np.array_equal(fixb[1], fixs[1])
    Ub, Ur = fixb[0] * np.exp(1j * fixb[1]), fixr[0] * np.exp(1j * fixr[1])
    assert (errr <= 1e-4).all() and np.abs(Ub - Ur).max() < TOL_V


def test_virtual_sweep_groups_leave_the_callers_slice_alone(tmp_path):
    """The virtual-sweep bordered step (HPF_MESH_SEL=0) is the one place where a nested sweep launches on slices of its own -- one launch context per
    virtual group -- inside its caller's slice of real scenarios.  64 buses, harmonics 1 .. 11 (blocks of 12 rows), 6 loop-closing lines with 12
    distinct endpoint buses: 1 + m = 145 virtual scenarios, so with HPF_GROUPS=4 every sweep of the border columns runs as four groups on four streams,
    with HPF_GROUPS=1 as one.  Two real scenarios with different loads, three iterations: the second scenario runs behind the first one's virtual
    sweeps, so a slice that is not what the caller passed shows up as a difference between the two runs, or as an untouched state.  Bit for bit."""
    hp = _hp()
    from harmonic_power_flow_amd import api, synth
    n, hmax, k, S = 64, 11, 6, 2
    fb, fl = synth.gen(n, seed=0, outdir=str(tmp_path))
    synth.add_ties(fl, n, k)                                  # (the host planner says 12 endpoint buses for this feeder and these lines)
    st = hp.Settings(H_MAX=hmax)
    buses, lines, m, nn, c = hp.init_network(fb, fl, settings=st)
    Y = hp.build_admittance_matrices(buses, lines, st.HARMONICS)
    NE = hp.import_Norton_Equivalents(buses, True, st, INPUTS)
    P0, Q0 = buses["P"].to_numpy(float), buses["Q"].to_numpy(float)
    scale = np.stack([np.ones(n), synth.scenario_scale(n, 1)])
    seed = None
    out = {}
    for groups in (1, 4):
        dm = api._device_model(buses, Y, NE, True, st.HARMONICS, solver="block_tree", max_scenarios=S, options="HPF_MESH_SEL=0 HPF_GROUPS=%d" % groups)
        try:
            dm.set_loads(P0 * scale, Q0 * scale)
            dm.set_state(None, None, n_scen=S)
            dm.fund_pf(1e-6, 30)
            if seed is None:
                seed = dm.get_state()
            dm.set_state(*seed)                               # (the same fundamental seed for both runs)
            dm.mismatch(want_f=False)
            dm.iterate(3)
            dm.sync()
            out[groups] = (dm.get_state(), dm.tree_census())
        finally:
            dm.close()
    (Vm1, Va1), cs1 = out[1]
    (Vm4, Va4), cs4 = out[4]
    print("\nvirtual sweeps of %d + 1 right-hand sides, one group | four: max |dVm| %.1e, max |dVa| %.1e; scenario 0 vs 1: %.1e"
          % (cs4["border_unknowns"], np.abs(Vm1 - Vm4).max(), np.abs(Va1 - Va4).max(), np.abs(Vm4[0] - Vm4[1]).max()))
    for cs in (cs1, cs4):
        assert cs["ties"] == k and cs["bordered_form"] == 0 and cs["border_unknowns"] + 1 >= 128      # (the four-way split really ran)
    assert not np.array_equal(Vm4[0], Vm4[1]) and not np.array_equal(Va4[0], Va4[1])                  # (the second scenario is no copy of the first)
    assert not np.array_equal(Vm4, seed[0])                                                           # (and the steps moved the state)
    assert np.array_equal(Vm1, Vm4) and np.array_equal(Va1, Va4)


def test_many_scenarios_compaction_over_several_tiles(tmp_path):
    """1 500 scenarios of a small feeder in one handle: the slot-list compaction works in tiles of 1 024 slots, the scenario
    groups split the compacted list -- every record equals the single-scenario solve of that scenario."""
    hp = _hp()
    from harmonic_power_flow_amd import api, sweep, synth
    st, buses, Y, NE, _ = _feeder(hp, 40, 11, tmp_path, seed=11, frac_nl=0.35)
    n, S = len(buses), 1500
    P0, Q0 = buses["P"].to_numpy(float), buses["Q"].to_numpy(float)
    scale = np.stack([synth.scenario_scale(n, s) for s in range(S)])
    dm = api._device_model(buses, Y, NE, True, st.HARMONICS, solver="block_tree", max_scenarios=S)
    try:
        rec, Vm, Va = sweep.solve_scenarios(dm, P0 * scale, Q0 * scale, want_voltages=True)
    finally:
        dm.close()
    assert ((rec["flags"] & 1) == 1).all()
    assert rec["n_iter"].min() < rec["n_iter"].max()                 # (the compaction has something to do)
    dm1 = api._device_model(buses, Y, NE, True, st.HARMONICS, solver="block_tree", max_scenarios=1)
    try:
        for s in (0, 1, 700, 1023, 1024, 1025, 1499):
            r1, Vm1, Va1 = sweep.solve_scenarios(dm1, P0 * scale[s], Q0 * scale[s], want_voltages=True)
            assert r1["n_iter"][0] == rec["n_iter"][s] and r1["err"][0] == rec["err"][s]
            assert np.array_equal(Vm1[0], Vm[s]) and np.array_equal(Va1[0], Va[s])
    finally:
        dm1.close()


def test_caller_stream_carries_scenario_group_0(tmp_path):
    """hpf_set_stream: with a caller-provided HIP stream the four scenario groups of a 128-scenario solve run on that stream (group 0) and three
    streams of the handle; records and voltages are bit-identical to the solve on the handle's own stream and to a one-group solve, work queued on the
    caller's stream before the solve is ordered before it, and the handle goes back to its own stream with set_stream(None)."""
    import torch
    hp = _hp()
    from harmonic_power_flow_amd import api, sweep, synth
    st, buses, Y, NE, _ = _feeder(hp, 60, 11, tmp_path, seed=5, frac_nl=0.35)
    n, S = len(buses), 128
    P0, Q0 = buses["P"].to_numpy(float), buses["Q"].to_numpy(float)
    scale = np.stack([synth.scenario_scale(n, s) for s in range(S)])
    dm = api._device_model(buses, Y, NE, True, st.HARMONICS, solver="block_tree", max_scenarios=S)
    try:
        assert dm.scenario_groups(S) == 4 and dm.scenario_groups(127) == 3 and dm.scenario_groups(63) == 1
        ref = sweep.solve_scenarios(dm, P0 * scale, Q0 * scale, want_voltages=True)
        ts = torch.cuda.Stream()
        dm.set_stream(ts.cuda_stream)
        with torch.cuda.stream(ts):
            busy = torch.ones(1 << 24, device="cuda")
            for _ in range(20):
                busy = busy * 1.0000001                           # work on the caller's stream ahead of the solve
        got = sweep.solve_scenarios(dm, P0 * scale, Q0 * scale, want_voltages=True)
        ts.synchronize()
        dm.set_stream(None)
        dm.set_option("scenario_groups", 1)
        one = sweep.solve_scenarios(dm, P0 * scale, Q0 * scale, want_voltages=True)
    finally:
        dm.close()
    for other in (got, one):
        assert np.array_equal(ref[0].view(np.uint8), other[0].view(np.uint8))
        assert np.array_equal(ref[1], other[1]) and np.array_equal(ref[2], other[2])
    assert ((ref[0]["flags"] & 1) == 1).all()


def test_build_switches_come_from_the_option_string_and_the_environment_only_on_opt_in(tmp_path, monkeypatch):
    """a handle's numerics must not depend on the process environment.  hpf_create_opts takes the build switches of ONE
    handle as a string; the HPF_* environment is consulted only under HPF_ENV_SWITCHES=1 (which the test-suite sets).  The census tells which
    tree was built: the option string and the opted-in environment give the same handle, the environment without the opt-in gives the default."""
    hp = _hp()
    from harmonic_power_flow_amd import api
    st, buses, Y, NE, _ = _feeder(hp, 300, 51, tmp_path, seed=2)

    def census(options=None):
        from harmonic_power_flow_amd import ingest
        from harmonic_power_flow_amd.device import DeviceModel
        m, n, c = ingest.network_constants(buses)
        dev, Y_N, I_N, n_dev = ingest.norton_arrays(buses, NE, True, len(st.HARMONICS))
        dm = DeviceModel(n, m, c, st.HARMONICS, Y.rowptr, Y.col, Y.Yval, dev, Y_N, I_N, n_dev, True, solver="block_tree", max_scenarios=4, options=options)
        try:
            return dm.tree_census()
        finally:
            dm.close()
    for k in ("HPF_LAZY", "HPF_SLEAF", "HPF_COMPRESS"):
        monkeypatch.delenv(k, raising=False)
    default = census()
    assert default["lazy_leaves"] > 0 and default["bordered"] > 0 and default["compress_steps"] > 0
    by_string = census("HPF_LAZY=0 HPF_COMPRESS=0")
    assert by_string["lazy_leaves"] == 0 and by_string["compress_steps"] == 0
    assert census("HPF_SLEAF=0,HPF_LAZY=0")["bordered"] == 0                     # (comma separated; a second switch in the same string)
    monkeypatch.setenv("HPF_LAZY", "0")
    monkeypatch.setenv("HPF_COMPRESS", "0")
    assert census() == by_string                                                  # environment, opted in (conftest: HPF_ENV_SWITCHES=1)
    monkeypatch.setenv("HPF_ENV_SWITCHES", "0")
    assert census() == default                                                    # ... and ignored without the opt-in
    assert census("HPF_LAZY=0 HPF_COMPRESS=0") == by_string                       # (the option string always counts)
    # HPF_TREE_DUMP takes a path and is read from the environment only: in an option string it is ignored (no file, not even one named after the
    # rest of the string), and the switches after it still apply
    dump_dir = tmp_path / "dump"
    dump_dir.mkdir()
    monkeypatch.delenv("HPF_TREE_DUMP", raising=False)
    assert census("HPF_TREE_DUMP=%s HPF_LAZY=0" % (dump_dir / "plan.txt"))["lazy_leaves"] == 0
    assert os.listdir(dump_dir) == []
