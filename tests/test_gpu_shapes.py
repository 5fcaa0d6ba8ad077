"""The block-tree solver on the feeders of tests/shapes.py -- deep paths, caterpillars, brooms, stars of 90 and 300 buses, a full binary tree,
feeders of one bus class --, the shapes at which the planner's capacities bind and which synth.gen's random trees never reach
(tests/test_shapes_plan_host.py asserts, without a GPU, that they do bind).  Per case, 3 scenarios of synth.scenario_scale:
  a. the default step and hpf_sparse_solve against the yardstick of tests/stepcheck.py at the gates of test_gpu_step_accuracy.py, f / err / J
     against the oracle at 1e-12 (rows of 90 and 300 entries through k_mismatch and the CSR Jacobian kernels);
  b. launch-shape identities, bit for bit: the tree walk with lists longer than its LDS ring against the per-depth launches, the back tail
     with hundreds of one-leaf families against the four launches; the forms of the 2x2 algebra and of the chains at the step gates;
  c. the fixed point against the reference's algorithm at the parity bar 1e-8, block tree and dense rocSOLVER;
  d. the one-class feeders: no nonlinear bus (no dense bus at all), one harmonic (blocks of 2)."""
import numpy as np
import pytest

import shapes
from conftest import INPUTS
from test_gpu_back_tail import _on_off
from test_gpu_back_walk import _variants
from test_gpu_step_accuracy import S, _judge, _run, _scales, _step_gate, _vs_oracle

pytestmark = pytest.mark.gpu

IDS = [c.id for c in shapes.CASES]
TOL_V = 1e-8            # the parity bar of test_gpu_parity.py


def _hp():
    import harmonic_power_flow_amd as hp
    return hp


def _shape_net(tmp_path, case, hmax=None, coupled=True):
    """_net of test_gpu_step_accuracy.py for the CSV pair of a shape"""
    hp = _hp()
    fb, fl = shapes.write(case.name, case.n, str(tmp_path))
    st = hp.Settings(H_MAX=hmax or case.hmax)
    buses, lines, m, nn, c = hp.init_network(fb, fl, settings=st)
    Y = hp.build_admittance_matrices(buses, lines, st.HARMONICS)
    NE = hp.import_Norton_Equivalents(buses, coupled, st, INPUTS)
    return dict(st=st, buses=buses, Y=Y, NE=NE, c=c, n=nn, coupled=coupled, fb=fb, fl=fl)


def _census_line(tag, cs):
    print("STEPCHECK %-44s census %s" % (tag, " ".join("%s %d" % (k, v) for k, v in cs.items() if v)))


# ---- a. step accuracy -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", shapes.CASES, ids=IDS)
def test_step_against_the_yardstick(case, tmp_path):
    net = _shape_net(tmp_path, case)
    # no_nl has no harmonic source: its first Newton step lands on harmonic voltages of exactly zero, where the polar Jacobian has zero
    # columns (d/dtheta of V e^{j theta} at V = 0) and is exactly singular -- the oracle stops after that one iteration.  A state "after 3
    # iterations" has no Newton step to judge there (SuperLU: "Factor is exactly singular"), so this case is judged at the pf seed alone.
    out = _run(net, states=("seed",) if case.name == "no_nl" else ("seed", "iter3"))
    out.setdefault("iter3", [])
    cs = out["census"]
    lost = _judge("shape " + case.id, out, net, sparse=True)
    _census_line("shape " + case.id, cs)
    # the handle runs the plan the host tests assert
    assert (cs["dense_buses"], cs["gauss_jordan"], cs["levels"]) == (case.dense, case.gj, case.levels), cs
    assert (cs["const_leaves"], cs["bordered"], cs["compress_steps"]) == (case.leaves, case.bordered, case.roles // 2), cs
    _vs_oracle(net, out)
    _step_gate(lost)


# ---- b. launch-shape identities -------------------------------------------------------------------------------------------------------
def _solver(net):
    from harmonic_power_flow_amd import api
    st, buses = net["st"], net["buses"]
    P0, Q0 = buses["P"].to_numpy(float), buses["Q"].to_numpy(float)
    scale = _scales(net["n"], S)

    def run():
        dm = api._device_model(buses, net["Y"], net["NE"], True, st.HARMONICS, solver="block_tree", max_scenarios=S)
        try:
            dm.set_loads(P0 * scale, Q0 * scale)
            dm.set_state(None, None, n_scen=S)
            dm.fund_pf(1e-6, 30)
            it, err, _ = dm.solve(1e-4, 50)
            dm.mismatch(want_f=False)               # one more step behind the solve: every scenario takes it, none frozen
            dm.iterate(1)
            dm.sync()
            Vm, Va = dm.get_state()
            census = dm.tree_census()
        finally:
            dm.close()
        return dict(it=it, err=err, Vm=Vm, Va=Va, census=census)
    return run


@pytest.mark.parametrize("name", ["allnl_path", "caterpillar", "binary_allnl", "comb_allnl"])
def test_walk_longer_than_its_ring_matches_the_depth_launches(name, tmp_path, monkeypatch):
    """allnl_path walks one list of 82 buses and caterpillar one of 38 through a ring of WALK_SLOTS = 32: the ring wraps, but every dependency
    is at most 3 records back and still in its slot.  comb_allnl is the case of the re-read: in its list of 67 buses a parent sits 33 records
    back and a compress child 66, their slots are overwritten and their x comes back from HBM (tests/test_shapes_plan_host.py asserts both
    from the plan).  binary_allnl fills all WALK_LISTS lists.  States and counts are those of the per-depth launches."""
    case = shapes.case(name)
    base = _variants(_solver(_shape_net(tmp_path, case)), monkeypatch)
    print("\nSTEPCHECK walk %-20s iterations %s back_walks %d" % (case.id, base["it"].tolist(), base["census"]["back_walks"]))
    assert (base["err"] <= 1e-4).all() and np.isfinite(base["Vm"]).all()


@pytest.mark.parametrize("name,n", [("star_allnl", 300), ("star_allnl", 90), ("caterpillar", 90)])
def test_tail_of_one_leaf_families_matches_the_four_launches(name, n, tmp_path, monkeypatch):
    """298 / 88 families of one leaf under one hub (4 of them lazy), 43 families along a spine: the tail against one launch per nesting order"""
    case = shapes.case(name, n)
    # (blocks of 52: groups below 16 scenarios take the fused per-depth launches by default; the tail runs behind the walk, opened to every
    # group size as in test_gpu_back_tail.py's meshed case)
    extra = {"HPF_BACKWALK_MIN": "1", "HPF_BACKWALK_MAX": "4096"} if case.hmax == 51 else None
    on = _on_off(_solver(_shape_net(tmp_path, case)), monkeypatch, extra)
    print("\nSTEPCHECK tail %-20s iterations %s back_tails %d" % (case.id, on["it"].tolist(), on["census"]["back_tails"]))
    assert (on["err"] <= 1e-4).all() and np.isfinite(on["Vm"]).all()


LIN_CASES = [("path", 51), ("one_nl_deep", 51), ("linstar_under_nl", 51), ("linstar_under_nl", 11)]


@pytest.mark.parametrize("switch", ["HPF_LINBUNDLE=0", "HPF_LINTREE=0", "HPF_CHAINBUNDLE=0"])
@pytest.mark.parametrize("name,hmax", LIN_CASES)
def test_forms_of_the_2x2_algebra_on_long_chains_and_large_units(name, hmax, switch, tmp_path):
    """a chain of 58 / 88 pass-through buses, a linear unit of 101 buses with 100 at one height: each switch at the step gates.  Only three
    combinations move the plan to another form (shapes.LIN_SWITCHED, asserted from the dump in tests/test_shapes_plan_host.py: tree bundles
    and a launch per height on linstar_under_nl); on path and one_nl_deep, which have no all-linear subtree and whose chain has its own
    launches by default, the switches leave the plan as it is and the run repeats the default step with the option parsed."""
    case = shapes.case(name, hmax=hmax)
    net = _shape_net(tmp_path, case)
    out = _run(net, options=switch)
    tag = "shape %s %s" % (case.id, switch)
    lost = _judge(tag, out, net)
    _census_line(tag, out["census"])
    _step_gate(lost)


# ---- c. fixed point -------------------------------------------------------------------------------------------------------------------
POLISH = 4              # Newton iterations behind the stop rule, on the device; the oracle runs on until err <= 1e-13 (at most 8 more)
TOL_STOP = 1e-6         # what the stop rule (err <= 1e-4) itself guarantees between two stopped iterates: the bound of test_gpu_parity.py


_ORACLE = {}            # the oracle's run of a case, shared by the two solvers' tests (star_allnl at 90 buses costs it half a minute: 88 coupled
                        # nonlinear buses under one hub fill SuperLU's factors)


def _oracle_scenario0(net, polish):
    """the reference's algorithm on scenario 0 (the model's loads times scenario_scale(n, 0)) -> (result of hpf at its stop, Vm, Va, err after
    `polish` > 0: continued to its fixed point, i.e. until err <= 1e-13 or the mismatch stops falling, at most 2 * POLISH iterations)"""
    import hpf_oracle as o
    key = (net["fb"].rsplit("/", 1)[-1], len(net["st"].HARMONICS), net["coupled"], bool(polish))
    if key in _ORACLE:
        return _ORACLE[key]
    onet = o.init_network(net["fb"], net["fl"])
    sc0 = _scales(onet.n, 1)[0]
    onet.P, onet.Q = onet.P * sc0, onet.Q * sc0
    r = o.hpf(onet, net["st"].HARMONICS, net["coupled"], INPUTS)
    Vm, Va, err = r["Vm_raw"].copy(), r["Va_raw"].copy(), r["err_h"]
    for _ in range(2 * POLISH if polish else 0):
        r2 = o.hpf_from_model(r["model"], Vm.copy(), Va.copy(), thresh_h=1e-13, max_iter_h=1)
        fell = r2["err_h"] < 0.5 * err
        if r2["n_iter_h"] == 0 or (not fell and err <= 1e-8):      # (at the round-off floor the mismatch wanders; keep the lower iterate)
            break
        Vm, Va, err = r2["Vm_raw"], r2["Va_raw"], r2["err_h"]
    _ORACLE[key] = (r, Vm, Va, err)
    return _ORACLE[key]


def _device_scenario0(net, solver, polish):
    """dm.solve on scenario 0, then `polish` more iterations -> (count of dm.solve, state at the stop, Vm, Va, err at the end, census)"""
    from harmonic_power_flow_amd import api
    st, buses = net["st"], net["buses"]
    sc0 = _scales(net["n"], 1)
    dm = api._device_model(buses, net["Y"], net["NE"], net["coupled"], st.HARMONICS, solver=solver, max_scenarios=1)
    try:
        dm.set_loads(buses["P"].to_numpy(float) * sc0, buses["Q"].to_numpy(float) * sc0)
        dm.set_state(None, None, n_scen=1)
        dm.fund_pf(1e-6, 30)
        it, err, _ = dm.solve(1e-4, 50)
        n_it = int(it[0])
        assert err[0] <= 1e-4 and n_it < 50, (n_it, err)
        stop = dm.get_state()
        if polish:
            dm.mismatch(want_f=False)
            dm.iterate(polish)
            dm.sync()
        Vm, Va = dm.get_state()
        err_end = float(dm.mismatch()[1][0])
        census = dm.tree_census() if solver == "block_tree" else None
    finally:
        dm.close()
    return n_it, (stop[0][0], stop[1][0]), Vm[0], Va[0], err_end, census


def _distance(Vm, Va, Vm_o, Va_o):
    """max |dU| and max |d|Vm|| (the raw polar pair is not unique: a negative magnitude with the angle turned by pi is the same voltage)"""
    return float(np.abs(Vm * np.exp(1j * Va) - Vm_o * np.exp(1j * Va_o)).max()), float(np.abs(np.abs(Vm) - np.abs(Vm_o)).max())


@pytest.mark.parametrize("solver", ["block_tree", "dense"])
@pytest.mark.parametrize("case", shapes.CASES, ids=IDS)
def test_fixed_point_against_the_reference(case, solver, tmp_path):
    """Two bounds, as in test_gpu_parity.py.  The state dm.solve returns lies within TOL_STOP of the oracle's stopped state: both are iterates
    below the threshold, possibly of different iteration counts, and the stop rule promises no more.  Continued past the stop to the fixed
    point on both sides, they agree at the parity bar TOL_V.  Every figure is printed.  no_nl is not continued: its first step is exact and
    the Jacobian behind it singular (see test_step_against_the_yardstick), so it meets TOL_V at the stop."""
    polish = 0 if case.name == "no_nl" else POLISH
    net = _shape_net(tmp_path, case)
    r, Vm_o, Va_o, err_o = _oracle_scenario0(net, polish)
    assert r["err_h"] <= 1e-4 and r["n_iter_h"] < 50
    n_it, stop, Vm, Va, err_d, _ = _device_scenario0(net, solver, polish)
    sU, sVm = _distance(stop[0], stop[1], r["Vm_raw"], r["Va_raw"])
    dU, dVm = _distance(Vm, Va, Vm_o, Va_o)
    print("\nSTEPCHECK fixed point %-24s %-10s iterations %d (oracle %d) at the stop max|dU| %.2e max|d|Vm|| %.2e; continued: err %.1e (oracle %.1e) "
          "max|dU| %.2e max|d|Vm|| %.2e" % (case.id, solver, n_it, r["n_iter_h"], sU, sVm, err_d, err_o, dU, dVm))
    assert sU <= TOL_STOP and sVm <= TOL_STOP
    assert dU <= TOL_V and dVm <= TOL_V


# ---- d. degenerate classes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coupled", [True, False])
def test_feeder_without_nonlinear_buses(coupled, tmp_path):
    """no dense bus, no level, an empty walk: the block-tree handle is 2x2 algebra alone and answers like the oracle, in its one iteration"""
    case = shapes.case("no_nl")
    net = _shape_net(tmp_path, case, coupled=coupled)
    r, Vm_o, Va_o, _ = _oracle_scenario0(net, 0)
    assert r["n_iter_h"] == 1
    n_it, _, Vm, Va, _, cs = _device_scenario0(net, "block_tree", 0)
    assert cs["dense_buses"] == 0 and cs["levels"] == 0, cs
    dU, dVm = _distance(Vm, Va, Vm_o, Va_o)
    print("\nSTEPCHECK no_nl coupled=%d iterations %d max|dU| %.2e max|d|Vm|| %.2e" % (coupled, n_it, dU, dVm))
    assert n_it == 1
    assert dU <= TOL_V and dVm <= TOL_V


@pytest.mark.parametrize("n", [90, 300])
def test_star_with_one_harmonic(n, tmp_path):
    """H_MAX = 1: blocks of 2, a hub row of n entries; hpf_create takes it and the step meets the gates (hpf_sparse_solve may refuse, -3)"""
    case = shapes.case("star", n)
    net = _shape_net(tmp_path, case, hmax=1)
    # judged at the pf seed: with one harmonic this feeder has converged after 3 iterations, and a step that small cannot be measured as
    # the difference of two states (stepcheck.newton_steps) -- tests/test_shapes_plan_host.py shows on the host that the refined reference
    # solution itself, passed through that difference, misses the eta gate there
    out = _run(net, states=("seed",))
    out["iter3"] = []
    lost = _judge("shape star-%d-H1" % n, out, net, sparse=True)
    _census_line("shape star-%d-H1" % n, out["census"])
    _vs_oracle(net, out)
    _step_gate(lost)
