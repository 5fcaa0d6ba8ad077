"""Newton steps with a PV bus at every role of the block-tree plan.  A PV bus has no V_m unknown and no Q equation at the fundamental; every
kernel family pads that row and column with identity on its own (loc_valid / mask_block of the 2x2 algebra, the constant-inverse and lazy leaves,
cvalid / rv of the Gauss-Jordan body, the scatter sites kst >= c, the generic wide kernels), and which of them runs depends on where in the tree
the bus sits.  The rest of the suite turns IDs 2, 3, ... into PV buses wherever synth.gen's permutation put them -- on gen(90, 0) a one-bus
linear subtree and a pass-through bus -- and judges such feeders at their fixed point only, where Newton absorbs a wrong step.  Here
tests/pv_place.py puts the PV bus on a chosen bus (tests/test_pv_place_host.py asserts, without a GPU, the role it has there), and every case is
judged like test_gpu_step_accuracy.py judges its own: f, err and J against the oracle at 1e-12, the fused step and hpf_sparse_solve against the
yardstick of tests/stepcheck.py at ETA_MAX and STEP_MAX, 3 scenarios, at the pf seed and after 3 iterations; the census shows that the plan of the
host table is the plan that ran.  Run with -m gpu on an MI355X."""
import pytest

import pv_place as pp

from conftest import INPUTS
from test_gpu_shapes import TOL_STOP, TOL_V, POLISH, _device_scenario0, _distance, _oracle_scenario0
from test_gpu_step_accuracy import S, _assert_generic_path, _judge, _net, _run, _scales, _step_gate, _vs_oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def wide_dir(tmp_path_factory):
    import wide_ne
    return wide_ne.write(str(tmp_path_factory.mktemp("wide_ne")), INPUTS)


def _pnet(tmp_path, case, wide_dir=None):
    """_net of test_gpu_step_accuracy.py on the placed files of a case"""
    fb, fl, _ = pp.write(case, tmp_path)
    net = _net(tmp_path, case.n, case.hmax, coupled=case.coupled, ne_dir=wide_dir if case.hmax > 99 else INPUTS, files=(fb, fl))
    assert net["c"] == 1 + len(case.nodes) and net["n"] == case.n
    return net


def _census(cs):
    return tuple(cs[k] for k in pp.CENSUS)


# No case is an expected failure.  At b = 100 (k_factor_q<100>, whose static pivot order loses the step gate on some PQ feeders:
# test_gpu_step_accuracy.STEP_LOSS) all 11 placements meet both gates; at b <= 52 an expected failure is not allowed: a miss there is a finding.
def _params(cases):
    return [pytest.param(c, id=c.id) for c in cases]


def _step_case(tag, case, tmp_path, wide_dir=None, sparse=True, oracle=True, census=True, judged=None, **run):
    net = _pnet(tmp_path, case, wide_dir)
    out = _run(net, **run)
    assert out["solver"] == run.get("solver", "block_tree")
    if oracle:
        _vs_oracle(net, out, ne_dir=wide_dir if case.hmax > 99 else INPUTS)
    if judged is not None:
        for state in ("seed", "iter3"):
            out[state] = [out[state][s] for s in judged]
    lost = _judge(tag, out, net, sparse=sparse)
    cs = out["census"]
    if cs is not None:
        print("STEPCHECK %-44s census %s" % (tag, " ".join("%s %d" % (k, v) for k, v in cs.items() if v)))
    if census:
        assert _census(cs) == case.census, (cs, case.census)
    return net, out, lost


# ---- a. one PV bus on each role, at every block class -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", _params(pp.SINGLE))
def test_single(case, tmp_path):
    """lin leaf / interior (root), pass, and the six dense roles of the table at b = 12, 28, 52 and 100"""
    _, _, lost = _step_case("pv " + case.id, case, tmp_path)
    _step_gate(lost)


@pytest.mark.parametrize("case", _params(pp.PAIRS))
def test_pairs(case, tmp_path):
    """c = 3: a PV bus under a PV bus, a bus that is bordered as a PQ bus under a PV Gauss-Jordan bus, a dense PV bus next to one of the 2x2
    algebra, two of one linear unit"""
    _, _, lost = _step_case("pv " + case.id, case, tmp_path)
    _step_gate(lost)


# ---- b. meshed ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,opts", [("factor-once", None), ("HPF_MESH_SEL=0", "HPF_MESH_SEL=0")])
@pytest.mark.parametrize("case", _params(pp.MESHED))
def test_meshed(case, form, opts, tmp_path):
    """three random ties, and a tie whose endpoint is the PV bus itself (its border unknowns lose the V_m one); both bordered forms"""
    # (the virtual-sweep form keeps the radial plan: no root path of a tie endpoint turns plain, so the table's census is the factor-once form's)
    net, out, lost = _step_case("pv %s %s" % (case.id, form), case, tmp_path, sparse=opts is None, oracle=opts is None, census=opts is None, options=opts)
    cs = out["census"]
    assert cs["ties"] == (len(case.ties) if isinstance(case.ties, tuple) else case.ties), cs
    assert (cs["bordered_form"] > 0) == (opts is None), cs
    _step_gate(lost)


# ---- c. shapes synth.gen does not draw --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", _params(pp.SHAPES))
def test_shapes(case, tmp_path):
    """a PV bus inside the long chains of k_chain_factor2 / k_chain_back2, the hub of a broom (its lazy leaves become constant-inverse leaves),
    the root and a leaf of a 101-bus linear unit in bundles and tree bundles, spine buses of a caterpillar.

    Two of these cases found a planner fault: a bus ABOVE a dense PV bus was eliminated before it -- the 43-bus chain
    contracted down to the hub of the broom, the compress step that made caterpillar bus 5 a pending child -- and the static pivot order of
    the PV bus's block then missed STEP_MAX (broom90-44-H51 3.28e-7 at eta 3.20e-14, caterpillar90-5-H51 4.98e-9 at eta 8.47e-14, both at
    the pf seed).  The planner now keeps the parent of a dense PV bus a dense bus and gives no PV bus the pending-child role."""
    _, _, lost = _step_case("pv " + case.id, case, tmp_path)
    _step_gate(lost)


# ---- d. switches ------------------------------------------------------------------------------------------------------------------------------
# (name, options of hpf_create, set_option pairs, capacity and scenarios, judged scenarios, what the census must show next to / instead of the table's)
def _same(cs, case):
    return _census(cs) == case.census


SWITCHES = [("HPF_LAZY=0", "HPF_LAZY=0", (), S, None, lambda cs, case: cs["lazy_leaves"] == 0),
            ("HPF_SLEAF=0", "HPF_SLEAF=0", (), S, None, lambda cs, case: cs["bordered"] == 0),
            ("HPF_COMPRESS=0", "HPF_COMPRESS=0", (), S, None, lambda cs, case: cs["compress_steps"] == 0 and _census(cs)[:5] == case.census[:5]),
            ("HPF_LINBUNDLE=0", "HPF_LINBUNDLE=0", (), S, None, _same), ("HPF_LINTREE=0", "HPF_LINTREE=0", (), S, None, _same),
            ("HPF_CHAINBUNDLE=0", "HPF_CHAINBUNDLE=0", (), S, None, _same),
            ("HPF_FUSELEVEL=0", "HPF_FUSELEVEL=0", (), S, None, lambda cs, case: _same(cs, case) and cs["fused_levels"] == 0),
            ("HPF_FUSEBACK=0", "HPF_FUSEBACK=0", (), S, None, _same),
            ("HPF_GJ_MODE=0", "HPF_GJ_MODE=0", (), S, None, lambda cs, case: cs["lazy_leaves"] == 0 and cs["fused_levels"] == 0),
            ("block_pivoting=1", None, (("block_pivoting", 1),), S, None, lambda cs, case: cs["gauss_jordan"] == cs["dense_buses"] >= case.census[0]),
            # 17 scenarios: number 16 sits in the second batch tile; judged: the first, the last of the first tile, and that one
            ("S=17", None, (), 17, (0, 15, 16), _same)]


@pytest.mark.parametrize("variant", [v[0] for v in SWITCHES])
@pytest.mark.parametrize("hmax", [27, 51])
@pytest.mark.parametrize("node", [20, 6])
def test_switches(node, hmax, variant, tmp_path):
    """PV on the bus that would be bordered (20) and on a compress-role bus with five dense children (6), b = 28 and 52, under every switch that
    moves the bus or its neighbours to another kernel"""
    name, opts, set_opts, n_scen, judged, want = next(v for v in SWITCHES if v[0] == variant)
    case = pp.case("gen", (node,), hmax)
    net, out, lost = _step_case("pv %s %s" % (case.id, name), case, tmp_path, sparse=False, oracle=False, census=False, judged=judged,
                                S_=n_scen, cap=n_scen, options=opts, set_opts=set_opts)
    assert want(out["census"], case), (name, out["census"], case.census)
    _step_gate(lost)


# ---- e. uncoupled, wide, dense ------------------------------------------------------------------------------------------------------------------
def test_uncoupled(tmp_path):
    """b = 30, uncoupled Norton data: no dense bus, the PV buses 8 (lin interior in the coupled plan) and 6 (a Gauss-Jordan bus there) both run in
    the 2x2 algebra"""
    case = pp.UNCOUPLED[0]
    _, out, lost = _step_case("pv " + case.id, case, tmp_path, census=False)
    assert out["census"]["dense_buses"] == 0, out["census"]
    _step_gate(lost)


def test_wide(tmp_path, wide_dir):
    """b = 102: every bus a dense bus of the generic 256-thread kernels, which pad the PV rows themselves"""
    case = pp.WIDE[0]
    net, out, lost = _step_case("pv " + case.id, case, tmp_path, wide_dir=wide_dir, census=False)
    _assert_generic_path(out, net)
    _step_gate(lost)


def test_dense_path_control(tmp_path):
    """the dense rocSOLVER path, on which the position of a bus cannot matter"""
    case = pp.case("gen", (20,), 27)
    _, _, lost = _step_case("pv %s dense" % case.id, case, tmp_path, sparse=False, oracle=False, census=False, solver="dense")
    _step_gate(lost)


# ---- f. the whole solve -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hmax", [11, 27, 51, 99])
def test_whole_solve_against_the_reference(hmax, tmp_path):
    """PV on bus 20, scenario 0: the stopped state within TOL_STOP of the oracle's, the fixed point at the parity bar TOL_V -- the two bounds of
    test_gpu_shapes.py.  (Its oracle cache is keyed by file name and width: this is the only test here that uses it, one feeder per width.)"""
    case = pp.case("gen", (20,), hmax)
    net = _pnet(tmp_path, case)
    r, Vm_o, Va_o, err_o = _oracle_scenario0(net, POLISH)
    assert r["err_h"] <= 1e-4 and r["n_iter_h"] < 50
    n_it, stop, Vm, Va, err_d, cs = _device_scenario0(net, "block_tree", POLISH)
    assert _census(cs) == case.census, cs
    sU, sVm = _distance(stop[0], stop[1], r["Vm_raw"], r["Va_raw"])
    dU, dVm = _distance(Vm, Va, Vm_o, Va_o)
    print("\nSTEPCHECK pv fixed point %-20s iterations %d (oracle %d) at the stop max|dU| %.2e max|d|Vm|| %.2e; continued: err %.1e (oracle %.1e) "
          "max|dU| %.2e max|d|Vm|| %.2e" % (case.id, n_it, r["n_iter_h"], sU, sVm, err_d, err_o, dU, dVm))
    assert sU <= TOL_STOP and sVm <= TOL_STOP
    assert dU <= TOL_V and dVm <= TOL_V


def test_a_scenario_of_a_batch_is_its_solve_alone(tmp_path):
    """PV on bus 20, b = 28: the batch of 3 against three single-scenario solves, bit for bit (states and stats)"""
    from harmonic_power_flow_amd import api
    case = pp.case("gen", (20,), 27)
    net = _pnet(tmp_path, case)
    st, buses = net["st"], net["buses"]
    sc_ = _scales(net["n"], S)
    P, Q = buses["P"].to_numpy(float) * sc_, buses["Q"].to_numpy(float) * sc_

    def solve(cap, loads):
        dm = api._device_model(buses, net["Y"], net["NE"], True, st.HARMONICS, solver="block_tree", max_scenarios=cap)
        try:
            out = []
            for p, q in loads:
                n_scen = 1 if p.ndim == 1 else p.shape[0]
                dm.set_loads(p, q)
                dm.set_state(None, None, n_scen=n_scen)
                dm.fund_pf(1e-6, 30)
                dm.solve(1e-4, 50)
                Vm, Va = dm.get_state()
                out.append((dm.stats().copy(), Vm.copy(), Va.copy()))
        finally:
            dm.close()
        return out
    alone = solve(1, [(P[s], Q[s]) for s in range(S)])
    batch = solve(S, [(P, Q)])[0]
    assert (batch[0]["flags"] & 1).all() and (batch[0]["err"] <= 1e-4).all()
    for s in range(S):
        for k in ("n_iter", "flags", "err", "thd_max"):
            assert batch[0][k][s:s + 1].tobytes() == alone[s][0][k][:1].tobytes(), (s, k)
        assert batch[1][s].tobytes() == alone[s][1][0].tobytes() and batch[2][s].tobytes() == alone[s][2][0].tobytes(), s
