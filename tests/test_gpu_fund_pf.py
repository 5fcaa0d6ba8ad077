"""The fundamental power flow (pf, HG:195-275) on the device against tests/pf_ref.py, the long-double restatement pinned to the oracle's pf in
tests/test_pf_ref_host.py -- not by its end state alone.  Newton absorbs a wrong step (the header of test_gpu_step_accuracy.py), in the pf
loop as in the harmonic one, so converged voltages and an iteration count cannot see a wrong Jacobian entry or a lossy elimination:

  * assembly: hpf_fund_mismatch and hpf_fund_jacobian(scen) per scenario of a batch at the flat start, at a perturbed state and at the
    converged pf state, with and without PV buses, on a dense-solver and on a block-tree handle;
  * one pf Newton step (hpf_fund_pf with max_iter = 1) of every form the library has -- dense LU, the level-parallel 2x2 elimination
    (k_lin_level_factor / _back, b <= 100), the one-thread tree walk (k_lin_factor<true> / k_lin_back<true>, b > 100), the dense LU of a
    meshed block-tree handle -- judged with stepcheck.judge on the reference's J and f: eta <= ETA_MAX, step error <= STEP_MAX;
  * a batch whose scenarios stop after different numbers of iterations (the active list of the pf loop) against the oracle's pf on each load."""
import numpy as np
import pytest
import scipy.sparse as sp

import pf_ref
import shapes
import stepcheck as sc
import test_gpu_step_accuracy as sa
from conftest import INPUTS

pytestmark = pytest.mark.gpu

S = 3
N_BUS = 90                     # the feeders of the step and batch cases (Nf <= 179)
N_ASM = 12                     # the feeders of the assembly cases, see test_assembly
F_TOL = 1e-13                  # |f - f_ref| <= F_TOL max(1, |f_ref|): the bar of test_gpu_parity.test_fundamental_pf_kernels
J_TOL = 1e-12                  # |J - J_ref| <= J_TOL max |J_ref|: the suite's bar for Jacobian entries


@pytest.fixture(scope="module")
def wide_dir(tmp_path_factory):
    import wide_ne
    return wide_ne.write(str(tmp_path_factory.mktemp("wide_ne")), INPUTS)


def _handle(net, solver, S_, scale):
    """a handle of S_ scenarios with the loads P, Q * scale [S_][n] set -> (dm, P, Q)"""
    from harmonic_power_flow_amd import api
    buses = net["buses"]
    dm = api._device_model(buses, net["Y"], net["NE"], True, net["st"].HARMONICS, solver=solver, max_scenarios=S_)
    P, Q = buses["P"].to_numpy(float) * scale, buses["Q"].to_numpy(float) * scale
    dm.set_loads(P, Q)
    return dm, P, Q


def _Y1(net):
    Y = net["Y"]
    return pf_ref.dense_Y1(np.asarray(Y.rowptr), np.asarray(Y.col), np.asarray(Y.Yval)[0], net["n"])


def _flat(dm, S_):
    dm.set_state(None, None, n_scen=S_)
    return dm.get_state()


def _perturbed(flat, n, S_):
    """angles within +-0.3 rad, magnitudes in 0.9 ... 1.1 at every bus but the slack, another draw per scenario; the harmonics stay"""
    Vm, Va = flat[0].copy(), flat[1].copy()
    for s in range(S_):
        rng = np.random.default_rng(4242 + s)
        Vm[s, 1:n] = rng.uniform(0.9, 1.1, n - 1)
        Va[s, 1:n] = rng.uniform(-0.3, 0.3, n - 1)
    return Vm, Va


# ---- assembly -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pv", [0, 2])
@pytest.mark.parametrize("solver", ["dense", "block_tree"])
def test_assembly(solver, n_pv, tmp_path):
    """f at F_TOL max(1, |f|) and J at J_TOL relative, per scenario, at the flat start, a perturbed state and the converged pf state.

    The feeder: synth.gen(12).  F_TOL is an absolute 1e-13 wherever |f| < 1 (flat start, converged state), and a float64 evaluation of
    V conj(Y1 V) cannot be closer to the long-double value than the rounding of its terms, about eps |Y1|_inf V^2: the oracle's own float64
    mismatch is 3.4e-13 away on synth.gen(90) (|Y1|_inf = 9 016 p.u.; synth.gen scales its impedances with 20 / n) and 1.3e-13 - 2.0e-13 on
    synth.gen(40), but 4e-14 on synth.gen(12) (|Y1|_inf = 983, the size of the golden nets' 859 and 734, where the suite uses this bar).
    The kernels are one thread per bus and per stored entry, so 12 buses take every branch 90 do: slack, PV, PQ and nonlinear rows, c = 1
    and c = 3.  The 90-bus feeders are covered by the step cases below, whose eta is formed with the reference's J and f.
    hpf_fund_jacobian serves a block-tree handle too (it allocates the dense Nf x Nf array on demand), so J is the handle's own in both."""
    net = sa._net(tmp_path, N_ASM, 11, n_pv=n_pv)
    n, c = net["n"], net["c"]
    assert c == 1 + n_pv
    from harmonic_power_flow_amd import synth
    scale = np.stack([synth.scenario_scale(n, s) for s in range(S)])
    dm, P, Q = _handle(net, solver, S, scale)
    Y1 = _Y1(net)
    worst = {}
    try:
        assert dm.solver == solver and dm.Nf == 2 * n - 1 - c
        flat = _flat(dm, S)
        pert = _perturbed(flat, n, S)
        dm.set_state(*flat)
        n_iter, err, _ = dm.fund_pf(1e-6, 30)
        assert (err <= 1e-6).all() and (n_iter >= 2).all(), (n_iter, err)
        conv = dm.get_state()
        for tag, (Vm, Va) in (("flat", flat), ("perturbed", pert), ("converged", conv)):
            dm.set_state(Vm, Va)
            f, e = dm.mismatch(fund=True)
            df = dj = 0.0
            for s in range(S):
                f_r = pf_ref.mismatch(Y1, Vm[s, :n], Va[s, :n], P[s], Q[s], c)
                J_r = pf_ref.jacobian(Y1, Vm[s, :n], Va[s, :n], c)
                fs = max(1.0, float(np.abs(f_r).max()))
                df = max(df, float(np.abs(f[s] - f_r).max()) / fs)
                dj = max(dj, float(np.abs(dm.jacobian(s, fund=True) - J_r).max() / np.abs(J_r).max()))
                assert abs(e[s] - float(np.abs(f_r).max())) <= F_TOL * fs, (tag, s)
            worst[tag] = (df, dj)
    finally:
        dm.close()
    print("\nPFASM %-10s c=%d  " % (solver, c) + "  ".join("%s: f %.1e J %.1e" % (k, v[0], v[1]) for k, v in worst.items()))
    for tag, (df, dj) in worst.items():
        assert df <= F_TOL and dj <= J_TOL, (tag, df, dj)


# ---- one pf Newton step of every form -------------------------------------------------------------------------------------------------
#        name                  H_MAX  solver        n_pv ties shape   form of the pf step
FORMS = [("dense",               11, "dense",       0,   0,   None),  # dense LU of the Nf x Nf system
         ("tree levels",         11, "block_tree",  0,   0,   None),  # k_lin_level_factor / _back, fund = 1: one launch per height
         ("tree walk",          101, "block_tree",  0,   0,   None),  # b = 102: k_lin_factor<true> / k_lin_back<true>, one thread per scenario
         ("meshed",              11, "block_tree",  0,   3,   None),  # loop-closing lines: the block-tree handle's pf goes through the dense LU
         ("tree levels 2 PV",    11, "block_tree",  2,   0,   None),
         ("tree walk 2 PV",     101, "block_tree",  2,   0,   None),
         ("tree levels path",    11, "block_tree",  0,   0,   "path"),   # 89 heights of one bus
         ("tree levels star",    11, "block_tree",  0,   0,   "star")]   # one height of 89 buses


def _form_net(form, tmp_path, wide_dir):
    name, hmax, solver, n_pv, ties, shape = form
    files = shapes.write(shape, N_BUS, str(tmp_path)) if shape else None
    return sa._net(tmp_path, N_BUS, hmax, n_pv=n_pv, ties=ties, ne_dir=wide_dir if hmax > 99 else INPUTS, files=files)


def _check_form(dm, form, net):
    name, hmax, solver, n_pv, ties, shape = form
    assert dm.solver == solver and dm.c == 1 + n_pv
    if solver == "block_tree":
        cs = dm.tree_census()
        assert cs["ties"] == ties, cs
        # the walk is the pf of the handles without multi-wave kernels (wave_block_size 0: 100 < 2 Hn <= 112), the levels of the others
        assert (2 * dm.Hn > 100) == ("walk" in name)


@pytest.mark.parametrize("form", FORMS, ids=[f[0].replace(" ", "_") for f in FORMS])
def test_one_pf_step(form, tmp_path, wide_dir):
    """dx = x0 - x1 across hpf_fund_pf(max_iter = 1), x = the fundamental part of the state in the reference's order, from the flat start and
    from the perturbed state, per scenario; J and f are the reference's (float64 casts of the long-double values)."""
    from harmonic_power_flow_amd import synth
    net = _form_net(form, tmp_path, wide_dir)
    n, c = net["n"], net["c"]
    scale = np.stack([synth.scenario_scale(n, s) for s in range(S)])
    dm, P, Q = _handle(net, form[2], S, scale)
    Y1 = _Y1(net)
    ynorm = float(np.abs(Y1).sum(axis=1).max())
    worst = [0.0, 0.0]
    try:
        _check_form(dm, form, net)
        flat = _flat(dm, S)
        for tag, (Vm0, Va0) in (("flat", flat), ("perturbed", _perturbed(flat, n, S))):
            dm.set_state(Vm0, Va0)
            n_iter, err, hist = dm.fund_pf(0.0, 1)
            assert (n_iter == 1).all(), n_iter
            Vm1, Va1 = dm.get_state()
            assert np.array_equal(Vm1[:, n:], Vm0[:, n:]) and np.array_equal(Va1[:, n:], Va0[:, n:])      # a pf step moves the fundamental alone
            assert np.array_equal(Vm1[:, :c], Vm0[:, :c]) and np.array_equal(Va1[:, 0], Va0[:, 0])         # ... and no fixed quantity
            for s in range(S):
                J = sp.csr_matrix(np.asarray(pf_ref.jacobian(Y1, Vm0[s, :n], Va0[s, :n], c), dtype=np.float64))
                f = np.asarray(pf_ref.mismatch(Y1, Vm0[s, :n], Va0[s, :n], P[s], Q[s], c), dtype=np.float64)
                dx = sc.stacked(Vm0[s, :n], Va0[s, :n], c) - sc.stacked(Vm1[s, :n], Va1[s, :n], c)
                eta, se, _ = sc.judge(J, f, dx)
                worst = [max(worst[0], eta), max(worst[1], se)]
                # the error the loop recorded is the mismatch of the state it left behind, to the rounding of a float64 evaluation of
                # V conj(Y1 V): terms of up to |Y1|_inf V^2 each (|Y1|_inf = 9e3 on synth.gen(90), 5e4 on `path`, 1e5 on `star`, whose impedances
                # are smaller); the oracle's own float64 mismatch is 0.17 eps |Y1|_inf away from the long-double one on synth.gen(90)
                f1 = pf_ref.mismatch(Y1, Vm1[s, :n], Va1[s, :n], P[s], Q[s], c)
                assert abs(hist[s, 0] - float(np.abs(f1).max())) <= 4 * np.finfo(float).eps * ynorm * float(Vm1[s, :n].max()) ** 2, (tag, s)
                assert eta <= sc.ETA_MAX and se <= sc.STEP_MAX, (form[0], tag, s, eta, se)
    finally:
        dm.close()
    print("\nPFSTEP %-20s worst eta %.2e step err %.2e" % (form[0], worst[0], worst[1]))


# ---- a batch that stops scenario by scenario ----------------------------------------------------------------------------------------------
PF_SCALES = (1e-6, 0.01, 1.0, 4.0, 6.0)       # times synth.scenario_scale: the oracle's pf takes 0, 2, 3, 4 and 4 iterations (asserted)


@pytest.mark.parametrize("hmax", [11, 101], ids=["tree_levels", "tree_walk"])
def test_batched_pf_stops_per_scenario(hmax, tmp_path, wide_dir):
    """S = 5, loads from 1e-6 to 6 times nominal: every scenario equals the oracle's pf on its load alone -- n_iter equal, state within
    1e-13 (the bar V_pf is held to) -- although the scenarios leave the loop's active list at different iterations."""
    import hpf_oracle as o
    from harmonic_power_flow_amd import synth
    net = sa._net(tmp_path, N_BUS, hmax, ne_dir=wide_dir if hmax > 99 else INPUTS)
    n = net["n"]
    S_ = len(PF_SCALES)
    scale = np.stack([k * synth.scenario_scale(n, s) for s, k in enumerate(PF_SCALES)])
    onet = o.init_network(net["fb"], net["fl"])
    rowptr, col, Yval = o.build_admittance_matrices(onet, [1])
    P0, Q0 = onet.P.copy(), onet.Q.copy()
    ref = []
    for s in range(S_):
        onet.P, onet.Q = P0 * scale[s], Q0 * scale[s]
        Vm, Va, err_t, it = o.pf(onet, rowptr, col, Yval)
        ref.append((Vm[:n].copy(), Va[:n].copy(), it))
    its = [r[2] for r in ref]
    assert its[0] == 0 and len(set(its)) >= 4 and max(its) < 30, its                    # different stopping points, one scenario never starts
    dm, P, Q = _handle(net, "block_tree", S_, scale)
    try:
        assert (2 * dm.Hn > 100) == (hmax > 99)
        dm.set_state(None, None, n_scen=S_)
        n_iter, err, hist = dm.fund_pf(1e-6, 30)
        Vm, Va = dm.get_state()
    finally:
        dm.close()
    dv = max(max(np.abs(Vm[s, :n] - ref[s][0]).max(), np.abs(Va[s, :n] - ref[s][1]).max()) for s in range(S_))
    print("\nPFBATCH H_MAX=%d n_iter %s (oracle %s) max |dV| %.2e" % (hmax, n_iter.tolist(), its, dv))
    assert n_iter.tolist() == its
    assert (err <= 1e-6).all()
    assert dv <= 1e-13
