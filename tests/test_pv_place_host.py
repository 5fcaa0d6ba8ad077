"""tests/pv_place.py without a GPU: place() is a relabelling of the feeder (same admittance matrices under the permutation, c PV buses more,
m unchanged); every row of pv_place.CASES has the role the table claims, as the PQ bus it was and as the PV bus it becomes, so that a later
planner change which moves a PV bus out of its role fails here and not silently on the GPU; the planner's rules keyed on the number
of PV buses (hpf_tree_plan.hpp: a PV bus is no parent of lazy leaves, no bordered bus, no parent of a vector-only bordered bus, no pending
child of a compress step, and its parent is no pass-through bus) hold on every plan; the dependency invariants of test_tree_plan_host.py hold with and without compress steps; and the oracle solves every case in
every scenario the GPU tests use (tests/test_gpu_pv_positions.py) inside their iteration limits."""
import os
import sys
import types

import numpy as np
import pytest

import pv_place as pp
import test_shapes_plan_host as shapes_host
from conftest import INPUTS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

PLANNED = [c for c in pp.CASES if c.hmax <= 99]          # (b > 100 runs the plain tree, which hpf_tree_plan does not dump: see test_gpu_pv_positions.py)
IDS = [c.id for c in PLANNED]
S = 3                                                    # scenarios of the GPU tests


def _hp():
    import harmonic_power_flow_amd as hp
    return hp


def _dense(Y, n):
    A = np.zeros((Y.Yval.shape[0], n, n), dtype=np.complex128)
    rows = np.repeat(np.arange(n), np.diff(Y.rowptr))
    A[:, rows, Y.col] = Y.Yval
    return A


@pytest.mark.parametrize("nodes", [[1], [20], [2], [6, 5], [20, 14], [17, 3], [2, 1], [58, 57, 56]])
def test_place_is_a_relabelling(nodes, tmp_path):
    """Y_h of the placed feeder is P Y_h P^T, entry for entry: every line admittance is the same number; a diagonal entry is minus the
    left-to-right sum of its row in column order (admittance.py), and the relabelling reorders the columns, so it is compared with that sum
    taken in the placed order -- exactly -- and with the original's to 4 ulp."""
    hp = _hp()
    from harmonic_power_flow_amd import ingest, synth
    st = hp.Settings(H_MAX=11)
    (tmp_path / "a").mkdir()
    fb0, fl0 = synth.gen(pp.N_GEN, seed=0, outdir=str(tmp_path / "a"), zscale=pp.Z)
    fb, fl = synth.gen(pp.N_GEN, seed=0, outdir=str(tmp_path), zscale=pp.Z)
    new = pp.place(fb, fl, nodes)
    b0, l0, m0, n0, c0 = hp.init_network(fb0, fl0, settings=st)
    b1, l1, m1, n1, c1 = hp.init_network(fb, fl, settings=st)
    ingest.validate_bus_order(b1)
    assert sorted(new) == list(range(n0)) and [int(new[t]) for t in nodes] == list(range(1, 1 + len(nodes)))
    assert (n1, m1, c0, c1) == (n0, m0, 1, 1 + len(nodes))
    assert all(new[i] < m0 for i in range(m0)) and all(new[i] == i for i in range(m0, n0)) and new[0] == 0   # linear buses among themselves
    assert list(b1["type"][1:c1]) == ["PV"] * len(nodes) and list(b1["type"][c1:]) == list(b0["type"][c1:])
    keep = np.arange(n0) >= c1                              # loads stay with their IDs
    assert np.array_equal(b1["P"].to_numpy()[keep], b0["P"].to_numpy()[keep]) and np.array_equal(b1["Q"].to_numpy()[keep], b0["Q"].to_numpy()[keep])
    assert (b1["P"].to_numpy()[1:c1] == -120 / st.BASE_POWER).all() and (b1["Q"].to_numpy()[1:c1] == 0).all()
    A0 = _dense(hp.build_admittance_matrices(b0, l0, st.HARMONICS), n0)
    A1 = _dense(hp.build_admittance_matrices(b1, l1, st.HARMONICS), n0)
    P = A1[:, new[:, None], new[None, :]]                   # the placed matrices in the original numbering
    off = ~np.eye(n0, dtype=bool)
    assert np.array_equal(P[:, off], A0[:, off])
    for q in range(A0.shape[0]):
        d = np.zeros(n0, dtype=np.complex128)
        for j in range(n0):                                 # the row sums in the placed column order
            d = d + np.where(off[:, j], A1[q][:, j], 0)
        want = -d
        sh = b1["X_sh"].to_numpy(float)
        if st.HARMONICS[q] != 1:
            want = np.where(sh != 0, want + 1 / (1j * np.where(sh != 0, sh, 1.0) * st.HARMONICS[q]), want)
        assert np.array_equal(np.diag(A1[q]), want)
        assert np.abs(np.diag(P[q]) - np.diag(A0[q])).max() <= 4 * np.finfo(float).eps * np.abs(np.diag(A0[q])).max()


def test_place_refuses_the_slack_and_nonlinear_buses(tmp_path):
    from harmonic_power_flow_amd import synth
    fb, fl = synth.gen(pp.N_GEN, seed=0, outdir=str(tmp_path), zscale=pp.Z)
    for bad in ([0], [59], [89], [20, 20]):
        with pytest.raises(AssertionError):
            pp.place(fb, fl, bad)


def r_pq_of(new, k_placed, r_pq):
    """the PQ-plan role of the bus that has index k_placed in the placed feeder"""
    return r_pq.get(int(np.nonzero(new == k_placed)[0][0]))


def _plans(case, tmp_path):
    """roles of the case's feeder before and after the placement, and the placed plan's dump block"""
    (tmp_path / "pq").mkdir(exist_ok=True)
    fb0, fl0, _ = pp.write(case, tmp_path / "pq", placed=False)
    fb, fl, new = pp.write(case, tmp_path)
    return pp.roles(fb0, fl0, case.hmax), pp.roles(fb, fl, case.hmax), pp.dump(fb, fl, case.hmax), (fb, fl), new


@pytest.mark.parametrize("case", PLANNED, ids=IDS)
def test_role_facts_and_planner_rules(case, tmp_path, monkeypatch):
    monkeypatch.delenv("HPF_COMPRESS", raising=False)
    r_pq, r_pv, block, _, new = _plans(case, tmp_path)
    c = 1 + len(case.nodes)
    assert tuple(pp.fmt(r_pq[k]) for k in case.nodes) == case.pq
    assert tuple(pp.fmt(r_pv[1 + j]) for j in range(len(case.nodes))) == case.pv
    assert pp.census_of(block) == case.census
    rows = pp.dense_rows(block)
    for j, k in enumerate(case.nodes):                      # rule at plan_bordered_buses: a bus that is bordered as a PQ bus is a plain Gauss-Jordan bus as a PV bus
        if not isinstance(r_pq[k], str) and r_pq[k].kind == 2:
            assert rows[1 + j].kind == 0 and rows[1 + j].vector_only == 0
        if isinstance(r_pq[k], str):                        # a bus of the 2x2 algebra stays one
            assert r_pv[1 + j] == r_pq[k]
    for k, r in rows.items():
        assert not (r.kind == 2 and k < c), (k, r)          # no bordered bus among the PV buses
        assert not (r.vector_only != 0 and 0 <= r.par < c), (k, r)     # no lazy leaf, no vector-only bordered bus under a PV bus (or the slack)
        # no bus above a dense PV bus is eliminated before it: it is no pending child of a compress step and hangs under no contracted chain
        assert not (0 < k < c and (r.compress_role == 2 or r.via_chain != 0)), (k, r)
    # the placement moves nothing but the PV buses' neighbourhood: the dense buses are the same set under the relabelling, but for the
    # parent of a dense PV bus, which is a pass-through bus under a PQ bus and a dense bus of its own under a PV bus (the hub of the broom)
    (tmp_path / "pq2").mkdir()
    fb0, fl0, _ = pp.write(case, tmp_path / "pq2", placed=False)
    rows_pq = pp.dense_rows(pp.dump(fb0, fl0, case.hmax))
    was_pass = sorted(rows[k].par for k in rows if 0 < k < c and r_pq_of(new, rows[k].par, r_pq) == "pass")
    assert sorted([int(new[k]) for k in rows_pq] + was_pass) == sorted(rows)
    assert was_pass == ([rows[1].par] if (case.base, case.nodes) == ("broom", (44,)) else [])
    for j, k in enumerate(case.nodes):
        if not isinstance(r_pq[k], str) and rows_pq[k].via_chain:
            assert rows[rows[1 + j].par].kind == 0 and rows[1 + j].via_chain == 0
    if (case.base, case.nodes) == ("broom", (44,)):
        # the hub of the broom: as a PQ bus LZ_MAX of its 31 leaves are lazy, as a PV bus none; all 31 are constant-inverse leaves of their own
        kids = [r for r in rows.values() if r.par == 1]
        assert len(kids) == 31 and all(r.kind == 1 and r.vector_only == 0 for r in kids)
        kids_pq = [r for r in pp.dense_rows(pp.dump(fb0, fl0, case.hmax)).values() if r.par == 44]
        assert sum(r.vector_only != 0 for r in kids_pq) == shapes_host.LZ_MAX and len(kids_pq) == 31


def test_every_role_class_is_placed_at_every_block_class():
    """the table itself: the 11 role representatives at H_MAX 11, 27, 51 and 99, and every class of the 2x2 algebra and of the dense buses
    among the PV roles"""
    for hmax in (11, 27, 51, 99):
        got = {c.nodes[0]: c for c in pp.SINGLE if c.hmax == hmax}
        assert set(got) == set(pp.ROLE_NODES)
        assert {got[k].pv[0] for k in (1, 3, 8, 17, 2)} == {"lin leaf root", "lin leaf", "lin interior", "lin interior root", "pass"}
        dense = [got[k] for k in (51, 14, 5, 6, 56, 20)]
        assert all(c.pv[0].startswith("dense kind0") for c in dense)
        # (role 2, the pending child of a compress step, exists among PQ buses only: the planner gives it to no PV bus)
        assert {c.pq[0].split()[5] for c in dense} == {"role0", "role1", "role2"} and {c.pv[0].split()[5] for c in dense} == {"role0", "role1"}
        if hmax <= 51:                                      # (b = 100 has neither lazy leaves nor bordered buses)
            assert got[20].pq[0].startswith("dense kind2 lazy1") and all(c.pq[0] != c.pv[0] for c in dense)


@pytest.mark.parametrize("case", PLANNED, ids=IDS)
def test_dependencies_with_and_without_compress_steps(case, tmp_path, monkeypatch):
    """the invariants of test_tree_plan_host.py (through their run on the shapes, test_shapes_plan_host.py) on the placed feeder's trees"""
    import tree_plan
    fb, fl, _ = pp.write(case, tmp_path)
    real = tree_plan.plan
    rows = pp.dense_rows(pp.dump(fb, fl, case.hmax)).values()
    facts = types.SimpleNamespace(n=case.n, hmax=case.hmax, name=case.base, dense=len(rows), roles=sum(r.compress_role != 0 for r in rows),
                                  levels=max(r.height for r in rows) + 1)

    def use(_):
        monkeypatch.setattr(tree_plan, "plan", lambda nb, hmax, seed=0, max_scenarios=1, ties=0, lines_out=False, files=None:
                            real(0, hmax, max_scenarios=max_scenarios, lines_out=lines_out, files=(fb, fl)))
    shapes_host.test_dependencies_with_and_without_compress_steps(facts, use, monkeypatch)


@pytest.fixture(scope="module")
def wide_dir(tmp_path_factory):
    import wide_ne
    return wide_ne.write(str(tmp_path_factory.mktemp("wide_ne")), INPUTS)


@pytest.mark.parametrize("case", pp.CASES, ids=[c.id for c in pp.CASES])
def test_the_oracle_solves_every_case_in_every_scenario(case, tmp_path, wide_dir):
    """the reference's algorithm converges on the placed feeder in each of the GPU tests' three scenarios: err <= 1e-4 in under 50 harmonic
    and under 30 power-flow iterations (what _run(converge=True) asserts of the device)"""
    import hpf_oracle as o
    from harmonic_power_flow_amd import synth
    fb, fl, _ = pp.write(case, tmp_path)
    st = _hp().Settings(H_MAX=case.hmax)
    onet = o.init_network(fb, fl)
    assert onet.c == 1 + len(case.nodes)
    P0, Q0 = onet.P.copy(), onet.Q.copy()
    for s in range(S):
        sc_ = synth.scenario_scale(case.n, s)
        onet.P, onet.Q = P0 * sc_, Q0 * sc_
        r = o.hpf(onet, st.HARMONICS, case.coupled, wide_dir if case.hmax > 99 else INPUTS)
        print("\nPVPLACE oracle %-32s scenario %d n_iter_f %d n_iter_h %d err_h %.2e" % (case.id, s, r["n_iter_f"], r["n_iter_h"], r["err_h"]))
        assert r["err_h"] <= 1e-4 and r["n_iter_h"] < 50 and r["n_iter_f"] < 30


@pytest.mark.parametrize("hmax", [27, 51])
@pytest.mark.parametrize("node", [20, 6])
def test_the_oracle_solves_the_17_scenarios_of_the_switch_cases(node, hmax, tmp_path):
    """scenarios 3 .. 16 of the feeders the GPU tests run with a batch of 17 (0 .. 2 are in the test above)"""
    import hpf_oracle as o
    from harmonic_power_flow_amd import synth
    case = pp.case("gen", (node,), hmax)
    fb, fl, _ = pp.write(case, tmp_path)
    st = _hp().Settings(H_MAX=hmax)
    onet = o.init_network(fb, fl)
    P0, Q0 = onet.P.copy(), onet.Q.copy()
    worst = 0
    for s in range(S, 17):
        sc_ = synth.scenario_scale(case.n, s)
        onet.P, onet.Q = P0 * sc_, Q0 * sc_
        r = o.hpf(onet, st.HARMONICS, True, INPUTS)
        worst = max(worst, r["n_iter_h"])
        assert r["err_h"] <= 1e-4 and r["n_iter_h"] < 50 and r["n_iter_f"] < 30, (s, r["n_iter_h"], r["err_h"])
    print("\nPVPLACE oracle %-32s scenarios 3 .. 16: at most %d harmonic iterations" % (case.id, worst))
