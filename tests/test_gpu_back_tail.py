"""The back sweep's tail (k_back_tail: the bordered buses and constant-inverse leaves behind the Gauss-Jordan buses in one launch that walks
their families, HPF_BACKTAIL) changes the launch shape only: the Newton states and iteration counts are bit for bit those of one launch per
nesting order and one for the leaves (HPF_BACKTAIL=0) -- at blocks of 12, 28 and 52 rows, with a ragged scenario tile, through hpf_solve
(scenarios that converge freeze and leave holes in the slot list), behind the tree walk and behind the per-depth launches, and in the bordered
step of a meshed feeder, whose second pass is a back sweep alone.  hpf_tree_census[16] (back sweeps that took the tail) shows that it ran."""
import numpy as np
import pytest

from test_gpu_robustness import _add_ties, _feeder, _hp, _solve

pytestmark = pytest.mark.gpu

FEEDERS = [(600, 11, 0), (400, 27, 0), (300, 51, 2)]      # buses, H_MAX, seed: the feeders of test_back_tail_plan_host.py


def _same(a, b):
    assert np.array_equal(a["it"], b["it"])
    assert np.array_equal(a["Vm"], b["Vm"]) and np.array_equal(a["Va"], b["Va"])


def _on_off(run, monkeypatch, extra=None, tails=True):
    for k, v in (extra or {}).items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("HPF_BACKTAIL", "1")
    on = run()
    assert (on["census"]["back_tails"] > 0) == tails, on["census"]
    monkeypatch.setenv("HPF_BACKTAIL", "0")
    off = run()
    assert off["census"]["back_tails"] == 0, off["census"]
    _same(on, off)
    return on


@pytest.mark.parametrize("S,extra", [(19, None), (40, {"HPF_GROUPS": "1"}), (19, {"HPF_BACKWALK": "0", "HPF_FUSEBACK": "0"})])
@pytest.mark.parametrize("n,hmax,seed", FEEDERS)
def test_tail_matches_the_four_launches(n, hmax, seed, S, extra, tmp_path, monkeypatch):
    hp = _hp()
    st, buses, Y, NE, _ = _feeder(hp, n, hmax, tmp_path, seed=seed)
    on = _on_off(lambda: _solve(hp, st, buses, Y, NE, S=S, polish=1), monkeypatch, extra)
    assert on["census"]["nested_bordered"] > 0 and on["census"]["lazy_leaves"] > 0
    assert (on["err"] <= 1e-4).all()
    assert (on["census"]["back_walks"] > 0) == (hmax == 51 and extra != {"HPF_BACKWALK": "0", "HPF_FUSEBACK": "0"})


def test_tail_matches_the_four_launches_on_a_meshed_feeder(tmp_path, monkeypatch):
    hp = _hp()
    from conftest import INPUTS
    from harmonic_power_flow_amd import api, synth
    n, k, S = 300, 3, 3
    fb, fl = synth.gen(n, seed=2, outdir=str(tmp_path))
    _add_ties(fl, n, k)
    st = hp.Settings(H_MAX=51)
    buses, lines, m, nn, c = hp.init_network(fb, fl, settings=st)
    Y = hp.build_admittance_matrices(buses, lines, st.HARMONICS)
    NE = hp.import_Norton_Equivalents(buses, True, st, INPUTS)
    P0, Q0 = buses["P"].to_numpy(float), buses["Q"].to_numpy(float)
    scale = np.stack([synth.scenario_scale(n, s) for s in range(S)])

    def run():
        dm = api._device_model(buses, Y, NE, True, st.HARMONICS, solver="block_tree", max_scenarios=S)
        try:
            assert dm.tree_census()["ties"] == k
            dm.set_loads(P0 * scale, Q0 * scale)
            dm.set_state(None, None, n_scen=S)
            dm.fund_pf(1e-6, 30)
            it, err, _ = dm.solve(1e-4, 50)
            Vm, Va = dm.get_state()
            census = dm.tree_census()
        finally:
            dm.close()
        return dict(it=it, err=err, Vm=Vm, Va=Va, census=census)
    # (the walk, and the tail behind it, in every group size: by default groups below 16 scenarios take the fused per-depth launches)
    on = _on_off(run, monkeypatch, {"HPF_BACKWALK_MIN": "1", "HPF_BACKWALK_MAX": "4096"})
    assert (on["err"] <= 1e-4).all()


def test_tail_stays_off_without_leaf_batching(tmp_path, monkeypatch):
    hp = _hp()
    st, buses, Y, NE, _ = _feeder(hp, 300, 51, tmp_path, seed=2)
    _on_off(lambda: _solve(hp, st, buses, Y, NE, S=19, polish=1), monkeypatch, {"HPF_LEAFBATCH": "0"}, tails=False)
