"""The back sweep's tree walk (k_back_walk: two launches per scenario group instead of one per depth, HPF_BACKWALK) changes the launch
shape only: the Newton states and iteration counts are bit for bit those of the per-depth launches (HPF_BACKWALK=0), fused with the
batched workgroups or not (HPF_FUSEBACK=0) -- on the headline feeder at 32 and 128 scenarios (hpf_solve: scenarios that converge freeze
and leave the active list), a meshed feeder (bordered step), without compress steps, and at blocks of 12 / 28 where the walk stays off.
HPF_BACKWALK_MIN / _MAX open the walk to every group size here, and hpf_tree_census[15] (back sweeps that walked) shows that it ran."""
import numpy as np
import pytest

from test_gpu_robustness import _add_ties, _feeder, _hp, _solve

pytestmark = pytest.mark.gpu

VARIANTS = ({"HPF_BACKWALK": "0"}, {"HPF_BACKWALK": "0", "HPF_FUSEBACK": "0"})


def _inputs():
    from conftest import INPUTS
    return INPUTS


def _same(a, b):
    assert np.array_equal(a["it"], b["it"])
    assert np.array_equal(a["Vm"], b["Vm"]) and np.array_equal(a["Va"], b["Va"])


def _variants(run, monkeypatch, extra=None, walks=True):
    monkeypatch.setenv("HPF_BACKWALK_MIN", "1")         # the walk in every group it can take (default: groups of 16 - 256)
    monkeypatch.setenv("HPF_BACKWALK_MAX", "4096")
    for k, v in (extra or {}).items():
        monkeypatch.setenv(k, v)
    base = run()
    assert (base["census"]["back_walks"] > 0) == walks, base["census"]
    for env in VARIANTS:
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            var = run()
            assert var["census"]["back_walks"] == 0
            _same(var, base)
    return base


@pytest.mark.parametrize("S", [1, 32, 128])
def test_walk_matches_depth_launches_on_the_headline_feeder(S, tmp_path, monkeypatch):
    hp = _hp()
    st, buses, Y, NE, _ = _feeder(hp, 1000, 51, tmp_path, seed=0)
    base = _variants(lambda: _solve(hp, st, buses, Y, NE, S=S, polish=1), monkeypatch)
    assert (base["err"] <= 1e-4).all()
    assert S == 1 or len(set(base["it"].tolist())) > 1            # scenarios froze at different iterations


@pytest.mark.parametrize("extra", [{"HPF_COMPRESS": "0"}, {"HPF_GROUPS": "1"}])
def test_walk_matches_depth_launches_on_other_trees(extra, tmp_path, monkeypatch):
    hp = _hp()
    st, buses, Y, NE, _ = _feeder(hp, 600, 51, tmp_path, seed=3)
    _variants(lambda: _solve(hp, st, buses, Y, NE, S=40, polish=1), monkeypatch, extra)


def test_walk_matches_depth_launches_on_a_meshed_feeder(tmp_path, monkeypatch):
    hp = _hp()
    from harmonic_power_flow_amd import api, synth
    n, k, S = 300, 4, 3
    fb, fl = synth.gen(n, seed=4, outdir=str(tmp_path))
    _add_ties(fl, n, k)
    st = hp.Settings(H_MAX=51)
    buses, lines, m, nn, c = hp.init_network(fb, fl, settings=st)
    Y = hp.build_admittance_matrices(buses, lines, st.HARMONICS)
    NE = hp.import_Norton_Equivalents(buses, True, st, _inputs())
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
    base = _variants(run, monkeypatch)
    assert (base["err"] <= 1e-4).all()


@pytest.mark.parametrize("hmax", [11, 27])
def test_walk_stays_off_for_other_block_sizes(hmax, tmp_path, monkeypatch):
    hp = _hp()
    st, buses, Y, NE, _ = _feeder(hp, 300, hmax, tmp_path, seed=1)
    _variants(lambda: _solve(hp, st, buses, Y, NE, S=9, polish=1), monkeypatch, walks=False)
