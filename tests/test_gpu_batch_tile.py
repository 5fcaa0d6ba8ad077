"""Scenario tiles of the batched factor bodies (leaf_batch_body / sleaf_batch_body: 16 scenarios per workgroup, or 8 with 32 threads per
scenario where the group is no larger than HPF_BATCH_TILE8_MAX for the bordered buses, HPF_LEAF_TILE8_MAX for the lazy leaves) change which thread computes a row or a harmonic, not what it computes: the
Newton states, errors and iteration counts are bit for bit the same with both tiles -- at blocks of 12, 28 and 52 rows, with full and ragged
tiles (19 scenarios: 8 + 8 + 3 against 16 + 3; 40: five full tiles of 8 against 16 + 16 + 8; either count is one scenario group whatever
HPF_GROUPS says -- a group holds at least 32 --, so the last test runs 128 scenarios as four groups of 32), through hpf_iterate and through hpf_solve (scenarios that converge freeze and leave holes in the slot list), in the
fused level launches and in the standalone ones (HPF_FUSELEVEL=0).  hpf_tree_census[17] / [18] (the tile of the last factor launch with
bordered buses / with lazy leaves) show which path ran."""
import numpy as np
import pytest

from test_gpu_robustness import _feeder, _hp, _solve

pytestmark = pytest.mark.gpu

FEEDERS = [(600, 11, 0), (400, 27, 0), (300, 51, 2)]      # buses, H_MAX, seed: blocks of 12, 28 and 52 rows
FORCE8 = "4096"                                           # every group takes tiles of 8


def _iterate(hp, st, buses, Y, NE, S, iters=3):
    """`iters` Newton iterations of every scenario from the fundamental power-flow seed through hpf_iterate"""
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
        dm.iterate(iters)
        dm.sync()
        _, err = dm.mismatch(want_f=False)
        Vm, Va = dm.get_state()
        census = dm.tree_census()
    finally:
        dm.close()
    return dict(it=np.full(S, iters), err=err, Vm=Vm, Va=Va, census=census)


def _both_tiles(run, monkeypatch, extra=None):
    for k, v in (extra or {}).items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("HPF_BATCH_TILE8_MAX", "0")
    monkeypatch.setenv("HPF_LEAF_TILE8_MAX", "0")
    t16 = run()
    assert t16["census"]["batch_tile"] == 16 and t16["census"]["leaf_batch_tile"] == 16, t16["census"]
    monkeypatch.setenv("HPF_BATCH_TILE8_MAX", FORCE8)
    monkeypatch.setenv("HPF_LEAF_TILE8_MAX", FORCE8)
    t8 = run()
    assert t8["census"]["batch_tile"] == 8 and t8["census"]["leaf_batch_tile"] == 8, t8["census"]
    assert t8["census"]["bordered"] > 0 and t8["census"]["lazy_leaves"] > 0
    assert np.array_equal(t8["it"], t16["it"])
    assert np.array_equal(t8["Vm"], t16["Vm"]) and np.array_equal(t8["Va"], t16["Va"])
    assert np.array_equal(t8["err"], t16["err"])
    assert np.isfinite(t8["Vm"]).all() and np.isfinite(t8["err"]).all()
    return t8


@pytest.mark.parametrize("S,extra", [(19, None), (40, None), (19, {"HPF_GROUPS": "1"}), (40, {"HPF_GROUPS": "1"})])
@pytest.mark.parametrize("n,hmax,seed", FEEDERS)
def test_tile8_matches_tile16_through_solve(n, hmax, seed, S, extra, tmp_path, monkeypatch):
    hp = _hp()
    st, buses, Y, NE, _ = _feeder(hp, n, hmax, tmp_path, seed=seed)
    t8 = _both_tiles(lambda: _solve(hp, st, buses, Y, NE, S=S), monkeypatch, extra)
    assert (t8["err"] <= 1e-4).all()
    print("\nn=%d hmax=%d S=%d: iterations %s" % (n, hmax, S, sorted(set(t8["it"].tolist()))))


@pytest.mark.parametrize("S,extra", [(19, None), (40, None), (19, {"HPF_GROUPS": "1"}), (40, {"HPF_GROUPS": "1"})])
@pytest.mark.parametrize("n,hmax,seed", FEEDERS)
def test_tile8_matches_tile16_through_iterate(n, hmax, seed, S, extra, tmp_path, monkeypatch):
    hp = _hp()
    st, buses, Y, NE, _ = _feeder(hp, n, hmax, tmp_path, seed=seed)
    _both_tiles(lambda: _iterate(hp, st, buses, Y, NE, S), monkeypatch, extra)


@pytest.mark.parametrize("n,hmax,seed", FEEDERS)
def test_tile8_matches_tile16_in_the_standalone_launches(n, hmax, seed, tmp_path, monkeypatch):
    hp = _hp()
    st, buses, Y, NE, _ = _feeder(hp, n, hmax, tmp_path, seed=seed)
    t8 = _both_tiles(lambda: _solve(hp, st, buses, Y, NE, S=19, polish=1), monkeypatch, {"HPF_FUSELEVEL": "0", "HPF_GROUPS": "1"})
    assert t8["census"]["fused_levels"] == 0


def test_tile_follows_the_group_size(tmp_path, monkeypatch):
    """HPF_BATCH_TILE8_MAX is a bound on the scenario group, not on the batch: under a bound of 32, 128 scenarios in one group keep tiles of 16,
    in four groups of 32 (four streams side by side) their bordered buses take tiles of 8 -- with the same states; the leaves have their own bound"""
    hp = _hp()
    st, buses, Y, NE, _ = _feeder(hp, 300, 51, tmp_path, seed=2)
    monkeypatch.setenv("HPF_BATCH_TILE8_MAX", "32")
    monkeypatch.setenv("HPF_LEAF_TILE8_MAX", "0")
    monkeypatch.setenv("HPF_GROUPS", "1")
    one = _iterate(hp, st, buses, Y, NE, 128, iters=2)
    monkeypatch.setenv("HPF_GROUPS", "4")
    four = _iterate(hp, st, buses, Y, NE, 128, iters=2)
    assert one["census"]["batch_tile"] == 16 and four["census"]["batch_tile"] == 8
    assert one["census"]["leaf_batch_tile"] == 16 and four["census"]["leaf_batch_tile"] == 16
    assert np.array_equal(one["Vm"], four["Vm"]) and np.array_equal(one["Va"], four["Va"]) and np.array_equal(one["err"], four["err"])
