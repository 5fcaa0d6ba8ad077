"""Beyond the block tree's width limit (2 Hn <= 112): what solver="auto" and an explicit solver="block_tree" do for a radial feeder of 32 buses
and more with 57 harmonics.  "auto" solves it on the dense GPU path, as it does for a meshed feeder the bordered step refuses; the explicit
request fails with a message that names the limit (pinned without a GPU in tests/test_wide_ne_host.py too)."""
import numpy as np
import pytest

from conftest import INPUTS

pytestmark = pytest.mark.gpu

TOL_V = 1e-8
N_BUS, H_MAX = 40, 113
SEED = 6                 # synth.gen(40, seed): the oracle converges at H_MAX = 113 with the wide table for seeds 6 (21 iterations), 9, 10 and 14 of 0 .. 15


@pytest.fixture(scope="module")
def wide_dir(tmp_path_factory):
    import wide_ne
    return wide_ne.write(str(tmp_path_factory.mktemp("wide_ne")), INPUTS)


def test_auto_solves_57_harmonics_on_the_dense_path(wide_dir, tmp_path):
    import harmonic_power_flow_amd as hp
    import hpf_oracle as o
    from harmonic_power_flow_amd import synth
    fb, fl = synth.gen(N_BUS, seed=SEED, outdir=str(tmp_path))
    st = hp.Settings(H_MAX=H_MAX)
    assert len(st.HARMONICS) == 57
    res = hp.solve(fb, fl, coupled=True, settings=st, ne_dir=wide_dir)
    r = o.hpf(o.init_network(fb, fl), st.HARMONICS, True, wide_dir)
    assert r["err_h"] <= 1e-4 and r["n_iter_h"] < 50
    Ud = res["V"]["V_m"].to_numpy() * np.exp(1j * res["V"]["V_a"].to_numpy())
    dv = float(np.abs(Ud - r["Vm"] * np.exp(1j * r["Va"])).max())
    print("\nWIDE n=%d H_MAX=%d auto -> %s  n_iter_h %d (oracle %d)  err_h %.2e  max|dV| %.2e"
          % (N_BUS, H_MAX, res["details"]["solver"], res["n_iter_h"], r["n_iter_h"], res["err_h"], dv))
    assert res["details"]["solver"] == "dense" and res["converged"]
    assert dv < TOL_V


def test_explicit_block_tree_names_the_limit(wide_dir, tmp_path):
    import harmonic_power_flow_amd as hp
    from harmonic_power_flow_amd import synth
    fb, fl = synth.gen(N_BUS, seed=SEED, outdir=str(tmp_path))
    with pytest.raises(ValueError, match=r"2\*Hn <= 112"):
        hp.solve(fb, fl, coupled=True, settings=hp.Settings(H_MAX=H_MAX), ne_dir=wide_dir, solver="block_tree")
    # one harmonic less is inside the limit: "auto" and the explicit request both get a block-tree handle
    import test_gpu_step_accuracy as sa
    from harmonic_power_flow_amd import api
    net = sa._net(tmp_path, N_BUS, H_MAX - 2, seed=SEED, ne_dir=wide_dir)
    for solver in ("auto", "block_tree"):
        dm = api._device_model(net["buses"], net["Y"], net["NE"], True, net["st"].HARMONICS, solver=solver)
        try:
            assert dm.solver == "block_tree" and dm.Hn == 56
        finally:
            dm.close()
