"""Per-scenario source currents against the CPU oracle alone (no GPU), and the host-side argument checks of the feature.

The scenarios every source test shares (tests/sources_emul.py): syn100 x harmonics to 11, coupled; 24 scenarios; loads from synth.scenario_scale;
per nonlinear bus a in [0.875, 1.125] units in service and a time shift phi in [-0.075, 0.075] rad, seed 20260.  The ranges first asked for --
a in [0.5, 1.5], phi in [-0.3, 0.3] -- make the oracle's harmonic NR (the reference's polar update from its flat start + pf) diverge on all 24
coupled scenarios, half that width on 4 of 24 (radial; 5 of 24 with the two loop-closing lines); at a quarter it converges on every one, in
17 .. 28 iterations (radial) at thresh_h = 1e-9.  The unmodified oracle solves a scenario with per-bus sources because it looks Norton data up
per bus (net.component): every nonlinear bus gets a component of its own with (I_src of the bus, the Y_N of its device)."""
import numpy as np
import pytest

from conftest import INPUTS

import hpf_oracle as o
import sources_emul as se

THRESH = 1e-9


@pytest.fixture(scope="module")
def feeder(tmp_path_factory):
    from harmonic_power_flow_amd import synth, sweep
    fb, fl = synth.gen(100, seed=0, outdir=str(tmp_path_factory.mktemp("syn100")))
    H = o.harmonics_upto(11)
    case = se.oracle_network(fb, fl, H, True, INPUTS)
    n = case["net"].n
    a, phi = se.scale_shift(n - case["net"].m)
    I_src = sweep.source_currents(case["I_N_bus"], a, phi, H)
    scales = [synth.scenario_scale(n, s) for s in range(se.S_SCEN)]
    return dict(case=case, n=n, Hn=len(H), I_src=I_src, scales=scales)


def _thd_max(r, n, Hn):
    return float(o.get_THD(np.abs(r["Vm_raw"]), n, Hn)[:, 0].max())


def test_the_oracle_converges_on_every_source_scenario_and_the_sources_move_the_answer(feeder):
    fd = feeder
    with_src = [se.oracle_solve(fd["case"], fd["scales"][s], fd["I_src"][s], THRESH) for s in range(se.S_SCEN)]
    its = [r["n_iter_h"] for r in with_src]
    print("\nSOURCES oracle, syn100 H11 coupled, a in %s, phi in %s: iterations %s" % (se.A_RANGE, se.PHI_RANGE, its))
    assert all(r["err_h"] <= THRESH for r in with_src)                    # a condition: no scenario may be left out
    plain = [se.oracle_solve(fd["case"], fd["scales"][s], None, THRESH) for s in range(se.S_SCEN)]
    assert all(r["err_h"] <= THRESH for r in plain)
    t1 = max(_thd_max(r, fd["n"], fd["Hn"]) for r in with_src)
    t0 = max(_thd_max(r, fd["n"], fd["Hn"]) for r in plain)
    print("SOURCES oracle: largest THD over the sweep %.6f with sources, %.6f with a = 1, phi = 0" % (t1, t0))
    assert abs(t1 - t0) > 1e-3 * t0
    # a = 1, phi = 0 through the per-bus components IS the plain scenario (the device: bit for bit, tests/test_gpu_sources.py)
    ones = se.oracle_solve(fd["case"], fd["scales"][0], fd["case"]["I_N_bus"], THRESH)
    assert ones["n_iter_h"] == plain[0]["n_iter_h"] and np.array_equal(ones["Vm_raw"], plain[0]["Vm_raw"])


def test_entry_points_refuse_bad_arguments_before_any_device_call():
    """a NULL handle, NULL data, an unknown form, a NaN entry: HPF_E_ARG from every one of the calls, without a GPU (with a handle the same checks
    run first: tests/test_gpu_sources.py)"""
    import ctypes as C
    from harmonic_power_flow_amd import _lib
    lib = _lib.load()
    good = np.ones(12)
    bad = good.copy()
    bad[5] = np.nan
    orders = np.array([1, 3, 5], dtype=np.int32)
    dp, ip = good.ctypes.data_as(_lib.c_dbl_p), orders.ctypes.data_as(_lib.c_int_p)
    for fn in (lib.hpf_set_sources, lib.hpf_queue_sources):
        assert fn(None, 1, 0, dp, ip) == -1
        assert fn(None, 1, 0, None, ip) == -1
        assert fn(None, 1, 7, dp, ip) == -1
        assert fn(None, 1, 1, dp, None) == -1
        assert fn(None, 1, 0, bad.ctypes.data_as(_lib.c_dbl_p), ip) == -1
    assert lib.hpf_get_sources(None, dp) == -1 and lib.hpf_clear_sources(None) == -1


def test_the_python_layer_refuses_wrong_shapes_on_the_host():
    from harmonic_power_flow_amd import sweep
    n_scen, nnl, Hn = 5, 3, 4
    f, a = sweep.sources_argument({"scale": np.full((n_scen, nnl), 2.0)}, n_scen, nnl, Hn)
    assert f == "scale_shift" and a.shape == (n_scen, nnl, 2) and (a[:, :, 0] == 2.0).all() and (a[:, :, 1] == 0.0).all()
    f, a = sweep.sources_argument({"shift": np.full((n_scen, nnl), 0.1)}, n_scen, nnl, Hn)
    assert (a[:, :, 0] == 1.0).all() and (a[:, :, 1] == 0.1).all()
    f, a = sweep.sources_argument({"currents": np.ones((n_scen, nnl, Hn))}, n_scen, nnl, Hn)
    assert f == "currents" and a.dtype == np.complex128
    assert sweep.sources_argument(None, n_scen, nnl, Hn) is None
    for bad in ({"scale": np.ones((n_scen, nnl + 1))}, {"shift": np.ones(nnl)}, {"currents": np.ones((n_scen, nnl))},
                {"currents": np.ones((n_scen, nnl, Hn)), "scale": np.ones((n_scen, nnl))}, {"gain": 1.0}, {}, [1.0]):
        with pytest.raises(ValueError):
            sweep.sources_argument(bad, n_scen, nnl, Hn)
    # source_currents: shapes, and the unit scale / zero shift
    I_N = (np.arange(nnl * Hn).reshape(nnl, Hn) + 1) * (1 - 0.5j)
    out = sweep.source_currents(I_N, np.ones((n_scen, nnl)), np.zeros((n_scen, nnl)), [1, 3, 5, 7])
    assert out.shape == (n_scen, nnl, Hn) and np.array_equal(out[2], I_N)
    half_turn = sweep.source_currents(I_N, np.full(nnl, 2.0), np.full(nnl, np.pi), [1, 3, 5, 7])
    assert np.abs(half_turn + 2.0 * I_N).max() <= 6 * 2.0 ** -52 * 2.0 * np.abs(I_N).max() + 2.0 * np.abs(I_N).max() * 7 * 2.0 ** -52
