"""The 64-harmonic Norton table of tests/wide_ne.py without a GPU: its first 50 harmonics are the committed table bit for bit, the oracle
converges on the widest block-tree case the GPU suite runs with it (H_MAX = 111, b = 112, the generator seed recorded in
test_gpu_step_accuracy.WIDTH_SEED), and the block-tree planner's width limit sits where the GPU tests assume it: 2 Hn <= 112."""
import ctypes as C
import os

import numpy as np
import pytest

import wide_ne
from conftest import INPUTS


@pytest.fixture(scope="module")
def wide_dir(tmp_path_factory):
    return wide_ne.write(str(tmp_path_factory.mktemp("wide_ne")), INPUTS)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def test_first_50_harmonics_are_the_committed_table_bit_for_bit(wide_dir):
    from harmonic_power_flow_amd import ingest
    K, HN = wide_ne.K, wide_ne.HN
    f0, Y0, I0, Yu0, Iu0 = ingest.read_Norton_file(os.path.join(INPUTS, "smps_NE.csv"))
    f1, Y1, I1, Yu1, Iu1 = ingest.read_Norton_file(os.path.join(wide_dir, "smps_NE.csv"))
    assert len(f0) == K and f1[:K] == f0 and f1 == [50 * (2 * k + 1) for k in range(HN)] and f1[-1] == 6350
    assert Y1.shape == (HN, HN) and I1.shape == Yu1.shape == Iu1.shape == (HN,)
    assert np.array_equal(_bits(Y1[:K, :K]), _bits(Y0))
    for a, b in ((I1, I0), (Yu1, Yu0), (Iu1, Iu0)):
        assert np.array_equal(_bits(a[:K]), _bits(b))
    # the rule, entry by entry, for the added rows and columns
    for i, j in ((50, 0), (0, 50), (63, 63), (57, 21), (13, 60)):
        assert Y1[i, j] == Y0[wide_ne.src(i), wide_ne.src(j)] * wide_ne.bump(i, j)
    assert I1[63] == I0[49] * 0.8 and Iu1[50] == Iu0[36] * 0.8 and Yu1[55] == Yu0[41] * wide_ne.bump(55, 0)
    assert sorted({round(wide_ne.bump(i, j), 12) for i in range(HN) for j in range(HN)}) == [0.96, 0.98, 1.0, 1.02, 1.04]
    # both ingest paths (the package's and the oracle's) select the same numbers from it
    import hpf_oracle as o
    h = o.harmonics_upto(127)
    I_o, Y_o = o.import_norton(os.path.join(wide_dir, "smps_NE.csv"), h, True)
    assert np.array_equal(Y_o, Y1 / o.base_admittance) and np.array_equal(I_o, I1 / o.base_current)


def test_oracle_converges_on_the_widest_block_tree_case(wide_dir, tmp_path):
    """H_MAX = 111 (b = 112), synth.gen(90, WIDTH_SEED[56]), coupled, every synth.scenario_scale scenario of the GPU case
    (seeds 0 and 2 of this width diverge in the oracle too: test_gpu_step_accuracy.WIDTH_SEED)."""
    import hpf_oracle as o
    from harmonic_power_flow_amd import synth
    from test_gpu_step_accuracy import N_BUS, S, WIDTH_SEED
    fb, fl = synth.gen(N_BUS, seed=WIDTH_SEED[56], outdir=str(tmp_path))
    h = o.harmonics_upto(111)
    net = o.init_network(fb, fl)
    rowptr, col, Yval = o.build_admittance_matrices(net, h)
    NE = o.import_Norton_Equivalents(net, h, True, wide_dir)
    P0, Q0 = net.P.copy(), net.Q.copy()
    for s in range(S):
        sc_ = synth.scenario_scale(net.n, s)
        net.P, net.Q = P0 * sc_, Q0 * sc_
        Vm, Va, _, _ = o.pf(net, rowptr, col, Yval)
        r = o.hpf_from_model(o.Model(net, h, rowptr, col, Yval, NE, True), Vm, Va)
        assert r["err_h"] <= 1e-4 and r["n_iter_h"] < 50, (s, r["n_iter_h"], r["err_h"])


def _plan_rc(fb, fl, hmax, ne_dir, out):
    """hpf_tree_plan (host only) of the model as api._device_model would describe it -> return code"""
    import harmonic_power_flow_amd as hp
    from harmonic_power_flow_amd import _lib, ingest
    st = hp.Settings(H_MAX=hmax)
    buses, lines, m, n, c = hp.init_network(fb, fl, settings=st)
    Y = hp.build_admittance_matrices(buses, lines, st.HARMONICS)
    NE = hp.import_Norton_Equivalents(buses, True, st, ne_dir)
    Hn = len(st.HARMONICS)
    keep = [np.ascontiguousarray(Y.rowptr, dtype=np.int32), np.ascontiguousarray(Y.col, dtype=np.int32),
            np.ascontiguousarray(Y.Yval, dtype=np.complex128)]
    dev, Y_N, I_N, n_dev = ingest.norton_arrays(buses, NE, True, Hn)
    keep += [np.ascontiguousarray(dev, dtype=np.int32), np.ascontiguousarray(Y_N), np.ascontiguousarray(I_N)]
    d = _lib.hpf_desc()
    d.n, d.m, d.c, d.Hn, d.nnz = n, m, c, Hn, len(keep[1])
    d.n_dev, d.coupled, d.solver, d.device, d.max_scenarios = int(n_dev), 1, _lib.SOLVER_BLOCK_TREE, 0, 1
    d.rowptr, d.col = keep[0].ctypes.data_as(_lib.c_int_p), keep[1].ctypes.data_as(_lib.c_int_p)
    d.Yval = keep[2].view(np.float64).ctypes.data_as(_lib.c_dbl_p)
    d.dev_of_bus = keep[3].ctypes.data_as(_lib.c_int_p)
    d.Y_N = keep[4].view(np.float64).ctypes.data_as(_lib.c_dbl_p)
    d.I_N = keep[5].view(np.float64).ctypes.data_as(_lib.c_dbl_p)
    return _lib.load().hpf_tree_plan(C.byref(d), os.path.join(out, "plan_H%d.txt" % hmax).encode())


def test_block_tree_plans_at_56_harmonics_and_refuses_57(wide_dir, tmp_path):
    """2 Hn <= 112 (tree_build_into): a radial model plans at Hn = 56 and is refused with HPF_E_ARG at Hn = 57 -- the line on which
    DeviceModel's solver="auto" turns to the dense path (device.BLOCK_TREE_MAX_B)."""
    from harmonic_power_flow_amd import device, synth
    fb, fl = synth.gen(40, seed=0, outdir=str(tmp_path))
    assert device.BLOCK_TREE_MAX_B == 112
    assert _plan_rc(fb, fl, 111, wide_dir, str(tmp_path)) == 0
    assert os.path.getsize(os.path.join(str(tmp_path), "plan_H111.txt")) > 0
    assert _plan_rc(fb, fl, 113, wide_dir, str(tmp_path)) == -1                  # HPF_E_ARG
    assert not os.path.exists(os.path.join(str(tmp_path), "plan_H113.txt"))


def test_explicit_block_tree_beyond_the_limit_is_refused_before_any_device_call(wide_dir, tmp_path):
    """DeviceModel(solver="block_tree") at Hn = 57: a ValueError that names the limit, raised before hpf_create (so it needs no GPU); with
    solver="auto" the same model goes to the dense path -- run on the device in tests/test_gpu_wide_limit.py."""
    import harmonic_power_flow_amd as hp
    from harmonic_power_flow_amd import api, synth
    fb, fl = synth.gen(40, seed=0, outdir=str(tmp_path))
    st = hp.Settings(H_MAX=113)
    buses, lines, m, n, c = hp.init_network(fb, fl, settings=st)
    Y = hp.build_admittance_matrices(buses, lines, st.HARMONICS)
    NE = hp.import_Norton_Equivalents(buses, True, st, wide_dir)
    with pytest.raises(ValueError, match=r"2\*Hn = 114 rows \(57 harmonics\); the block tree takes 2\*Hn <= 112"):
        api._device_model(buses, Y, NE, True, st.HARMONICS, solver="block_tree")
    # "auto" is refused the same way only where the dense Jacobians would not fit either
    with pytest.raises(ValueError, match=r"2\*Hn <= 112, and the dense path would need"):
        api._device_model(buses, Y, NE, True, st.HARMONICS, solver="auto", max_scenarios=2000)
