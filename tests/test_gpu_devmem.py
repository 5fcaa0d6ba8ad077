"""Ownership of device memory (csrc/hpf_devmem.hpp, hpf_debug_device_memory, DESIGN.md "Memory ownership"; run with -m gpu on an MI355X): every block
a handle allocates goes back when its group ends or the handle closes.

The figures are the library's own count of live blocks and bytes, not the device's free memory: they do not see other processes, so every
assertion is exact.  They are process-wide, so the test works with differences from the count it reads after a gc.collect().

Shapes, the smallest that reach every group of buffers: a 40-bus synthetic radial feeder at harmonics to 11 (blocks of 12) with 4 scenario slots on
the block tree (tree scratch, repeat buffers, the queue's fast path: 12 scenarios through the 4 slots); the same feeder with 3 loop-closing lines
(border and selected-inversion buffers, the queue in waves); net2 of the golden inputs on the dense solver (d_J and pivots).  The partial-failure
paths of an allocation need no GPU: tests/test_devmem_host.py."""
import gc
import os

import numpy as np
import pytest

from conftest import INPUTS

pytestmark = pytest.mark.gpu
N_BUS, SLOTS, N_QUEUE, CYCLES = 40, 4, 12, 3


def _net(kind, outdir):
    import harmonic_power_flow_amd as hp
    from harmonic_power_flow_amd import synth
    st = hp.Settings(H_MAX=11)
    if kind == "dense":
        fb, fl = os.path.join(INPUTS, "net2_buses.csv"), os.path.join(INPUTS, "net2_lines.csv")
    else:
        fb, fl = synth.gen(N_BUS, seed=0, outdir=str(outdir))
        if kind == "meshed":
            synth.add_ties(fl, N_BUS, 3)
    buses, lines, m, n, c = hp.init_network(fb, fl, settings=st)
    scale = np.stack([synth.scenario_scale(n, s) for s in range(N_QUEUE)])
    rng = np.random.default_rng(0)
    ab = np.stack([1.0 + 0.05 * rng.uniform(-1, 1, (N_QUEUE, n - m)), 0.02 * rng.uniform(-1, 1, (N_QUEUE, n - m))], axis=2)
    return dict(st=st, buses=buses, Y=hp.build_admittance_matrices(buses, lines, st.HARMONICS), NE=hp.import_Norton_Equivalents(buses, True, st, INPUTS),
                solver="dense" if kind == "dense" else "block_tree", P=buses["P"].to_numpy(float) * scale, Q=buses["Q"].to_numpy(float) * scale, ab=ab)


@pytest.fixture(scope="module", params=["radial", "meshed", "dense"])
def net(request, tmp_path_factory):
    return _net(request.param, tmp_path_factory.mktemp("devmem_" + request.param))


def _pair(mem, name, begin, end):
    """begin() allocates, end() gives exactly that back"""
    before = mem()
    begin()
    during = mem()
    end()
    after = mem()
    print("  %-14s blocks %+d  bytes %+d  -> %+d / %+d after the pair" % (name, during[0] - before[0], during[1] - before[1], after[0] - before[0],
                                                                        after[1] - before[1]))
    assert during[0] > before[0] and during[1] > before[1], name
    assert after == before, name


def test_every_block_goes_back(net):
    from harmonic_power_flow_amd import api
    from harmonic_power_flow_amd.device import device_memory as mem
    for cycle in range(CYCLES):
        gc.collect()
        base = mem()
        dm = api._device_model(net["buses"], net["Y"], net["NE"], True, net["st"].HARMONICS, solver=net["solver"], max_scenarios=SLOTS)
        try:
            created = mem()
            print("%s cycle %d: create blocks %+d  bytes %+d" % (net["solver"], cycle, created[0] - base[0], created[1] - base[1]))
            assert created[0] > base[0] and created[1] > base[1]
            dm.set_option("keep_previous_state", 1)
            dm.set_option("step_residual_check", 1)
            dm.timing(True)
            dm.set_loads(net["P"][:SLOTS], net["Q"][:SLOTS])
            dm.set_state(None, None, n_scen=SLOTS)
            dm.fund_pf(1e-6, 30)
            dm.solve(1e-6, 20)
            dm.jacobian_csr(0)
            dm.branch_flows()                              # (builds the branch table, which stays: the branch statistics below find it in place)
            Vm, Va = dm.get_state()
            _pair(mem, "distortion", dm.distortion_begin, dm.distortion_end)
            _pair(mem, "branch_stats", dm.branch_stats_begin, dm.branch_stats_end)
            _pair(mem, "start", lambda: dm.set_start(Vm[0], Va[0]), dm.clear_start)
            _pair(mem, "sources", lambda: dm.set_sources(net["ab"][:SLOTS], "scale_shift"), dm.clear_sources)
            dm.queue_sources(net["ab"], "scale_shift")
            rec = dm.solve_queue(net["P"], net["Q"], thresh=1e-6, max_iter=20)
            assert len(rec) == N_QUEUE
            used = mem()
            assert used[0] >= created[0] and used[1] >= created[1]
        finally:
            dm.close()
        left = mem()
        print("%s cycle %d: after close blocks %+d  bytes %+d" % (net["solver"], cycle, left[0] - base[0], left[1] - base[1]))
        assert left == base
