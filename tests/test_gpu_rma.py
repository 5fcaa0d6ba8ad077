"""Resonance mode analysis on the GPU (hpf_resonance_modes, the k_rma_* kernels; run with -m gpu on an MI355X).

(a) EXACT: every product, sum and quotient is rounded on its own, every sum has one order and every maximum a total order, so all five outputs
must equal the host emulation (tests/rma_emul.py: the functions of csrc/hpf_resonance.hpp in the kernels' order) byte for byte -- for grid
lengths around the wavefront size, one and several steps, automatic and forced chunks, with pf and without, bus counts on both sides of the
32-bus tile of the sums (chain33, chain65), ties (net1) and degenerate modes (star9).
(b) syn12 with its banks and net1 at 64 steps against numpy.linalg.eig of the dense Y under the two bounds of tests/test_rma_emul.py.
(c) Physics: a 0.1 p.u. capacitor bank at bus 18 of syn40 makes one resonance near h = 16.7; the critical mode peaks at the grid point where
the largest |Z_ii| of hpf_impedance_scan peaks, bus 18 takes the largest part in it, and at the peak its modal share pf_18 / lambda is Z_18,18.
(d) The device memory count is the same before and after a call, also one that returns HPF_E_SINGULAR."""
import ctypes as C

import numpy as np
import pytest

import rma_emul as rm
import zscan_emul as ze

pytestmark = pytest.mark.gpu


def _api():
    from harmonic_power_flow_amd import api
    return api


def _grid(F):
    return np.array([2.5]) if F == 1 else np.linspace(0.5, 50.5, F)


@pytest.mark.parametrize("name", ["n1", "n2", "chain9", "star9", "chain33", "chain65", "syn12", "syn40", "net1"])
def test_device_equals_the_emulation_byte_for_byte(name):
    api = _api()
    model, banks = rm.shape(name)
    for F in (1, 63, 64, 65, 130):
        h = _grid(F)
        yx = rm.y_extra(model, h, banks)
        for iters in (1, 5):
            rc, want = rm.modes(model, h, yx, iters)
            assert rc == 0
            for chunk in (0, 64, 17):
                for full in (True, False):
                    got = api.resonance_modes_arrays(model, h, yx, iters, chunk, full)
                    assert got[0] == 0, (name, F, iters, chunk, full)
                    assert full or got[5] is None
                    for key, arr in zip(rm.OUTPUTS[:5 if full else 4], got[1:]):
                        assert rm.same(arr, want[key]), (name, F, iters, chunk, full, key)


@pytest.mark.parametrize("name", ["syn12", "net1"])
def test_device_against_the_dense_eigenpair(name):
    api = _api()
    model, banks = rm.shape(name)
    d = rm.dense(name)
    assert np.all(d["gap"] <= 0.5)
    rc, lam, zm, res, top, pf = api.resonance_modes_arrays(model, rm.GRID, rm.y_extra(model, rm.GRID, banks), 64)
    assert rc == 0
    s_lam, s_pf = rm.bound_shares(dict(lam=lam, pf=pf), d)
    print(name, "share of the eigenvalue bound used %.3g, of the participation bound %.3g; max res %.3g" % (s_lam.max(), s_pf.max(), res.max()))
    assert np.all(s_lam <= 1.0) and np.all(s_pf <= 1.0)
    assert np.all(res <= 1e-12)
    assert np.all(np.abs(pf.sum(axis=1) - 1.0) <= int(model["n"]) * 2.0 ** -50)


def test_a_capacitor_bank_makes_one_mode_and_its_bus_takes_the_largest_part():
    import harmonic_power_flow_amd as hp
    net = ze.network("syn40")
    h = np.linspace(0.5, 50.5, 513)
    r = hp.resonance_modes(net["buses"], net["lines"], h, capacitors={18: 0.1}, iters=32)
    scan = hp.impedance_scan(net["buses"], net["lines"], h, capacitors={18: 0.1})
    table = r.modes()
    print(table.to_string())
    near = [f for f in table.index if abs(f - 166) <= 1]
    assert len(near) == 1 and int(table.loc[near[0], "top"]) == 18
    f = near[0]
    assert r.converged()[f] and r.top[f] == 18
    assert abs(int(np.abs(scan.Z).max(axis=1).argmax()) - 166) <= 1
    p = r.bus_ids.index(18)
    ratio = abs(r.pf[f, p] / r.lam[f]) / abs(scan.Z[f, p])
    print("index %d, h = %.4f, zm = %.4g, |pf_18 mu| / |Z_18,18| = %.4f" % (f, h[f], r.zm[f], ratio))
    assert abs(ratio - 1.0) <= 0.02
    peaks_only = hp.resonance_modes(net["buses"], net["lines"], h, capacitors={18: 0.1}, iters=32, full=False)
    assert peaks_only.pf is None and rm.same(peaks_only.zm, r.zm) and np.array_equal(peaks_only.top, r.top)
    with pytest.raises(ValueError):
        peaks_only.modes()


def _live():
    from harmonic_power_flow_amd import _lib
    blocks, nbytes = C.c_int64(), C.c_int64()
    assert _lib.load().hpf_debug_device_memory(C.byref(blocks), C.byref(nbytes)) == 0
    return blocks.value, nbytes.value


def test_a_call_leaves_no_device_memory_behind():
    api = _api()
    model, _ = rm.shape("net1")
    before = _live()
    assert api.resonance_modes_arrays(model, _grid(65), None, 5, 17)[0] == 0 and _live() == before
    n1, _ = rm.shape("n1")                                    # xsh only: Y = 0 at h = 1; the error comes after every allocation and launch
    h = np.array([0.5, 1.0, 2.0])
    rc, lam, zm, res, top, pf = api.resonance_modes_arrays(n1, h, None, 3)
    want = rm.modes(n1, h, None, 3)
    assert rc == 3 and want[0] == 3 and not np.isfinite(zm[1]) and np.isfinite(zm[[0, 2]]).all()
    for key, arr in zip(rm.OUTPUTS, (lam, zm, res, top, pf)):   # (the bits of a NaN are the machine's: the finite points and the pattern)
        ok = np.isfinite(want[1][key])
        assert np.array_equal(np.isfinite(arr), ok) and rm.same(arr[ok], want[1][key][ok]), key
    assert _live() == before
