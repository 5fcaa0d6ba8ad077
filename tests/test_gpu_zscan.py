"""Impedance scan on the GPU (hpf_impedance_scan, the k_zscan_* kernels; run with -m gpu on an MI355X).

(a) EXACT: every product, sum and quotient of the scan is rounded on its own and every sum has one order, so Z, Zt, zpeak and fpeak must equal the
host emulation (tests/zscan_emul.py: the functions of csrc/hpf_zscan.hpp in the kernels' order) bit for bit -- for every grid length around the
wavefront size, every chunk length (chunk independence, the peak fold across chunks), every selection and both `full` settings.
(b) y_extra and shunts="norton" against the dense inverse of Yval + diag(Y_N) under the bound of tests/test_zscan_emul.py: the error relative to
max_i |Z_ii| of the point is at most 2^-52 kappa_2, with kappa_2 <= 1e7 asserted.
(c) The device memory count is the same before and after a scan, also one that returns an error after everything was allocated.
(d) One hp.impedance_scan call: the resonance a capacitor makes sits where the dense reference has it."""
import ctypes as C

import numpy as np
import pytest

from conftest import INPUTS

import zscan_emul as ze
import zscan_ref as ref

pytestmark = pytest.mark.gpu


def _api():
    from harmonic_power_flow_amd import api
    return api


def _grid(F):
    return np.array([2.5]) if F == 1 else np.linspace(0.5, 50.5, F)


def _shapes():
    syn12, syn40 = ze.network("syn12")["model"], ze.network("syn40")["model"]
    return {"n1": (ze.raw_model(1, []), {}), "n2": (ze.chain(2), {}), "chain9": (ze.chain(9), {}), "star9": (ze.star(9), {}),
            "syn12": (syn12, {5: 0.002, 9: 0.02}), "syn40": (syn40, {17: 0.01, 33: 0.004}), "net1": (ze.network("net1")["model"], {})}


def _selection(model, n_sel):
    """the root, a leaf and an inner bus (as far as the network has them)"""
    n = model["n"]
    parent, _, depth, _ = ze.plan(model)
    leaf = int(max(range(n), key=lambda i: (depth[i], i)))
    inner = int(parent[leaf]) if n > 1 else 0
    return [0, leaf, inner][:n_sel]


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


@pytest.mark.parametrize("shape", ["n1", "n2", "chain9", "star9", "syn12", "syn40", "net1"])
def test_device_equals_the_emulation_bit_for_bit(shape):
    api = _api()
    model, banks = _shapes()[shape]
    for F in (1, 63, 64, 65, 130):
        h = _grid(F)
        yx = ze.capacitors(model, h, banks) if banks else None
        for n_sel, full in ((0, True), (0, False), (1, True), (1, False), (3, True), (3, False)):
            sel = _selection(model, n_sel)
            want = ze.scan(model, h, yx, sel, 0, full)
            assert want[0] == 0
            for chunk in (0, 64, 17):
                got = api.impedance_scan_arrays(model, h, yx, sel, chunk, full)
                assert got[0] == 0, (shape, F, n_sel, chunk)
                for name, a, b in zip(("Z", "Zt", "zpeak", "fpeak"), got[1:], want[1:]):
                    assert _same(a, b), (shape, F, n_sel, full, chunk, name)


def test_equal_peaks_go_to_the_smaller_grid_index():
    api = _api()
    model = ze.network("net1")["model"]
    g = _grid(70)
    h = np.concatenate([g, g])                               # every value twice, 70 points apart: in another chunk for chunk = 64 and 17
    want = ze.scan(model, h)
    for chunk in (0, 64, 17):
        rc, Z, _, zpeak, fpeak = api.impedance_scan_arrays(model, h, chunk=chunk)
        assert rc == 0 and fpeak.max() < 70
        assert _same(fpeak, want[4]) and _same(zpeak, want[3]) and _same(Z, want[1])
        a = np.sqrt(Z.real * Z.real + Z.imag * Z.imag)
        assert np.array_equal(fpeak, a.argmax(axis=0)) and np.array_equal(zpeak, a.max(axis=0))


def test_y_extra_and_norton_shunts_against_the_dense_inverse():
    import harmonic_power_flow_amd as hp
    from harmonic_power_flow_amd import ingest
    st = hp.Settings()
    net = ze.network("syn12")
    buses, lines = net["buses"], net["lines"]
    n = len(buses)
    harmonics = list(st.HARMONICS)
    h = np.array(harmonics, dtype=float)
    NE = hp.import_Norton_Equivalents(buses, True, st, INPUTS)
    dev, Y_N, _, _ = ingest.norton_arrays(buses, NE, True, len(harmonics))
    Y = hp.build_admittance_matrices(buses, lines, harmonics)
    dense = np.stack([Y.dense(x) for x in harmonics])
    for q in range(len(harmonics)):
        for i in np.nonzero(dev >= 0)[0]:
            dense[q, i, i] += Y_N[dev[i], q, q]
    kappa = np.linalg.cond(dense, 2)
    assert kappa.max() <= 1e7, kappa.max()
    Zd = np.linalg.inv(dense)
    want = np.diagonal(Zd, axis1=1, axis2=2)
    scale = np.abs(want).max(axis=1)
    res = hp.impedance_scan(buses, lines, h, shunts="norton", transfer=[1, n], settings=st, ne_dir=INPUTS)
    err = np.abs(res.Z - want).max(axis=1) / scale
    print("norton: kappa max %.3g, share of the bound used %.3g" % (kappa.max(), (err / (ref.EPS * kappa)).max()))
    assert np.all(err <= ref.EPS * kappa)
    for s, j in enumerate((0, n - 1)):
        assert np.all(np.abs(res.Zt[:, s, :] - Zd[:, :, j]).max(axis=1) / scale <= ref.EPS * kappa)
    # the same shunts handed in as an array, plus a capacitor
    yx = np.zeros((len(h), n), dtype=np.complex128)
    for i in np.nonzero(dev >= 0)[0]:
        yx[:, i] = Y_N[dev[i], np.arange(len(h)), np.arange(len(h))]
    res2 = hp.impedance_scan(buses, lines, h, shunts=yx, transfer=[1, n])
    assert _same(res2.Z, res.Z) and _same(res2.Zt, res.Zt)
    res3 = hp.impedance_scan(buses, lines, h, shunts=yx, capacitors={int(buses["ID"].iloc[5]): 0.002})
    dense[:, 5, 5] += 1j * h * 0.002
    kappa3 = np.linalg.cond(dense, 2)
    assert kappa3.max() <= 1e7
    want3 = np.diagonal(np.linalg.inv(dense), axis1=1, axis2=2)
    assert np.all(np.abs(res3.Z - want3).max(axis=1) / np.abs(want3).max(axis=1) <= ref.EPS * kappa3)
    with pytest.raises(ValueError):
        hp.impedance_scan(buses, lines, np.array([3.0, 4.0]), shunts="norton", settings=st, ne_dir=INPUTS)


def _live():
    from harmonic_power_flow_amd import _lib
    blocks, nbytes = C.c_int64(), C.c_int64()
    assert _lib.load().hpf_debug_device_memory(C.byref(blocks), C.byref(nbytes)) == 0
    return blocks.value, nbytes.value


def test_a_scan_leaves_no_device_memory_behind():
    api = _api()
    model = ze.network("net1")["model"]
    before = _live()
    rc = api.impedance_scan_arrays(model, _grid(130), None, [0, 3], 17)[0]
    assert rc == 0 and _live() == before
    floating = ze.raw_model(1, [], xsh0=0.0)                  # Z = 1 / 0 at every point: the error comes after every allocation and launch
    rc, Z, _, zpeak, fpeak = api.impedance_scan_arrays(floating, np.array([0.5, 1.0, 2.0]))
    assert rc == 3 and not np.isfinite(zpeak[0]) and fpeak[0] == 0 and not np.isfinite(Z).any()
    assert _live() == before


def test_python_scan_finds_the_resonance_of_a_capacitor_bank():
    import harmonic_power_flow_amd as hp
    net = ze.network("syn40")
    buses, lines, model = net["buses"], net["lines"], net["model"]
    h = np.linspace(0.5, 50.5, 513)
    bus = 18                                                  # 1-based ID: position 17
    res = hp.impedance_scan(buses, lines, h, capacitors={bus: 0.01}, full=True)
    Zd, kappa, _ = ref.dense_scan(model, h, ze.capacitors(model, h, {bus - 1: 0.01}))
    want = np.abs(Zd[:, bus - 1, bus - 1])
    assert abs(int(res.peak_index[bus - 1]) - int(want.argmax())) <= 1
    assert abs(res.peak_h[bus - 1] - h[want.argmax()]) <= (h[1] - h[0]) * (1 + 1e-12)
    assert res.peak[bus - 1] == np.sqrt(res.Z.real ** 2 + res.Z.imag ** 2)[:, bus - 1].max()
    found = res.resonances(bus, prominence=0.5)
    assert int(res.peak_index[bus - 1]) in found.index or res.peak_index[bus - 1] in (0, len(h) - 1)
    peaks_only = hp.impedance_scan(buses, lines, h, capacitors={bus: 0.01}, full=False)
    assert peaks_only.Z is None and _same(peaks_only.peak, res.peak) and _same(peaks_only.peak_index, res.peak_index)
