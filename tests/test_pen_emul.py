"""Harmonic penetration without a GPU: the host emulation (tests/pen_emul.py: the functions of csrc/hpf_penetration.hpp in the kernels' order)
against numpy.linalg.solve on zscan_ref.dense_Y, its statistics against NumPy on the emulated V, and bit-identity of every output across chunkings.

Bound of the comparison of voltages, the one of tests/test_zscan_emul.py: for every (scenario, frequency point) the error, relative to
max_i |V_i|, is at most 2^-52 kappa_2(Y(h)) -- the forward-error scale of a backward-stable solve; derived, not tuned.  So that the bound hides
nothing, kappa_2 <= 1e7 is asserted at every point."""
import numpy as np
import pytest

import pen_emul as pe
import zscan_emul as ze

GRID = np.linspace(0.5, 50.5, 130)
KAPPA_MAX = 1e7
S = 5

_RUNS = {}


def _case(name):
    """-> model, y_extra, inj, I, (code, outputs) of the emulation with automatic chunks; computed once and shared (left unchanged)"""
    if name not in _RUNS:
        banks = {"syn12": {5: 0.002, 9: 0.02}, "syn40": {17: 0.01, 33: 0.004}}.get(name)
        model = ze.chain(9) if name == "chain9" else ze.star(9) if name == "star9" else ze.network(name)["model"]
        n = int(model["n"])
        yx = ze.capacitors(model, GRID, banks) if banks else None
        inj = np.arange(n // 2, n, dtype=np.int32)           # the upper half of the buses
        I = pe.currents(S, len(GRID), len(inj), seed=n)
        _RUNS[name] = (model, yx, inj, I, pe.penetration(model, GRID, I, inj, yx))
    return _RUNS[name]


CASES = ["chain9", "star9", "syn12", "syn40", "net1", "net2"]


@pytest.mark.parametrize("name", CASES)
def test_emulation_matches_the_dense_solve(name):
    model, yx, inj, I, (rc, out) = _case(name)
    assert rc == 0
    if name in ("net1", "net2"):
        assert len(ze.plan(model)[3]) == {"net1": 4, "net2": 1}[name]
    Vd, kappa = pe.dense(model, GRID, I, inj, yx)
    assert kappa.max() <= KAPPA_MAX, kappa.max()
    share = pe.bound_share(out["V"], Vd, kappa)
    print(name, "kappa max %.3g" % kappa.max(), "share of the bound used %.3g" % share.max())
    assert np.all(share <= 1.0)


@pytest.mark.parametrize("name", CASES)
def test_statistics_are_those_of_the_emulated_voltages(name):
    _, _, _, _, (rc, out) = _case(name)
    want = pe.stats_numpy(out["V"])
    for key, w in want.items():
        assert pe.same(out[key], w), (name, key)


@pytest.mark.parametrize("name", CASES)
def test_every_output_is_bit_identical_for_every_chunking(name):
    model, yx, inj, I, (rc, base) = _case(name)
    for chunk_f in (0, 17, 64):
        for chunk_s in (0, 2, 5):
            rc2, got = pe.penetration(model, GRID, I, inj, yx, chunk_f, chunk_s)
            assert rc2 == rc
            for key in pe.OUTPUTS:
                assert pe.same(got[key], base[key]), (name, chunk_f, chunk_s, key)
    rc3, stats_only = pe.penetration(model, GRID, I, inj, yx, 17, 2, full=False)
    assert stats_only["V"] is None and all(pe.same(stats_only[k], base[k]) for k in pe.OUTPUTS[1:])


def test_chunk_lengths():
    B = (256 << 20) // 16
    assert pe.chunks(130, 5, 0, 0, 100, 10) == (130, 5)                       # everything fits
    assert pe.chunks(130, 5, 17, 2, 100, 10) == (17, 2) and pe.chunks(13, 5, 17, 9, 100, 10) == (13, 5)      # forced: as given, clipped
    Fc, Sc = pe.chunks(25, 1024, 0, 0, 2000, 1350)                            # 1 000 buses, 350 injecting, statistics only
    assert Sc == 1024 and Fc == B // (2000 + 1024 * 1350) == 12
    Fc, Sc = pe.chunks(25, 65536, 0, 0, 2000, 2000)                           # one point with all scenarios does not fit
    assert Fc == 1 and Sc == (B - 2000) // 2000 // 64 * 64 and Fc * (2000 + Sc * 2000) <= B
    Fc, Sc = pe.chunks(4096, 64, 256, 0, 2000, 2000)                          # forced points: the scenarios that fit next to them
    assert Fc == 256 and Sc == (B // 256 - 2000) // 2000 and Fc * (2000 + Sc * 2000) <= B


def test_equal_scenarios_tie_to_the_smaller_index_and_zero_currents_give_zero():
    model = ze.network("net1")["model"]
    n = int(model["n"])
    inj = np.arange(n, dtype=np.int32)
    I = pe.currents(4, 7, n, seed=3)
    I[2] = I[0]                                               # scenario 2 repeats scenario 0
    I[1] = 0.0
    I[3] = 0.5 * I[0]
    rc, out = pe.penetration(model, GRID[:7], I, inj, None, 3, 2)             # the twins sit in different scenario chunks
    assert rc == 0
    assert np.all(out["varg"] == 0) and np.all(out["rss_arg"] == 0)
    assert np.all(out["V"][1] == 0) and np.all(out["rss"][1] == 0)
    assert pe.same(out["V"][2], out["V"][0])


def test_a_floating_network_is_reported_singular_with_the_outputs_written():
    model = ze.raw_model(1, [], xsh0=0.0)
    rc, out = pe.penetration(model, np.array([0.5, 1.0, 2.0]), np.ones((2, 3, 1), dtype=np.complex128), [0])
    assert rc == 3 and not np.isfinite(out["V"]).any() and np.all(out["varg"] == 0)
