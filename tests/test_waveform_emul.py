"""Voltage waveforms and waveform statistics without a GPU: the functions of csrc/hpf_waveform.hpp executed serially on the host in the kernel's
order (tests/waveform_emul.py) against the NumPy restatement tests/waveform_ref.py; the definition itself (tie rule, pure sine, the slack bound
of the sampled peak); the host side (sweep.WaveformStats) and the argument checks of the entry points that need no device.

On the host sqrt and / are correctly rounded on both sides, both sides round every real product, difference and sum on its own in the same order and
read the same table (hpf_waveform_table), so samples, peak, kpeak, crest and slack must be EQUAL."""
import os

import numpy as np
import pytest

import distortion_emul as de
import waveform_emul as we
import waveform_ref as ref

from harmonic_power_flow_amd import _lib, sweep

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden(name, S=3):
    """the golden's final voltages and S - 1 perturbed copies (magnitudes and, strongly, angles) -> harmonics, n, Hn, U [S][n][Hn]"""
    g = np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=True)
    harmonics = [int(h) for h in g["harmonics"]]
    Hn = len(harmonics)
    Vm0, Va0 = g["V_final"][:, 0].astype(np.float64), g["V_final"][:, 1].astype(np.float64)
    n = len(Vm0) // Hn
    k = np.arange(len(Vm0))
    Vm = np.stack([Vm0 * (1.0 + 0.03 * np.sin(0.7 * s + 0.37 * k)) for s in range(S)])
    Va = np.stack([Va0 + 0.4 * s * np.cos(0.3 * s + 0.11 * k) for s in range(S)])
    return harmonics, n, Hn, ref.rect(Vm, Va, n, Hn)


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def test_the_three_tables_agree():
    for T in (64, 256, 1024, 4096):
        ct, st = ref.lib_table(T)
        et = we.table(T)
        assert _same(ct, et[0]) and _same(st, et[1])
        oc, os_ = ref.own_table(T)
        assert np.abs(ct - oc).max() <= 2.0 ** -52 and np.abs(st - os_).max() <= 2.0 ** -52
        for j, (c, s) in zip((0, T // 4, T // 2, 3 * T // 4), ((1, 0), (0, 1), (-1, 0), (0, -1))):
            assert ct[j] == c and st[j] == s


@pytest.mark.parametrize("name", ["net1_H51_c", "lin4_H11_c"])
@pytest.mark.parametrize("T", [64, 256, 4096])
@pytest.mark.parametrize("orders", ["odd", "all"])
def test_emulator_equals_numpy_bit_for_bit(name, T, orders):
    harmonics, n, Hn, U = golden(name)
    h = harmonics if orders == "odd" else list(range(1, Hn + 1))
    ct, st = ref.lib_table(T)
    sel = [0, n - 1, n // 2, 0]
    got = we.waveform(U, h, T, ct, st, sel)
    want = ref.waveform(U, h, T, ct, st)
    assert _same(got["v"], want["v"][:, sel])
    for k in ("peak", "kpeak", "crest", "slack"):
        assert _same(got[k], want[k]), k
    assert np.isfinite(want["peak"]).all() and (want["peak"] > 0).all() and (want["slack"] > 0).all()
    assert _same(we.rms(U[1, n - 1]), want["rms"][1, n - 1])
    if orders == "odd":
        assert (want["crest"] > 1.4).all()                          # (phases and harmonics only raise it measurably on these feeders)
        # odd orders only: half-wave symmetry v[k + T/2] = -v[k] up to the table's last bit -- the peak is reported in the first occurrence
        assert len(set(want["kpeak"].ravel().tolist())) > 1


def test_ties_go_to_the_smallest_sample():
    """Va = 0 and a table made symmetric (ct[T - j] = ct[j]): v[T - k] = v[k] bit for bit, so every peak away from k = 0 and T / 2 is a tie of two
    samples, and the smaller one must be reported -- by the lanes' own walk and by the butterfly alike."""
    harmonics, n, Hn, U = golden("net1_H51_c", 1)
    sign = np.where(np.arange(Hn) % 3 == 1, -1.0, 1.0)
    U = (np.abs(U) * sign * (1.0 + 0.2 * np.cos(np.arange(n))[:, None] * np.arange(Hn))).astype(np.complex128)
    for T in (64, 1024):
        ct, st = ref.lib_table(T)
        j = np.arange(T)
        ct = ct[np.minimum(j, T - j)]
        got = we.waveform(U, harmonics, T, ct, st, range(n))
        want = ref.waveform(U, harmonics, T, ct, st)
        v = got["v"][0]
        assert _same(v[:, 1:], v[:, :0:-1])                          # v[k] = v[T - k]
        kp = got["kpeak"][0]
        tied = (kp != 0) & (kp != T // 2)
        assert tied.any() and (kp <= T // 2).all()
        assert _same(np.abs(v[tied, kp[tied]]), np.abs(v[tied, T - kp[tied]]))
        assert _same(kp, want["kpeak"][0]) and _same(got["peak"], want["peak"])


@pytest.mark.parametrize("T", [4, 64, 1024, 4096])
def test_a_pure_sine_has_peak_amplitude_and_crest_sqrt_two_exactly(T):
    amps = np.array([1.0, 0.5, 2.0, 1.03, 1.1, 0.97, 0.49, 3.3, 325.26911934581187, 1e-3])
    U = np.zeros((1, len(amps), 1), dtype=np.complex128)
    U[0, :, 0] = amps
    ct, st = we.table(T)
    got = we.waveform(U, [1], T, ct, st)
    assert _same(got["peak"][0], amps) and (got["kpeak"] == 0).all()
    assert (got["crest"] == np.sqrt(2.0)).all(), got["crest"] - np.sqrt(2.0)
    want = ref.waveform(U, [1], T, ct, st)
    assert _same(got["crest"], want["crest"]) and _same(got["slack"], want["slack"])


@pytest.mark.parametrize("name", ["syn1000_H51_c", "net1_H51_c", "lin4_H11_c"])
@pytest.mark.parametrize("T", [256, 1024])
def test_the_sampled_peak_brackets_the_finer_one_within_its_slack(name, T):
    """peak_T <= peak_16T <= peak_T + slack_T with peak_T, slack_T AND peak_16T from the header's functions (the emulator takes any power of
    two, 16 T = 16 384 included; the table of wave_table): the samples of T are samples of 16 T (same doubles: the angle 2 pi j / T is formed by
    the same product), and the continuous peak -- above every sampled one -- lies within slack_T of peak_T."""
    harmonics, n, Hn, U = golden(name, 2)
    w1 = we.waveform(U, harmonics, T, *we.table(T))
    w16 = we.waveform(U, harmonics, 16 * T, *we.table(16 * T))
    assert (w1["slack"] > 0).all() and (w16["slack"] < w1["slack"]).all()
    assert (w1["peak"] <= w16["peak"]).all() and (w16["peak"] <= w1["peak"] + w1["slack"]).all()
    worst = float(((w16["peak"] - w1["peak"]) / w1["slack"]).max())
    print("\nWAVEFORM %s, T = %d: largest (peak_16T - peak_T) / slack_T = %.3f" % (name, T, worst))
    assert 0.0 <= worst <= 1.0


def _scenario_stats(S=24):
    harmonics, n, Hn, U = golden("net1_H51_c", S)
    ct, st = ref.lib_table(256)
    w = we.waveform(U, harmonics, 256, ct, st)
    flags = np.ones(S, dtype=np.int32)
    flags[7] = 2                                                    # not converged: skipped
    flags[9] = 256 | 2                                              # started warm, not converged: deferred
    flags[11] = 1 | 8                                               # reported by the queue: deferred there, added by an explicit add
    thd = np.full(S, 0.05)
    thd[13] = np.inf                                                # a non-finite THD: skipped
    lim = np.array([np.median(w["peak"][:, i]) for i in range(n)])
    return n, w, flags, thd, lim, float(np.median(w["crest"]))


def test_emulated_accumulator_matches_numpy_and_merge_of_halves_equals_the_whole():
    S = 24
    n, w, flags, thd, lim, climit = _scenario_stats(S)
    ids = 100 + np.arange(S)

    def stats(sl, queue):
        a = we.accumulate(w["peak"][sl], w["crest"][sl], ids[sl], flags[sl], thd[sl], lim, climit, queue=queue)
        return sweep.WaveformStats(256, lim, climit, **a)

    for queue in (False, True):
        whole = stats(slice(0, S), queue)
        dfr = (flags == (256 | 2)) | (queue & ((flags & 8) != 0))
        want = ref.accumulate(w["peak"], w["crest"], ids, flags, np.isfinite(thd), lim, climit, deferred=dfr)
        assert whole.counts.tolist() == want["counts"].tolist() == [S - 3 - int(queue), 2, 1 + int(queue)]
        for f in ref.EXACT:
            assert _same(getattr(whole, f), want[f]), f
        for f in ref.SUMS:
            assert np.allclose(getattr(whole, f), want[f], rtol=S * 2.0 ** -52, atol=0), f
        assert 0 < whole.peak_over.sum() < whole.added * n and 0 < whole.crest_over.sum() < whole.added * n
        for cut in (1, 10, 12, S - 1):
            both = stats(slice(0, cut), queue).merge(stats(slice(cut, S), queue))
            other = stats(slice(cut, S), queue).merge(stats(slice(0, cut), queue))
            for f in ref.EXACT:
                assert _same(getattr(both, f), getattr(whole, f)) and _same(getattr(other, f), getattr(whole, f)), (cut, f)
            for f in ref.SUMS:
                assert np.allclose(getattr(both, f), getattr(whole, f), rtol=S * 2.0 ** -52, atol=0), f
    # an equal maximum in two scenarios: the smaller id, whichever half it sits in
    pk = np.repeat(w["peak"][:1], 4, axis=0)
    a = we.accumulate(pk, pk, [40, 30, 20, 50], np.ones(4, np.int32), np.zeros(4))
    assert (a["peak_arg"] == 20).all() and (a["crest_arg"] == 20).all() and a["counts"].tolist() == [4, 0, 0]
    # the list as the device walks it (slots, terminator, gids, id_base; bits 8 and 9): 6 storages x 5 buses
    rng = np.random.default_rng(12)
    S, n = 6, 5
    pk, cr = rng.uniform(0.9, 1.1, (S, n)), rng.uniform(1.3, 1.5, (S, n))
    pk[de.LIST_TIED[0]], cr[de.LIST_TIED[0]] = 1.2, 1.6             # the largest of every bus ...
    pk[de.LIST_TIED[1]], cr[de.LIST_TIED[1]] = 1.2, 1.6             # ... twice
    lim, thd = np.full(n, 1.0), np.full(S, 0.05)
    for kw, sel, eids, efl, dfr, counts in de.list_cases(S):
        for queue in (False, True):
            got = we.accumulate(pk, cr, None, kw["flags"], thd, lim, 1.4, queue=queue, slots=kw["slots"], gids=kw["gids"], id_base=kw["id_base"])
            want = ref.accumulate(pk[sel], cr[sel], eids, efl, np.ones(len(sel), bool), lim, 1.4, deferred=dfr)
            assert got["counts"].tolist() == want["counts"].tolist() == counts
            for f in ref.EXACT:
                assert _same(got[f], want[f]), f
            for f in ref.SUMS:
                assert np.allclose(got[f], want[f], rtol=S * 2.0 ** -52, atol=0), f
        if kw["id_base"]:
            assert (got["peak_arg"] == 1001).all() and (got["crest_arg"] == 1001).all()     # 1000 + gid; the tie: not 1005, which came first


def test_waveformstats_container_round_trips():
    n, w, flags, thd, lim, climit = _scenario_stats()
    S = len(flags)
    st = sweep.WaveformStats(256, lim, climit, **we.accumulate(w["peak"], w["crest"], np.arange(S), flags, thd, lim, climit))
    back = st.unpack(st.pack())
    for f in sweep.WaveformStats.ARRAYS:
        assert _same(getattr(back, f), getattr(st, f)) and getattr(back, f).dtype == getattr(st, f).dtype, f
    assert st.pack().size == 24 + 64 * n and back.samples == 256 and back.crest_limit == climit
    ids = 7 + 3 * np.arange(S)
    moved = st.with_ids(ids)
    assert _same(moved.peak_arg, ids[st.peak_arg]) and _same(moved.crest_arg, ids[st.crest_arg]) and _same(moved.peak_max, st.peak_max)
    empty = sweep.WaveformStats(256, lim, climit, **we.empty(n))
    assert (empty.with_ids(ids).peak_arg == -1).all() and np.isnan(empty.mean()).all()
    for f in sweep.WaveformStats.ARRAYS:
        assert _same(getattr(empty.merge(st), f), getattr(st, f)) and _same(getattr(st.merge(empty), f), getattr(st, f)), f
    assert sweep.gather_waveform_stats(st, 1, ids).peak_arg.tolist() == moved.peak_arg.tolist()
    assert np.allclose(st.mean("peak"), st.peak_sum / st.added) and (st.std("crest") >= 0).all()
    b, sid, val = st.worst(1)[0]
    assert val == st.peak_max.max() and sid == st.peak_arg[b]
    with pytest.raises(ValueError):
        st.merge(sweep.WaveformStats(512, lim, climit, **we.empty(n)))
    with pytest.raises(ValueError):
        st.merge(sweep.WaveformStats(256, lim, climit + 1, **we.empty(n)))


def test_argument_checks_that_need_no_device():
    lib = _lib.load()
    buf = np.zeros(8192)
    p = buf.ctypes.data_as(_lib.c_dbl_p)
    for T in (0, -64, 32, 63, 100, 1000, 8192, 4097):
        assert lib.hpf_waveform_table(T, p, p) == -1, T
    assert lib.hpf_waveform_table(64, None, p) == -1 and lib.hpf_waveform_table(64, p, None) == -1
    assert buf.sum() == 0
    # (a NULL handle is refused first: the order, selection and T checks behind it need a handle and are tested in tests/test_gpu_waveform.py)
    orders = np.array([1, 3, 5, 7], dtype=np.int32)
    o = orders.ctypes.data_as(_lib.c_int_p)
    assert lib.hpf_waveform(None, o, 1024, 0, None, None, None, None, None, None) == -1
    assert lib.hpf_waveform(None, o, 100, 0, None, None, None, None, None, None) == -1
    assert lib.hpf_waveform_stats_begin(None, o, 1024, None, np.inf) == -1
    assert lib.hpf_waveform_stats_add(None, 0) == -1
    assert lib.hpf_waveform_stats_get(None, *[None] * 11) == -1
    assert lib.hpf_waveform_stats_end(None) == -1
