"""The per-entry arithmetic of the distortion accumulator (csrc/hpf_distortion.hpp: what k_distortion_add runs per thread), executed serially
on the host against the NumPy restatement tests/distortion_ref.py.  No GPU involved.

On the host sqrt and / are correctly rounded on both sides, so max, arg, over, the histogram and the counts must be EQUAL; the four sums may
differ by the order of summation only: a recursive sum of `added` non-negative terms is within added x 2^-53 x (sum) of the exact one whatever
the order, hence the two sides within added x 2^-52 x sum |x| (resp. sum x^2: the products are the same doubles on both sides)."""
import numpy as np
import pytest

import distortion_emul as de
import distortion_ref as ref

GOLDEN = ["net1_H11_c", "net2_H11_c", "net3_H11_c", "net1_H51_c", "net2_H51_c", "net3_H51_c"]


def check(got, want, exact=True):
    for f in ref.EXACT:
        assert np.array_equal(got[f], want[f]), f
    added = int(want["counts"][0])
    x, thd = want["x"], want["thd"]
    for f, s in (("x_sum", x.sum(0)), ("x_sumsq", (x * x).sum(0)), ("thd_sum", thd.sum(0)), ("thd_sumsq", (thd * thd).sum(0))):
        assert (np.abs(got[f] - want[f]) <= ref.sum_bound(s, added)).all(), f


@pytest.mark.parametrize("name", GOLDEN)
def test_golden_voltages_in_twenty_perturbed_scenarios(name):
    Vm, ids, flags, n, Hn = de.golden_case(name)
    cfg = de.settings_for(Vm, flags, n, Hn)
    got = de.accumulate(Vm, ids, flags, n, Hn, **cfg)
    want = ref.accumulate(Vm, ids, flags, n, Hn, **cfg)
    assert want["counts"].tolist() == [19, 1, 0]
    assert 0 < want["thd_over"].sum() < 19 * n and (want["x_over"].sum(axis=1) > 0).all()      # the limits do cut the samples
    assert want["thd_hist"][:, -1].sum() == 0 and (want["thd_hist"].sum(axis=1) == 19).all()
    check(got, want)
    assert (got["x_arg"] != 7).all() and (got["thd_arg"] != 7).all()


def _edge_case():
    """12 scenarios x 5 buses x 4 harmonic positions of random signed magnitudes: a negative fundamental, two identical scenarios (tied maxima,
    the later one carrying the SMALLER id), a sample equal to its limit, thd exactly hist_max and beyond, a NaN scenario, a diverged one."""
    rng = np.random.default_rng(11)
    S, n, Hn = 12, 5, 4
    V = rng.uniform(-1.0, 1.0, (S, Hn, n))
    V[:, 0, :] = rng.uniform(0.9, 1.1, (S, n)) * np.where(rng.random((S, n)) < 0.3, -1.0, 1.0)
    V[:, 1:, :] *= 0.25
    V[3] *= 1.5                                             # the largest samples of most entries ...
    V[8] = V[3]                                             # ... twice
    V[5, :, 0] = [2.0, 0.0, 1.0, 0.0]                       # thd = 0.5 exactly
    V[6, :, 0] = [-1.0, 1.0, 1.0, 1.0]                      # thd = sqrt(3)
    V[9, 2, 4] = np.nan
    ids = np.array([40, 41, 42, 43, 44, 45, 46, 47, 8, 49, 50, 51])
    flags = np.ones(S, dtype=np.int32)
    flags[10] = 2
    Vm = V.reshape(S, Hn * n)
    x, thd = ref.samples(Vm, n, Hn)
    limit = np.array([1.0, x[1, 1, 2], x[4, 2, 1], 0.1])   # two samples sit exactly on their limit: > is strict
    return Vm, ids, flags, n, Hn, dict(limit=limit, thd_limit=float(thd[2, 3]), hist_max=0.5, bins=7)


def test_ties_strict_limits_histogram_edges_and_skipped_scenarios():
    Vm, ids, flags, n, Hn, cfg = _edge_case()
    assert (Vm.reshape(-1, Hn, n)[:, 0, :] < 0).any()
    got = de.accumulate(Vm, ids, flags, n, Hn, **cfg)
    want = ref.accumulate(Vm, ids, flags, n, Hn, **cfg)
    assert want["counts"].tolist() == [10, 2, 0]
    check(got, want)
    assert (got["x_arg"] == 8).sum() > 0 and (got["x_arg"] != 43).all()            # tie: the smaller id, although it arrived later
    x, thd = want["x"], want["thd"]
    assert got["x_over"][1, 2] == (x[:, 1, 2] > cfg["limit"][1]).sum() < (x[:, 1, 2] >= cfg["limit"][1]).sum()
    assert got["thd_over"][3] == (thd[:, 3] > cfg["thd_limit"]).sum() < (thd[:, 3] >= cfg["thd_limit"]).sum()
    assert got["thd_hist"][0, -1] >= 2                       # thd == hist_max and sqrt(3) both land in the overflow bin
    assert (got["thd_hist"].sum(axis=1) == 10).all()


def test_accumulating_in_two_calls_equals_one_and_the_queue_defers_reported_scenarios():
    Vm, ids, flags, n, Hn, cfg = _edge_case()
    one = de.accumulate(Vm, ids, flags, n, Hn, **cfg)
    two = de.accumulate(Vm[:5], ids[:5], flags[:5], n, Hn, **cfg)
    two = de.accumulate(Vm[5:], ids[5:], flags[5:], n, Hn, into=two, **cfg)
    for f in de.NAMES:
        assert np.array_equal(one[f], two[f]), f               # (the same order of arrival: the sums too)
    fl = flags.copy()
    fl[0] |= 8
    fl[1] |= 64
    fl[10] |= 4
    q = de.accumulate(Vm, ids, fl, n, Hn, queue=True, **cfg)
    dfr = np.zeros(len(ids), bool)
    dfr[[0, 1, 10]] = True
    want = ref.accumulate(Vm, ids, fl, n, Hn, deferred=dfr, **cfg)
    assert want["counts"].tolist() == [8, 1, 3]
    check(q, want)
    check(de.accumulate(Vm, ids, fl, n, Hn, queue=False, **cfg), ref.accumulate(Vm, ids, fl, n, Hn, **cfg))     # hpf_distortion_add: no deferral
    # the list as the device walks it (slots, terminator, gids, id_base; bits 8 and 9): 6 storages x 5 buses x 3 harmonic positions
    rng = np.random.default_rng(12)
    S, n, Hn = 6, 5, 3
    V = rng.uniform(-1.0, 1.0, (S, Hn, n))
    V[:, 0, :] = rng.uniform(0.9, 1.1, (S, n))
    V[:, 1:, :] *= 0.1
    V[de.LIST_TIED[0], 0, :] = 1.5                                     # the largest fundamental and, three times the others' harmonics, the
    V[de.LIST_TIED[0], 1:, :] = 0.3                                    # largest distortion of every bus ...
    V[de.LIST_TIED[1]] = V[de.LIST_TIED[0]]                            # ... twice
    Vm = V.reshape(S, Hn * n)
    cfg = dict(limit=np.array([1.0, 0.05, 0.05]), thd_limit=0.07, hist_max=0.5, bins=7)
    for kw, sel, eids, efl, dfr, counts in de.list_cases(S):
        for queue in (False, True):
            got = de.accumulate(Vm, None, kw["flags"], n, Hn, queue=queue, slots=kw["slots"], gids=kw["gids"], id_base=kw["id_base"], **cfg)
            want = ref.accumulate(Vm[sel], eids, efl, n, Hn, deferred=dfr, **cfg)
            assert got["counts"].tolist() == want["counts"].tolist() == counts
            check(got, want)
        if kw["id_base"]:
            assert (got["x_arg"] == 1001).all() and (got["thd_arg"] == 1001).all()      # 1000 + gid; the tie: not 1005, which came first


def test_nothing_added_leaves_the_initial_values():
    Vm, ids, flags, n, Hn, cfg = _edge_case()
    got = de.accumulate(Vm, ids, np.zeros_like(flags), n, Hn, **cfg)
    want = ref.accumulate(Vm, ids, np.zeros_like(flags), n, Hn, **cfg)
    assert got["counts"].tolist() == [0, 12, 0] and (got["x_arg"] == -1).all() and (got["thd_arg"] == -1).all()
    for f in ref.EXACT + ref.SUMS:
        assert np.array_equal(got[f], want[f]) and (f.endswith("_arg") or f == "counts" or not got[f].any()), f
