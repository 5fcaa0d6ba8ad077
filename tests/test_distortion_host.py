"""Host side of the distortion statistics (sweep.DistortionStats, sweep.gather_distortion) and the argument checks of the four entry points.
No GPU involved: the per-part statistics come from the host emulation of the device arithmetic (tests/distortion_emul.py), the yardstick is the
NumPy restatement (tests/distortion_ref.py) of the whole set."""
import itertools
import os
import socket

import numpy as np
import pytest

import distortion_emul as de
import distortion_ref as ref

from harmonic_power_flow_amd import sweep


def _stats(arrays, Hn, cfg):
    return sweep.DistortionStats(list(range(1, 2 * Hn, 2)), cfg["limit"], cfg["thd_limit"], cfg["hist_max"],
                                 **{k: arrays[k] for k in sweep.DistortionStats.ARRAYS})


def _case(name="net1_H11_c"):
    Vm, ids, flags, n, Hn = de.golden_case(name)
    Vm[13] = Vm[4]                                           # tied maxima across parts
    return Vm, ids, flags, n, Hn, de.settings_for(Vm, flags, n, Hn)


def _check_whole(got, want):
    for f in ref.EXACT:
        assert np.array_equal(getattr(got, f), want[f]), f
    added, x, thd = int(want["counts"][0]), want["x"], want["thd"]
    for f, s in (("x_sum", x.sum(0)), ("x_sumsq", (x * x).sum(0)), ("thd_sum", thd.sum(0)), ("thd_sumsq", (thd * thd).sum(0))):
        assert (np.abs(getattr(got, f) - want[f]) <= ref.sum_bound(s, added)).all(), f


@pytest.mark.parametrize("name", ["net1_H11_c", "net3_H51_c"])
def test_merge_of_parts_in_any_order_gives_the_whole(name):
    Vm, ids, flags, n, Hn, cfg = _case(name)
    want = ref.accumulate(Vm, ids, flags, n, Hn, **cfg)
    for cuts in ((0, 9, 20), (0, 6, 13, 20)):
        parts = [_stats(de.accumulate(Vm[a:b], ids[a:b], flags[a:b], n, Hn, **cfg), Hn, cfg) for a, b in zip(cuts[:-1], cuts[1:])]
        for order in itertools.permutations(range(len(parts))):
            m = parts[order[0]]
            for k in order[1:]:
                m = m.merge(parts[k])
            _check_whole(m, want)
    empty = _stats(de.empty(n, Hn, cfg["bins"]), Hn, cfg)
    _check_whole(empty.merge(parts[0]).merge(parts[1]).merge(empty).merge(parts[2]), want)


def test_merge_refuses_mismatching_settings():
    Vm, ids, flags, n, Hn, cfg = _case()
    a = _stats(de.accumulate(Vm, ids, flags, n, Hn, **cfg), Hn, cfg)
    for change in (dict(thd_limit=cfg["thd_limit"] * 2), dict(hist_max=cfg["hist_max"] * 2), dict(bins=32), dict(limit=cfg["limit"] * 1.5)):
        c2 = dict(cfg, **change)
        with pytest.raises(ValueError):
            a.merge(_stats(de.accumulate(Vm, ids, flags, n, Hn, **c2), Hn, c2))
    Vm2, ids2, flags2, n2, Hn2 = de.golden_case("net2_H11_c")
    c2 = dict(cfg, limit=cfg["limit"][:Hn2])
    with pytest.raises(ValueError):
        a.merge(_stats(de.accumulate(Vm2, ids2, flags2, n2, Hn2, **c2), Hn2, c2))


@pytest.mark.parametrize("bins", [64, 5, 256])
def test_percentile_mean_std_and_worst_against_numpy(bins):
    Vm, ids, flags, n, Hn, cfg = _case("net1_H51_c")
    cfg = dict(cfg, bins=bins)
    st = _stats(de.accumulate(Vm, ids, flags, n, Hn, **cfg), Hn, cfg)
    want = ref.accumulate(Vm, ids, flags, n, Hn, **cfg)
    x, thd, added = want["x"], want["thd"], int(want["counts"][0])
    w = cfg["hist_max"] / bins
    for p in (0, 50, 90, 95, 99, 100):
        exact = np.percentile(thd, p, axis=0, method="higher")
        up = st.thd_percentile(p)
        # the bin [lo, hi) that holds the sample: lo <= exact < hi = up, so 0 < up - exact <= w (the edges are k * w rounded: 4 ulp of slack)
        assert (up - exact > -1e-12 * w).all() and (up - exact <= w * (1 + 1e-12)).all(), p
    # mean: |sum / added - mean| <= bound / added + one rounding; std from sum and sum of squares loses digits by cancellation: the bound of
    # var = sumsq / added - mean^2 is (a few) 2^-52 x mean(x^2), compared on the variance
    mx, mt = st.mean()
    sx, s_t = st.std()
    for got, got_s, v in ((mx, sx, x), (mt, s_t, thd)):
        m = v.mean(axis=0)
        assert (np.abs(got - m) <= (added + 2) * 2.0 ** -52 * np.abs(m)).all()
        assert (np.abs(got_s ** 2 - v.var(axis=0)) <= 4 * (added + 4) * 2.0 ** -52 * (v * v).mean(axis=0)).all()
    top = st.worst(3)
    order = np.argsort(-want["thd_max"], kind="stable")[:3]
    assert [t[0] for t in top] == order.tolist() and [t[1] for t in top] == want["thd_arg"][order].tolist()
    assert [t[2] for t in top] == want["thd_max"][order].tolist()
    # overflow bin: a percentile that falls there is reported as inf
    c2 = dict(cfg, hist_max=float(np.median(thd)))
    s2 = _stats(de.accumulate(Vm, ids, flags, n, Hn, **c2), Hn, c2)
    up = s2.thd_percentile(100)
    assert np.isinf(up[thd.max(axis=0) >= c2["hist_max"]]).all() and np.isinf(up).any()


def test_gather_with_world_one_applies_the_ids_and_pack_round_trips():
    Vm, ids, flags, n, Hn, cfg = _case()
    st = _stats(de.accumulate(Vm, np.arange(20), flags, n, Hn, **cfg), Hn, cfg)
    gids = sweep.scenario_ids(3, 8, 20)
    g = sweep.gather_distortion(st, 1, ids=gids)
    want = ref.accumulate(Vm, gids, flags, n, Hn, **cfg)
    _check_whole(g, want)
    assert sweep.gather_distortion(st, 1) is st
    back = st.unpack(st.pack())
    for f in sweep.DistortionStats.ARRAYS:
        assert np.array_equal(getattr(back, f), getattr(st, f)) and getattr(back, f).dtype == getattr(st, f).dtype


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    for p in (here, os.path.dirname(here)):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist
    import distortion_emul as de_
    from harmonic_power_flow_amd import sweep as sw
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    Vm, ids, flags, n, Hn, cfg = _case()
    mine = sw.scenario_ids(rank, world, len(ids) // world)
    local = de_.accumulate(Vm[mine], np.arange(len(mine)), flags[mine], n, Hn, **cfg)       # the device numbers a rank's scenarios locally
    out = sw.gather_distortion(_stats(local, Hn, cfg), world, ids=mine)
    q.put((rank, {f: getattr(out, f) for f in sw.DistortionStats.ARRAYS}))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_gather_merges_strided_shares_under_global_ids():
    import torch.multiprocessing as mp
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=180) for _ in range(world))
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    Vm, ids, flags, n, Hn, cfg = _case()
    want = ref.accumulate(Vm, ids, flags, n, Hn, **cfg)
    _check_whole(_stats(res[0], Hn, cfg), want)
    assert (want["thd_arg"] % 2 == 1).any() and (want["thd_arg"] % 2 == 0).any()            # maxima from both ranks
    for f in sweep.DistortionStats.ARRAYS:
        assert np.array_equal(res[0][f], res[1][f]), f                                      # every rank holds the same statistics, sums included


def test_entry_points_refuse_a_null_handle_before_any_device_call():
    from harmonic_power_flow_amd import _lib
    lib = _lib.load()
    assert lib.hpf_distortion_begin(None, None, 0.08, 0.2, 64) == -1
    assert lib.hpf_distortion_add(None, 0) == -1
    assert lib.hpf_distortion_get(None, *([None] * 12)) == -1
    assert lib.hpf_distortion_end(None) == -1
