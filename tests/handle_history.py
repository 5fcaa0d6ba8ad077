"""Episodes: self-contained uses of one libhpf handle (tests/test_gpu_handle_history.py).  Test infrastructure only.

An EPISODE defines its own batch (set_loads, then set_state / apply_start -- or it is one solve_queue call), sets every option it relies on and
puts back to the default every option it changed, closes what it opened, and returns a dict of named numpy arrays and return codes.  By the
call-order rules of include/hpf.h its outputs then depend on nothing that happened on the handle before it, so the yardstick of an episode is
the same episode on a FRESH handle of the same slot count (`reference`, computed once per kind and cached), and the comparison is byte equality
(`same`): two runs of one configuration are bit-identical everywhere in this project -- records, voltages, err_hist with its NaN tail, eta, the
CSR Jacobian, and every array of the three accumulators, the sums included: the order in which hpf_solve_queue harvests scenarios is fixed by
the device-side lists for a fixed slot count, queue chunk and group count (tests/test_gpu_branch.py, test_both_accumulators_open_change_neither,
asserts the same).

The feeder and the helpers are those of tests/mixed_batch.py: synth.gen(90, seed=0), harmonics to 27 (b = 28), scenario s with the loads
P0 * synth.scenario_scale(n, s).  Three kinds of handle: "radial" (72 slots, batches of 70 / 5 / 17 / 1, a queue of 100: the 16-scenario
tiles, the group boundary at slot 32, ragged tiles and the queue's refill all occur), "meshed" (the feeder + 2 ties) and "dense" (8 slots,
batches of 5 / 1 / 3, a queue of 12).

R episodes are refusals.  Each call named there is refused by a check that runs on the host before any HIP call (read in csrc/hpf_lib.hip:
hpf_set_sources, hpf_set_loads, hpf_set_state, hpf_iterate, hpf_get_sources, accum_add, hpf_start_apply, hpf_set_option, hpf_solve_queue); the
episode asserts the documented code and hpf_num_scenarios before and after the refused call."""
import numpy as np

import mixed_batch as mb

OK, E_ARG, E_STATE = 0, -1, -2
DEFAULTS = {"pivot_growth_limit_log10": 10, "auto_repivot": 1, "rectangular_update": 0, "step_residual_check": 0, "keep_previous_state": 0,
            "block_pivoting": 0, "scenario_groups": 4, "queue_chunk": 4}
KINDS = {"radial": dict(ties=0, solver="block_tree", slots=72, big=70, small=5, mid=17, few=5, queue=100, short=90),
         "meshed": dict(ties=2, solver="block_tree", slots=8, big=5, small=1, mid=3, few=3, queue=12, short=10),
         "dense": dict(ties=0, solver="dense", slots=8, big=5, small=1, mid=3, few=3, queue=12, short=10)}
MIXED = "NBAAB"


class Ctx:
    """one kind of handle: the feeder, the sizes, every input an episode needs (prepared once, never changed) and the cached references"""

    def __init__(self, kind, outdir):
        from harmonic_power_flow_amd import synth
        self.kind = kind
        self.__dict__.update(KINDS[kind])
        self.net = net = mb.feeder(outdir, ties=self.ties)
        n = net["n"]
        rows = max(self.queue, self.slots + 1)
        scale = np.stack([synth.scenario_scale(n, s) for s in range(rows)])
        self.P, self.Q = net["P0"] * scale, net["Q0"] * scale
        self.mixed = mb.compose(net, MIXED, solver=self.solver)
        dm = self.fresh(1)
        try:
            self.m, self.nnl = dm.m, dm.n - dm.m
            dm.set_loads(net["P0"], net["Q0"])                 # the base case of E7 and the given state of E12: solved + two more iterations
            dm.set_state(None, None, n_scen=1)
            dm.fund_pf(1e-6, 30)
            _, err, _ = dm.solve(mb.THRESH, mb.MAX_ITER)
            assert err[0] <= mb.THRESH
            dm.mismatch(want_f=False)
            dm.iterate(2)
            dm.sync()
            Vm, Va = dm.get_state()
            self.base = (Vm[0].copy(), Va[0].copy())
        finally:
            dm.close()
        rng = np.random.default_rng(7)                         # (a, phi) of hpf_set_sources form 1: the ranges of tests/test_gpu_devmem.py
        self.ab = np.stack([1.0 + 0.05 * rng.uniform(-1, 1, (rows, self.nnl)), 0.02 * rng.uniform(-1, 1, (rows, self.nnl))], axis=2)
        self.refs = {}

    def fresh(self, slots=None):
        return mb.model(self.net, self.slots if slots is None else slots, self.solver)

    def reference(self, name):
        if name not in self.refs:
            dm = self.fresh()
            try:
                self.refs[name] = EPISODES[name](dm, self)
            finally:
                dm.close()
        return self.refs[name]


# ---- what episodes are made of ------------------------------------------------------------------------------------------------------------------

def _seeded(dm, c, S, sources=None):
    """the batch of scenarios 0 .. S-1 at its pf seed"""
    dm.set_loads(c.P[:S], c.Q[:S])
    if sources is not None:
        dm.set_sources(sources, "scale_shift")
    dm.set_state(None, None, n_scen=S)
    nf, ef, _ = dm.fund_pf(1e-6, 30)
    return {"pf_iter": nf, "pf_err": ef}


def _solved(dm, out, max_iter=mb.MAX_ITER, **kw):
    res = dm.solve(mb.THRESH, max_iter, **kw)
    out.update(n_iter=res[0], err=res[1], err_hist=res[2], stats=dm.stats())
    out["Vm"], out["Va"] = dm.get_state()
    return res


def _plain(S, max_iter=mb.MAX_ITER):
    """S: a size of KINDS by name, or a number"""
    def run(dm, c):
        size = getattr(c, S) if isinstance(S, str) else S
        out = _seeded(dm, c, size)
        _solved(dm, out, max_iter)
        assert out["err_hist"].shape == (size, max_iter + 1) and (out["n_iter"] <= max_iter).all()
        return out
    return run


def _mixed(repivot):
    """E5: N B A A B at limit 0 (mb.compose); what each kind of handle does with it is what tests/test_gpu_mixed_batches.py states"""
    def run(dm, c):
        dm.set_option("pivot_growth_limit_log10", 0)
        dm.set_option("auto_repivot", repivot)
        try:
            out = mb.solve_on(dm, c.mixed)
        finally:
            dm.set_option("pivot_growth_limit_log10", DEFAULTS["pivot_growth_limit_log10"])
            dm.set_option("auto_repivot", DEFAULTS["auto_repivot"])
        out.pop("jac")
        repeats = c.kind == "radial" and repivot == 1
        want = {"N": 4 | (16 if repeats else 0), "B": 1, "A": 1 if c.kind == "dense" else (1 | 8 | (16 if repeats else 0))}
        got = out["stats"]["flags"] & ~mb.MODE_BITS
        assert got.tolist() == [want[k] for k in MIXED], (c.kind, repivot, got)
        return out
    return run


def _sources(clear):
    def run(dm, c):
        S = c.mid
        out = _seeded(dm, c, S, sources=c.ab[:S])
        _solved(dm, out)
        out["I_src"] = dm.get_sources()
        assert (out["stats"]["flags"] & 1024).all()
        if clear:
            dm.clear_sources()
        return out
    return run


def _start(dm, c):
    S = c.few
    dm.set_start(*c.base)
    try:
        dm.set_loads(c.P[:S], c.Q[:S])
        dm.apply_start(S)
        out = {}
        _solved(dm, out)
        out["start_Vm"], out["start_Va"] = dm.get_start()
        assert (out["stats"]["flags"] & 256).all()
    finally:
        dm.clear_start()
    return out


def _start_then_loads(dm, c):
    """E7': the sweep's re-solve order -- apply_start, THEN set_loads of the same size, solve: the state and bit 8 survive the loads (hpf.h at
    hpf_set_loads)"""
    S = c.few
    dm.set_start(*c.base)
    try:
        dm.set_loads(c.P[:S], c.Q[:S])
        dm.apply_start(S)
        dm.set_loads(c.P[1:S + 1], c.Q[1:S + 1])
        out = {}
        out["Vm_entered"], out["Va_entered"] = dm.get_state()
        assert np.array_equal(out["Vm_entered"], np.tile(c.base[0], (S, 1))) and np.array_equal(out["Va_entered"], np.tile(c.base[1], (S, 1)))
        _solved(dm, out)
        assert (out["stats"]["flags"] & 256).all()
    finally:
        dm.clear_start()
    return out


def _option(name, value, S="mid", extra=None):
    def run(dm, c):
        dm.set_option(name, value)
        try:
            out = _seeded(dm, c, getattr(c, S))
            _solved(dm, out)
            if extra:
                extra(dm, out)
        finally:
            dm.set_option(name, DEFAULTS[name])
        return out
    return run


def _eta(dm, out):
    out["eta_last"], out["eta_max"] = dm.step_residuals()


def _jac(dm, out):
    J = dm.jacobian_csr(0, last=True)
    out["J_data"], out["J_indices"], out["J_indptr"] = J.data.copy(), J.indices.copy(), J.indptr.copy()


def _trace(dm, c):
    out = _seeded(dm, c, 3)
    res = _solved(dm, out, trace=True)
    out["Vm_traj"], out["Va_traj"] = res[3], res[4]
    return out


def _iterate(dm, c):
    out = _seeded(dm, c, c.mid)
    out["f"], out["e0"] = dm.mismatch()
    dm.iterate(3)
    dm.sync()
    out["Vm"], out["Va"] = dm.get_state()
    return out


def _accum_out(out, pre, stats):
    for f in type(stats).ARRAYS:
        out[pre + f] = np.asarray(getattr(stats, f)).copy()


def _queue(variant):
    def run(dm, c):
        G = c.queue
        out = {}
        if variant == "sources":
            dm.queue_sources(c.ab[:G], "scale_shift")
        if variant == "accum":
            dm.distortion_begin()
            dm.branch_stats_begin()
            dm.waveform_stats_begin(256)
        if variant == "chunk1":
            dm.set_option("queue_chunk", 1)
        try:
            out["rec"], out["Vm"], out["Va"] = dm.solve_queue(c.P[:G], c.Q[:G], want_voltages=True)
            if variant == "accum":
                _accum_out(out, "dist_", dm.distortion_get())
                _accum_out(out, "branch_", dm.branch_stats_get())
                _accum_out(out, "wave_", dm.waveform_stats_get())
                fl = out["rec"]["flags"]                     # added: converged and not reported for a re-solve (include/hpf.h)
                assert out["dist_counts"][0] == out["branch_counts"][0] == out["wave_counts"][0] == ((fl & (1 | 4 | 8 | 64)) == 1).sum() > 0
        finally:
            if variant == "accum":
                dm.distortion_end()
                dm.branch_stats_end()
                dm.waveform_stats_end()
            if variant == "chunk1":
                dm.set_option("queue_chunk", DEFAULTS["queue_chunk"])
        src = (out["rec"]["flags"] & 1024) != 0
        assert (src.all() if variant == "sources" else not src.any()) and dm.S == 0
        return out
    return run


def _flows(dm, c):
    """E12: branch_flows and waveform after set_state of a given state alone, then after a solve"""
    S, n = c.few, c.net["n"]
    dm.set_loads(c.P[:S], c.Q[:S])
    dm.set_state(np.tile(c.base[0], (S, 1)), np.tile(c.base[1], (S, 1)))
    out = {}
    for tag in ("given_", "solved_"):
        for k, v in dm.branch_flows().items():
            out[tag + "br_" + k] = v
        for k, v in dm.waveform(256, buses=[0, n - 1]).items():
            out[tag + "wf_" + k] = v
        if tag == "given_":
            _solved(dm, out)
    return out


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------

def refused(dm, want, fn, *args):
    """fn(*args) must raise HpfError(want) and leave hpf_num_scenarios alone -> {"code", "S_moved"} (the count itself belongs to whatever batch the
    handle held before an episode that sets none: no output)"""
    from harmonic_power_flow_amd._lib import HpfError
    before = dm.S
    try:
        fn(*args)
        code = OK
    except HpfError as e:
        code = e.code
    after = dm.S
    assert code == want and after == before, (getattr(fn, "__name__", "call"), code, want, before, after)
    return {"code": np.int64(code), "S_moved": np.int64(after - before)}


def _three(dm, c):
    dm.set_loads(c.P[:3], c.Q[:3])


def _r_sources_rows(dm, c):
    _three(dm, c)
    return refused(dm, E_ARG, dm.set_sources, c.ab[:2], "scale_shift")


def _r_loads_too_many(dm, c):
    return refused(dm, E_ARG, dm.set_loads, c.P[:c.slots + 1], c.Q[:c.slots + 1])


def _r_state_other_size(dm, c):
    _three(dm, c)
    return refused(dm, E_ARG, lambda: dm.set_state(None, None, n_scen=2))


def _r_iterate_no_mismatch(dm, c):
    _three(dm, c)
    dm.set_state(None, None, n_scen=3)
    return refused(dm, E_STATE, dm.iterate, 1)


def _r_get_sources(dm, c):
    _three(dm, c)
    return refused(dm, E_STATE, dm.get_sources)


def _r_add_closed(dm, c):
    _three(dm, c)
    out = {}
    for name in ("distortion_add", "branch_stats_add", "waveform_stats_add"):
        out.update({name + "_" + k: v for k, v in refused(dm, E_STATE, getattr(dm, name), 0).items()})
    return out


def _r_apply_no_start(dm, c):
    _three(dm, c)
    return refused(dm, E_STATE, dm.apply_start, 3)


def _r_option_range(dm, c):
    out = {}
    for name, value in (("queue_chunk", 17), ("scenario_groups", 9), ("rectangular_update", 2), ("step_residual_check", 2),
                        ("pivot_growth_limit_log10", 301), ("no_such_option", 1)):
        out.update({name + "_" + k: v for k, v in refused(dm, E_ARG, dm.set_option, name, value).items()})
    return out


def _r_queue_registration(dm, c):
    """sources registered for another number of scenarios: refused, nothing solved, the registration gone (the next queue runs without sources:
    E11 checks bit 10 of every record)"""
    dm.queue_sources(c.ab[:c.short], "scale_shift")
    return refused(dm, E_ARG, lambda: dm.solve_queue(c.P[:c.queue], c.Q[:c.queue]))


def _r_meshed_pivoting(dm, c):
    return refused(dm, E_STATE, dm.set_option, "block_pivoting", 1)


EPISODES = {
    "E1_big": _plain("big"),
    "E2_small_3_iterations": _plain("small", 3),
    "E3_mid_60_iterations": _plain("mid", 60),
    "E4_one_0_iterations": _plain(1, 0),
    "E5_mixed": _mixed(1),
    "E5_mixed_no_repivot": _mixed(0),
    "E6_sources_cleared": _sources(True),
    "E6_sources_left": _sources(False),
    "E7_start": _start,
    "E7_start_then_loads": _start_then_loads,
    "E8_rectangular": _option("rectangular_update", 1),
    "E8_step_check": _option("step_residual_check", 1, extra=_eta),
    "E8_keep_previous": _option("keep_previous_state", 1, extra=_jac),
    "E8_block_pivoting": _option("block_pivoting", 1),
    "E8_one_group": _option("scenario_groups", 1, S="big"),
    "E9_trace": _trace,
    "E10_iterate": _iterate,
    "E11_queue": _queue("plain"),
    "E11_queue_sources": _queue("sources"),
    "E11_queue_accumulators": _queue("accum"),
    "E11_queue_chunk1": _queue("chunk1"),
    "E12_flows_and_waveforms": _flows,
    "R_sources_rows": _r_sources_rows,
    "R_loads_too_many": _r_loads_too_many,
    "R_state_other_size": _r_state_other_size,
    "R_iterate_no_mismatch": _r_iterate_no_mismatch,
    "R_get_sources": _r_get_sources,
    "R_add_closed": _r_add_closed,
    "R_apply_no_start": _r_apply_no_start,
    "R_option_range": _r_option_range,
    "R_queue_registration": _r_queue_registration,
    "R_meshed_pivoting": _r_meshed_pivoting,
}


def names(kind):
    """-> (E episodes in the listed order, R episodes) of a kind of handle: block_pivoting = 1 is an episode where the handle takes it and a
    refusal on the meshed handle"""
    E = [k for k in EPISODES if k.startswith("E") and not (kind == "meshed" and k == "E8_block_pivoting")]
    R = [k for k in EPISODES if k.startswith("R") and (kind == "meshed" or k != "R_meshed_pivoting")]
    return E, R


def fixed_order(kind):
    """every episode in the listed order, a refusal after every third (those left over at the end)"""
    E, R = names(kind)
    out, r = [], 0
    for i, e in enumerate(E):
        out.append(e)
        if i % 3 == 2 and r < len(R):
            out.append(R[r])
            r += 1
    return out + R[r:]


PARTS = {"radial": 1, "meshed": 1, "dense": 6}               # a dense episode factors 2 518 x 2 518 matrices some 30 times: its lists run in six handles


def parts(order, kind):
    """the list cut into PARTS[kind] consecutive pieces, one long-lived handle each"""
    k = PARTS[kind]
    cut = [len(order) * i // k for i in range(k + 1)]
    return [order[a:b] for a, b in zip(cut, cut[1:])]


def same(a, b):
    """byte equality of two episode results -> the names that differ (empty: equal)"""
    bad = [k for k in sorted(set(a) | set(b)) if k not in a or k not in b]
    for k in sorted(set(a) & set(b)):
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.dtype != y.dtype or x.shape != y.shape or np.ascontiguousarray(x).tobytes() != np.ascontiguousarray(y).tobytes():
            bad.append(k)
    return bad


def run_and_compare(dm, c, name, before):
    """episode `name` on the used handle dm against its reference; `before`: what ran on dm so far (for the message)"""
    got = EPISODES[name](dm, c)
    bad = same(got, c.reference(name))
    assert not bad, "%s handle: episode %s differs from a fresh handle in %s after %s" % (c.kind, name, bad, list(before))
    return got
