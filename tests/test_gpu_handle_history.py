"""A reused handle behaves like a fresh one, call by call (run with -m gpu on an MI355X).

Production drives ONE handle through a whole sweep (sweep.solve_scenarios) and the reference-shaped calls borrow handles from an LRU (api.py);
nearly every other device test creates a handle, does one thing and destroys it.  What survives from one call to the next -- the host flags of
csrc/hpf_internal.hpp (loads_set, state_set, mismatch_valid, prev_valid, solve_done, from_start, src_set, start_set, the queue registration, the
trace, hist_cap, gj_mode around the pivoted repeat, every option, the accumulators' `open`) and the device arrays sized for S_max that no call
frees (d_hist, d_pivflag, d_eta, d_niter, d_err, d_stats, the repeat buffers, the previous state, the sources, the start state, the active lists,
the virtual slots of a meshed handle, the accumulators' scratch) -- is tested here as a whole.

1. Episodes (tests/handle_history.py) on one long-lived handle per kind (radial, meshed, dense): in the listed order with a refusal after every
   third (a), in three seeded permutations (b), and -- radial -- every episode after every other (c: the case that names a leaking pair).
   Every result equals the same episode on a fresh handle byte for byte; the message names the episode and what ran before it.  (The dense
   handle's lists are cut into six consecutive pieces, one handle each -- hh.PARTS: a pass over all its episodes takes 13 s.)
   (d) hpf_debug_device_memory after a second pass over all episodes equals its value after the first -- what the handle holds beyond the first
   episode is what its features allocate lazily, once -- and closing the handle returns every block.
2. The call-order rules of include/hpf.h as a table (tests/handle_contract.py) against three seeded random walks of 200 calls on a 12-bus
   feeder: every return code and hpf_num_scenarios, every entry accepted and refused at least once where a state allows it; and a directed case
   for each host fix a walk may not reach (hpf_clear_sources on a batch without sources, a change of block_pivoting before hpf_iterate).
3. The Python handle cache: reference-shaped calls in a seeded order on one network under handle_cache(4) against handle_cache(0).

DESIGN.md 3.15 has the episode table, what resets each flag and buffer, the guards that reading them for the walk changed, and the mutations
this file catches."""
import gc

import numpy as np
import pytest

from conftest import INPUTS

import handle_contract as hc
import handle_history as hh

pytestmark = pytest.mark.gpu

_CTX = {}
RADIAL = hh.names("radial")[0] + hh.names("radial")[1]


@pytest.fixture(scope="module")
def ctx(tmp_path_factory):
    def get(kind):
        if kind not in _CTX:
            _CTX[kind] = hh.Ctx(kind, tmp_path_factory.mktemp("history_" + kind))
        return _CTX[kind]
    yield get
    _CTX.clear()


def _run(c, order):
    dm = c.fresh()
    try:
        for i, name in enumerate(order):
            hh.run_and_compare(dm, c, name, order[:i])
    finally:
        dm.close()


# ---- 1. episodes ----------------------------------------------------------------------------------------------------------------------------

KIND_PARTS = [(kind, part) for kind in sorted(hh.KINDS) for part in range(hh.PARTS[kind])]
KIND_IDS = ["%s-part%d" % kp if hh.PARTS[kp[0]] > 1 else kp[0] for kp in KIND_PARTS]


@pytest.mark.parametrize("kind,part", KIND_PARTS, ids=KIND_IDS)
def test_every_episode_in_the_listed_order_equals_a_fresh_handle(ctx, kind, part):
    """(a): S = 70, then 5 with 3 iterations (err_hist of 4 columns in rows of 51), 17 with 60 (d_hist grows), 1 with none; the mixed batch with a
    NaN slot, a repeated slot and a never-activated slot; sources cleared and left; the start state; one option after the other; the trace;
    iterate; four queues; flows and waveforms -- and a refused call after every third."""
    _run(ctx(kind), hh.parts(hh.fixed_order(kind), kind)[part])


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("kind,part", KIND_PARTS, ids=KIND_IDS)
def test_every_episode_in_a_shuffled_order_equals_a_fresh_handle(ctx, kind, part, seed):
    """(b): the same list in three seeded permutations, each on a handle of its own"""
    order = hh.fixed_order(kind)
    _run(ctx(kind), hh.parts([order[i] for i in np.random.default_rng(seed).permutation(len(order))], kind)[part])


@pytest.mark.parametrize("first", RADIAL)
def test_every_episode_after_this_one_equals_a_fresh_handle(ctx, first):
    """(c), radial: X, Y, X, Y', X, Y'', ... over every Y on one handle"""
    c = ctx("radial")
    dm = c.fresh()
    try:
        ran = []
        for name in RADIAL:
            for step in (first, name):
                hh.run_and_compare(dm, c, step, ran[-4:])
                ran.append(step)
    finally:
        dm.close()


# what the episodes allocate once and keep beyond E1 (which itself brings d_hist and the three repeat buffers): 14 blocks
LAZY_BLOCKS = ("d_Vmp", "d_Vap", "d_swapVm", "d_swapVa",                  # keep_previous_state, hpf_jacobian_csr_last
               "d_respart", "d_eta",                                       # step_residual_check
               "d_jptr", "d_jval", "d_jcol",                               # the CSR Jacobian
               "d_br_from", "d_br_to", "d_br_y", "d_br_part",              # the branch table
               "d_src")                                                    # source storage (E6': not cleared; the queue with sources)


@pytest.mark.parametrize("kind,part", KIND_PARTS, ids=KIND_IDS)
def test_device_memory_settles_after_one_pass_and_goes_back(ctx, kind, part):
    """(d): what the episodes leave allocated beyond the first one is allocated once.  In blocks this is asserted exactly: a whole pass adds the
    14 of LAZY_BLOCKS (read in csrc/hpf_lib.hip: each is allocated where its feature is first used and kept) and nothing else -- a piece of the
    dense list at most those.  In bytes the expected figure would repeat the allocator's rounding and the growth of d_hist from 51 to 61
    columns, so there the assertion is that a second pass ends at exactly the figures of the first; closing returns everything."""
    from harmonic_power_flow_amd.device import device_memory as mem
    c = ctx(kind)
    order = hh.parts(hh.fixed_order(kind), kind)[part]
    gc.collect()
    base = mem()
    dm = c.fresh()
    try:
        created = mem()
        hh.EPISODES[order[0]](dm, c)
        first = mem()
        for name in order[1:]:
            hh.EPISODES[name](dm, c)
        once = mem()
        for name in order:
            hh.EPISODES[name](dm, c)
        twice = mem()
    finally:
        dm.close()
    gc.collect()
    print("\nHISTORY %s memory (blocks, bytes): created %s, after the first episode %s, after one pass %s, after two %s"
          % (kind, [a - b for a, b in zip(created, base)], [a - b for a, b in zip(first, base)], [a - b for a, b in zip(once, base)],
             [a - b for a, b in zip(twice, base)]))
    assert base[0] < created[0] <= first[0] <= once[0] and created[1] <= first[1] <= once[1]
    if hh.PARTS[kind] == 1:
        assert first[0] - created[0] == 4 and once[0] - first[0] == len(LAZY_BLOCKS), (created, first, once)
    else:
        assert once[0] - created[0] <= 4 + len(LAZY_BLOCKS), (created, once)
    assert twice == once, (once, twice)
    assert mem() == base


# ---- 2. the call-order contract -----------------------------------------------------------------------------------------------------------------

WALK_BUSES, WALK_HMAX, WALK_SLOTS, WALK_CALLS = 12, 11, 4, 200


@pytest.fixture(scope="module")
def walk_net(tmp_path_factory):
    import harmonic_power_flow_amd as hp
    from harmonic_power_flow_amd import synth
    fb, fl = synth.gen(WALK_BUSES, seed=0, outdir=str(tmp_path_factory.mktemp("history_walk")))
    st = hp.Settings(H_MAX=WALK_HMAX)
    buses, lines, m, n, c = hp.init_network(fb, fl, settings=st)
    net = dict(st=st, buses=buses, Y=hp.build_admittance_matrices(buses, lines, st.HARMONICS), NE=hp.import_Norton_Equivalents(buses, True, st, INPUTS),
               n=n, Hn=len(st.HARMONICS))
    scale = np.stack([synth.scenario_scale(n, s) for s in range(6)])
    net["P"], net["Q"] = buses["P"].to_numpy(float) * scale, buses["Q"].to_numpy(float) * scale
    rng = np.random.default_rng(11)
    net["ab"] = np.stack([1.0 + 0.05 * rng.uniform(-1, 1, (6, n - m)), 0.02 * rng.uniform(-1, 1, (6, n - m))], axis=2)
    Vm0 = np.full((net["Hn"], n), 0.1)                       # the reference's start, as a start state
    Vm0[0] = 1.0
    net["start"] = (Vm0.reshape(-1), np.zeros(net["Hn"] * n))
    assert n - m > 0
    return net


def _code(fn, *args, **kw):
    from harmonic_power_flow_amd._lib import HpfError
    try:
        fn(*args, **kw)
    except HpfError as e:
        return e.code
    return hc.OK


def alphabet(net):
    """[(label, device(dm, model) -> code of the library, table(model) -> code of the header)]; `device` runs first and may read the model
    (the rows of set_sources(S)), `table` then moves it"""
    P, Q, ab = net["P"], net["Q"], net["ab"]
    A = []
    for k in (1, 3, 4, 5):                                   # 5 > S_max
        A.append(("set_loads(%d)" % k, lambda dm, m, k=k: _code(dm.set_loads, P[:k], Q[:k]), lambda m, k=k: m.set_loads(k)))
        A.append(("set_state(%d)" % k, lambda dm, m, k=k: _code(dm.set_state, None, None, n_scen=k), lambda m, k=k: m.set_state(k)))
    for k in (3, 5):
        A.append(("start_apply(%d)" % k, lambda dm, m, k=k: _code(dm.apply_start, k), lambda m, k=k: m.set_state(k, apply=True)))
    A.append(("set_sources(S)", lambda dm, m: _code(dm.set_sources, ab[:max(m.num_scenarios(), 1)], "scale_shift"),
              lambda m: m.set_sources(max(m.num_scenarios(), 1))))
    A.append(("set_sources(2)", lambda dm, m: _code(dm.set_sources, ab[:2], "scale_shift"), lambda m: m.set_sources(2)))
    A.append(("get_sources", lambda dm, m: _code(dm.get_sources), lambda m: m.read("get_sources")))
    A.append(("clear_sources", lambda dm, m: _code(dm.clear_sources), lambda m: m.clear_sources()))
    A.append(("start_set", lambda dm, m: _code(dm.set_start, *net["start"]), lambda m: m.start_state("set")))
    A.append(("start_capture", lambda dm, m: _code(dm.capture_start, 0), lambda m: m.start_state("capture")))
    A.append(("start_get", lambda dm, m: _code(dm.get_start), lambda m: m.start_state("get")))
    A.append(("start_clear", lambda dm, m: _code(dm.clear_start), lambda m: m.start_state("clear")))
    A.append(("mismatch", lambda dm, m: _code(dm.mismatch), lambda m: m.run("mismatch")))
    A.append(("iterate(1)", lambda dm, m: _code(dm.iterate, 1), lambda m: m.run("iterate")))
    A.append(("fund_pf(1)", lambda dm, m: _code(dm.fund_pf, 1e-6, 1), lambda m: m.run("fund_pf")))

    def solve(dm, m):
        res = []
        code = _code(lambda: res.append(dm.solve(1e-4, 1)))
        m.took_step = bool(res) and res[0][0][0] > 0          # the kept state of a scenario exists if it took a step (hpf.h, hpf_jacobian_last)
        return code
    A.append(("solve(1)", solve, lambda m: m.run("solve")))
    A.append(("get_stats", lambda dm, m: _code(dm.stats), lambda m: m.read("get_stats")))
    A.append(("step_residuals", lambda dm, m: _code(dm.step_residuals), lambda m: m.read("step_residuals")))
    A.append(("jacobian_csr_last", lambda dm, m: _code(dm.jacobian_csr, 0, last=True), lambda m: m.read("jacobian_last")))
    A.append(("branch_flows", lambda dm, m: _code(dm.branch_flows), lambda m: m.read("branch_flows")))
    A.append(("waveform", lambda dm, m: _code(dm.waveform, 64, buses=[0]), lambda m: m.read("waveform")))
    for which, begin in (("distortion", ()), ("branch_stats", ()), ("waveform_stats", (64,))):
        for what, args in (("begin", begin), ("add", (0,)), ("get", ()), ("end", ())):
            A.append((which + "_" + what, lambda dm, m, which=which, what=what, args=args: _code(getattr(dm, which + "_" + what), *args),
                      lambda m, which=which, what=what: m.accum(which, what)))
    A.append(("solve_queue(6)", lambda dm, m: _code(dm.solve_queue, P, Q, max_iter=8), lambda m: m.solve_queue(6)))
    for k in (6, 5):
        A.append(("queue_sources(%d)" % k, lambda dm, m, k=k: _code(dm.queue_sources, ab[:k], "scale_shift"), lambda m, k=k: m.queue_sources(k)))
    for name, values in (("keep_previous_state", (0, 1)), ("step_residual_check", (0, 1)), ("rectangular_update", (0, 1, 2)), ("queue_chunk", (1, 4, 17)),
                         ("scenario_groups", (1, 4, 9)), ("auto_repivot", (0, 1)), ("block_pivoting", (0, 1)), ("no_such_option", (1,))):
        for v in values:
            A.append(("%s=%d" % (name, v), lambda dm, m, name=name, v=v: _code(dm.set_option, name, v), lambda m, name=name, v=v: m.set_option(name, v)))
    return A


# entries no state of the handle accepts: a size beyond S_max, 2 rows (no batch of the alphabet has 2 scenarios), values out of range
NEVER = {"set_loads(5)", "set_state(5)", "start_apply(5)", "set_sources(2)", "rectangular_update=2", "queue_chunk=17", "scenario_groups=9",
         "no_such_option=1"}
PREPARED = {1: ("set_loads(3)", "set_state(3)"),             # how each walk begins: a batch; a solve with the previous state kept; a valid mismatch
            2: ("keep_previous_state=1", "set_loads(3)", "set_state(3)", "solve(1)", "jacobian_csr_last"),
            3: ("step_residual_check=1", "distortion_begin", "set_loads(4)", "set_state(4)", "mismatch")}


def draw_walk(A, seed, calls=WALK_CALLS):
    """the labels of a walk, drawn against the table alone (so it can be replayed without a device).  A uniform draw over 60 entries almost
    never builds loads, state, mismatch, iterate, or solve, begin, add; so the first calls prepare a batch, and then one draw in four is
    uniform over all entries, two are taken among the entries the table would accept in the current state and one among those it would
    refuse -- in both cases among those this walk has not yet had accepted / refused, while there are any"""
    import copy
    rng = np.random.default_rng(seed)
    model, labels, had = hc.Contract(WALK_SLOTS), list(PREPARED[seed]), {(label, hc.OK) for label in PREPARED[seed]}
    by_label = {label: table for label, _, table in A}
    for label in labels:
        by_label[label](model)
    while len(labels) < calls:
        how = int(rng.integers(4))
        pool = A
        if how > 0:
            want = {e[0]: e[2](copy.deepcopy(model)) for e in A}
            pool = [e for e in A if (want[e[0]] == hc.OK) == (how > 1)]
            pool = [e for e in pool if (e[0], want[e[0]]) not in had] or pool
        label = pool[int(rng.integers(len(pool)))][0]
        had.add((label, by_label[label](model)))
        labels.append(label)
    return labels


def test_return_codes_of_three_random_walks_follow_the_header(walk_net):
    """Three seeded walks of 200 calls over every entry point of a batch's life, refused ones included: the library's code and
    hpf_num_scenarios against the table of tests/handle_contract.py after every call.  Across the walks every entry that some state accepts IS
    accepted at least once, and every entry is refused at least once where some state refuses it.  (Every call the table refuses is refused
    by the library on the host, and every call it accepts reads device data an earlier accepted call defined: the guards were read first,
    DESIGN.md 3.15.)"""
    import mixed_batch as mb
    A = alphabet(walk_net)
    by_label = {label: (device, table) for label, device, table in A}
    accepted, refused = set(), set()
    for seed in (1, 2, 3):
        dm = mb.model(walk_net, WALK_SLOTS, "block_tree")
        model = hc.Contract(WALK_SLOTS)
        trail = []
        try:
            for step, label in enumerate(draw_walk(A, seed)):
                device, table = by_label[label]
                trail.append(label)
                got = device(dm, model)
                want = table(model)
                if label == "solve(1)" and got == hc.OK:
                    model.prev = model.prev and model.took_step
                assert got == want and dm.S == model.num_scenarios(), (
                    "walk %d call %d %s: code %d, the header says %d; hpf_num_scenarios %d, the header says %d; after %s"
                    % (seed, step, label, got, want, dm.S, model.num_scenarios(), trail[-15:-1]))
                (accepted if got == hc.OK else refused).add(label)
        finally:
            dm.close()
        print("\nHISTORY walk %d: %d accepted, %d refused entries so far" % (seed, len(accepted), len(refused)))
    every = {label for label, _, _ in A}
    assert accepted == every - NEVER, ("never accepted", sorted(every - NEVER - accepted), "accepted against the list", sorted(accepted & NEVER))
    always = {label for label in every - NEVER if label.split("_")[-1] in ("begin", "end") or "=" in label or
              label.startswith(("set_loads", "clear_sources", "start_set", "start_clear", "queue_sources"))}
    assert refused == every - always, ("never refused", sorted(every - always - refused))


def _prepared(net, bp=0, state=None):
    """a 3-scenario batch on a fresh handle of the walk's feeder -> dm (block_pivoting = bp set first; state: arrays, or the reference's start)"""
    import mixed_batch as mb
    dm = mb.model(net, WALK_SLOTS, "block_tree", (("block_pivoting", bp),))
    dm.set_loads(net["P"][:3], net["Q"][:3])
    if state is None:
        dm.set_state(None, None, n_scen=3)
    else:
        dm.set_state(*state)
    return dm


def test_clear_sources_touches_only_a_batch_that_has_sources(walk_net):
    """hpf_clear_sources with source STORAGE left by an earlier batch or queue, but no sources in the batch: the mismatch stays valid and
    hpf_solve stays the last call (it ended both, depending on storage no caller can see); on a batch with sources it ends both."""
    net = walk_net
    dm = _prepared(net)
    try:
        dm.queue_sources(net["ab"], "scale_shift")
        dm.solve_queue(net["P"], net["Q"], max_iter=8)                       # leaves the queue's source storage behind, and no batch
        dm.set_loads(net["P"][:3], net["Q"][:3])
        dm.set_state(None, None, n_scen=3)
        dm.fund_pf(1e-6, 30)
        dm.solve(1e-4, 50)
        dm.distortion_begin()
        assert _code(dm.get_sources) == hc.E_STATE
        dm.clear_sources()
        assert _code(dm.distortion_add, 0) == hc.OK and dm.distortion_get().counts.sum() == 3
        dm.distortion_end()
        dm.set_sources(net["ab"][:3], "scale_shift")
        dm.set_loads(net["P"][:3], net["Q"][:3])                             # drops the sources, keeps the storage and the state
        dm.mismatch(want_f=False)
        dm.clear_sources()
        assert _code(dm.iterate, 1) == hc.OK
        dm.set_sources(net["ab"][:3], "scale_shift")                         # a batch WITH sources
        dm.mismatch(want_f=False)
        dm.clear_sources()
        assert _code(dm.iterate, 1) == hc.E_STATE
    finally:
        dm.close()


@pytest.mark.parametrize("to", [1, 0])
def test_a_change_of_block_pivoting_ends_the_mismatch(walk_net, to):
    """mismatch in one mode, block_pivoting changed, iterate: refused (the step of the other mode reads the mismatch in another layout, which the
    last hpf_mismatch did not write); after a new mismatch the step equals, bit for bit, the step of a handle that was in that mode from the
    start.  Setting the value it already has ends nothing."""
    net = walk_net
    dm = _prepared(net)
    try:
        dm.fund_pf(1e-6, 30)
        seed = dm.get_state()
    finally:
        dm.close()
    ref = _prepared(net, bp=to, state=seed)
    try:
        ref.mismatch(want_f=False)
        ref.iterate(1)
        ref.sync()
        want = ref.get_state()
    finally:
        ref.close()
    dm = _prepared(net, bp=1 - to, state=seed)
    try:
        dm.mismatch(want_f=False)
        dm.iterate(1)                                                        # (leaves the mismatch valid, and only this mode's image current)
        dm.set_option("block_pivoting", 1 - to)
        assert _code(dm.iterate, 1) == hc.OK                                 # the same value: still valid
        dm.set_option("block_pivoting", to)
        assert _code(dm.iterate, 1) == hc.E_STATE
        dm.set_state(*seed)
        dm.mismatch(want_f=False)
        dm.iterate(1)
        dm.sync()
        got = dm.get_state()
    finally:
        dm.close()
    assert not hh.same({"Vm": got[0], "Va": got[1]}, {"Vm": want[0], "Va": want[1]})
    assert not np.array_equal(got[0], seed[0])


# ---- 3. the Python cache ------------------------------------------------------------------------------------------------------------------------

def _flat(x, pre=""):
    """the numbers of a result of a reference-shaped call -> {name: array}"""
    import pandas as pd
    import scipy.sparse as sp
    if isinstance(x, dict):
        return {k2: v2 for k, v in sorted(x.items()) for k2, v2 in _flat(v, pre + str(k) + ".").items()}
    if isinstance(x, (tuple, list)) and not all(np.isscalar(v) for v in x):
        return {k2: v2 for i, v in enumerate(x) for k2, v2 in _flat(v, pre + str(i) + ".").items()}
    if isinstance(x, pd.DataFrame):
        return {pre + "frame": x.select_dtypes("number").to_numpy(dtype=float)}
    if sp.issparse(x):
        return {pre + "data": x.data, pre + "indices": x.indices, pre + "indptr": x.indptr}
    if x is None or isinstance(x, str):
        return {pre + "text": np.frombuffer(str(x).encode(), dtype=np.uint8)}
    a = np.asarray(x)
    return {pre + "value": a if a.dtype != object else np.frombuffer(repr(x).encode(), dtype=np.uint8)}


def test_reference_shaped_calls_on_cached_handles_equal_uncached_calls(tmp_path):
    """hp.hpf plain, with sources, with the rectangular update, with the step check, on other loads; hp.solve with line flows and waveforms; hp.pf
    -- 18 calls under handle_cache(4): a seeded permutation of the seven variants, nine more seeded draws, and the same variant twice in a row
    at two places.  Every number of every result equals the same call under handle_cache(0), where each call creates and destroys its own
    handle."""
    import harmonic_power_flow_amd as hp
    from harmonic_power_flow_amd import synth
    import mixed_batch as mb
    fb, fl = synth.gen(mb.N_BUS, seed=mb.SEED, outdir=str(tmp_path))
    st = hp.Settings(H_MAX=mb.H_MAX)
    buses, lines, m, n, c = hp.init_network(fb, fl, settings=st)
    Y = hp.build_admittance_matrices(buses, lines, st.HARMONICS)
    other = buses.copy()
    other["P"] = other["P"] * 0.9
    rng = np.random.default_rng(5)
    src = {"scale": 1.0 + 0.05 * rng.uniform(-1, 1, n - m), "shift": 0.02 * rng.uniform(-1, 1, n - m)}

    def call_hpf(b=buses, **kw):
        det = {}
        res = hp.hpf(b, lines, True, settings=st, ne_dir=INPUTS, verbose=False, details=det, **kw)
        return res, {k: det[k] for k in ("err_hist", "stats", "Vm_raw", "Va_raw", "step_eta_max", "solver")}
    variants = {"plain": call_hpf, "sources": lambda: call_hpf(sources=src), "rectangular": lambda: call_hpf(update="rectangular"),
                "check_steps": lambda: call_hpf(check_steps=True), "other_loads": lambda: call_hpf(other),
                "solve": lambda: {k: v for k, v in hp.solve(fb, fl, settings=st, ne_dir=INPUTS, line_flows=True, waveforms=True).items() if k != "details"},
                "pf": lambda: hp.pf(Y, buses, settings=st, verbose=False)}
    size = hp.handle_cache()["size"]
    try:
        hp.close_all()
        hp.handle_cache(0)
        want = {k: _flat(f()) for k, f in variants.items()}
        assert hp.handle_cache()["held"] == 0
        assert hh.same(want["plain"], want["other_loads"]) and hh.same(want["plain"], want["rectangular"]) and hh.same(want["plain"], want["sources"])
        hp.handle_cache(4)
        names = sorted(variants)
        draw = np.random.default_rng(6)                      # (of its own: the order does not depend on the size of `src`)
        order = [names[i] for i in draw.permutation(len(names))] + [names[i] for i in draw.integers(len(names), size=9)]
        order[5:5] = [order[4]]                              # the same variant twice in a row
        order.append(order[-1])
        assert set(order) == set(variants) and len(order) == 18
        before = hp.handle_cache()
        for i, name in enumerate(order):
            bad = hh.same(_flat(variants[name]()), want[name])
            assert not bad, "%s on a cached handle differs from an uncached call in %s after %s" % (name, bad, order[:i])
        after = hp.handle_cache()
        # (at most one handle per model key: the feeder on the block tree, the pf's dense one, and what line flows / waveforms borrow)
        assert after["misses"] - before["misses"] <= 4 and after["hits"] - before["hits"] >= len(order) - 4 and after["held"] >= 1
    finally:
        hp.handle_cache(size)
        hp.close_all()
