"""hpf_solve and hpf_solve_queue on batches in which only SOME scenarios are flagged, repeated, non-finite or already converged (run with
-m gpu on an MI355X) -- the case of a real Monte-Carlo sweep, and the only one in which the repeat mask (k_mark_repeat, k_restore_masked,
k_mask_to_list, the mask branch of k_finalize, the masked nr_pass) is neither all ones nor all zeros.

The compositions come from tests/mixed_batch.py (kinds A, B, C, N; derived from the code, not from measured values).  Every expectation is
either an exact record derived from the stop rule (B, N) or bit identity with a run that takes the other road to the same arithmetic: the
block_pivoting = 1 handle for repeated scenarios, the auto_repivot = 0 handle for scenarios that must be left alone, the scenario alone in a
one-slot handle.  Only the dense handle has a tolerance: 1e-10 on |dU|, the bound tests/test_gpu_parity.py gives to rocSOLVER's batch rounding."""
import numpy as np
import pytest

import mixed_batch as mb

pytestmark = pytest.mark.gpu

LIMIT0 = (("pivot_growth_limit_log10", 0),)
PIVOTED = (("block_pivoting", 1),)


def bits_equal(a, b):
    return np.array_equal(mb.bits(a), mb.bits(b))


def _kinds(S, few, few_kind, rest_kind):
    return "".join(few_kind if s in few else rest_kind for s in range(S))


# S = 5; S = 17: a ragged second tile with holes of the repeat pass at slots 0, 15 and 16; S = 70: two scenario groups with the boundary at
# slot 32 (group_bound), the few working scenarios at 0, 31, 32 and 69 -- and the inverse placement
PLACEMENTS = {"S5": "BAABA", "S17": _kinds(17, (0, 5, 15, 16), "B", "A"), "S70_few": _kinds(70, (0, 31, 32, 69), "A", "B"),
              "S70_inverse": _kinds(70, (0, 31, 32, 69), "B", "A")}
AB17 = PLACEMENTS["S17"]


@pytest.fixture(scope="module")
def radial(tmp_path_factory):
    return mb.feeder(tmp_path_factory.mktemp("mixed_radial"))


@pytest.fixture(scope="module")
def meshed(tmp_path_factory):
    return mb.feeder(tmp_path_factory.mktemp("mixed_meshed"), ties=2)


def _check_A(r, ref, b, what):
    """every A: repeated (bits 3 and 4), converged, the block_pivoting = 1 handle's result bit for bit"""
    for s in mb.where(b, "A"):
        assert (r["stats"]["flags"][s] & ~mb.MODE_BITS) == (1 | 8 | 16), (what, s, r["stats"]["flags"][s])
        assert r["it"][s] >= 1
        mb.assert_same(r, ref, s, what=what)


# ---- 1. hpf_solve, radial block tree ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("place", sorted(PLACEMENTS))
def test_flagged_scenarios_are_repeated_next_to_scenarios_that_never_start(radial, place):
    """1a: A + B at limit 0.  A = the block_pivoting = 1 handle of the same composition bit for bit (there B takes no step either), and = the
    scenario alone in a one-slot handle at limit 0 (the pivoted kernels run one workgroup per scenario); B exactly as the stop rule says."""
    b = mb.compose(radial, PLACEMENTS[place])
    r = mb.run(radial, b, LIMIT0)
    ref = mb.run(radial, b, PIVOTED)
    _check_A(r, ref, b, place)
    for s in mb.where(b, "B"):
        mb.check_B(r, b, s)
        mb.check_B(ref, b, s)
    A = mb.where(b, "A")
    if len(A) > 16:                              # the inverse placements: the scenarios at the tile and group boundaries
        A = [s for s in A if s in (1, 2, 14, 17, 30, 33, 34, 47, 48, 63, 64, 68)]
    alone = mb.run_alone(radial, b, A, LIMIT0)
    for s in A:
        assert (alone[s]["stats"]["flags"][0] & ~mb.MODE_BITS) == (1 | 8 | 16)
        mb.assert_same(r, alone[s], s, 0, what=place + " alone")


@pytest.mark.parametrize("kinds", ["NCNCC", _kinds(17, (0, 7, 15, 16), "N", "C")])
def test_non_finite_scenarios_are_repeated_and_their_neighbours_left_alone(radial, kinds):
    """1b: C + N at the default limit.  Only N is in the repeat mask: C must come out as from a handle that never repeats (auto_repivot = 0),
    in every output; N carries bits 2 and 4 (bit 2 alone without the repeat), no step, the entering state."""
    b = mb.compose(radial, kinds)
    r = mb.run(radial, b)                        # (hpf_solve returned HPF_OK: anything else raises)
    ref = mb.run(radial, b, (("auto_repivot", 0),))
    for s in mb.where(b, "C"):
        assert (r["stats"]["flags"][s] & ~mb.MODE_BITS) == 1, (s, r["stats"]["flags"][s])
        assert r["it"][s] >= 1
        mb.assert_same(r, ref, s, what="C beside N")
    for s in mb.where(b, "N"):
        mb.check_N(r, b, s, repeated=True)
        mb.check_N(ref, b, s, repeated=False)


@pytest.mark.parametrize("max_iter", [0, 1])
def test_max_iter_zero_and_one_on_a_mixed_batch(radial, max_iter):
    """1c: with 0 nobody steps (A: bit 1, B: bit 0); with 1, A takes exactly one step in the pass whose result is returned; B untouched."""
    b = mb.compose(radial, AB17)
    r = mb.run(radial, b, LIMIT0, max_iter=max_iter)
    ref = mb.run(radial, b, PIVOTED, max_iter=max_iter)
    for s in mb.where(b, "B"):
        mb.check_B(r, b, s)
    for s in mb.where(b, "A"):
        assert r["it"][s] == max_iter and r["hist"].shape[1] == max_iter + 1
        assert (r["stats"]["flags"][s] & ~mb.MODE_BITS) == (2 | (8 | 16 if max_iter else 0)), (s, r["stats"]["flags"][s])
        if max_iter == 0:
            mb.assert_untouched(r, b, s)
            assert bits_equal(r["err"][s], r["e0"][s]) and r["e0"][s] > mb.THRESH
        mb.assert_same(r, ref, s, what="max_iter %d" % max_iter)


def test_step_residuals_of_a_mixed_batch(radial):
    """1d: step_residual_check.  eta of A = the block_pivoting = 1 handle's (the eta of repeated scenarios alone starts again), B has none,
    bits 6 / 7 = the verdict on the first pass / on the pass whose result is returned (resid_flag_bits) at the default limit 1e-10."""
    b = mb.compose(radial, AB17)
    check = (("step_residual_check", 1),)
    r = mb.run(radial, b, LIMIT0 + check, eta=True)
    ref = mb.run(radial, b, PIVOTED + check, eta=True)
    first = mb.run(radial, b, LIMIT0 + check + (("auto_repivot", 0),), eta=True)     # the first pass on its own
    for s in mb.where(b, "B"):
        mb.check_B(r, b, s, eta=True)
    for s in mb.where(b, "A"):
        mb.assert_same(r, ref, s, what="residual check")
        assert bits_equal(r["eta_last"][s], ref["eta_last"][s]) and bits_equal(r["eta_max"][s], ref["eta_max"][s]), s
        assert np.isfinite(r["eta_max"][s]) and r["eta_max"][s] >= r["eta_last"][s] >= 0
        want = (1 | 8 | 16) | (64 if not first["eta_max"][s] <= 1e-10 else 0) | (128 if not r["eta_max"][s] <= 1e-10 else 0)
        assert (r["stats"]["flags"][s] & ~mb.MODE_BITS) == want, (s, r["stats"]["flags"][s], want)
    print("\nMIXED 1d: eta_max of A: first pass %.2e, repeat %.2e" % (first["eta_max"][mb.where(b, "A")].max(), r["eta_max"][mb.where(b, "A")].max()))


def test_previous_state_of_a_repeated_scenario(radial):
    """1d: keep_previous_state.  The Jacobian of the last iteration of a repeated scenario is the repeat's (k_keep_prev over the masked list)."""
    b = mb.compose(radial, AB17)
    keep = (("keep_previous_state", 1),)
    A = mb.where(b, "A")
    probe = (int(A[0]), int(A[-1]))
    r = mb.run(radial, b, LIMIT0 + keep, jac_of=probe)
    ref = mb.run(radial, b, PIVOTED + keep, jac_of=probe)
    for s in probe:
        mb.assert_same(r, ref, s, what="keep_previous_state")
        assert r["jac"][s].size > 0 and bits_equal(r["jac"][s], ref["jac"][s]), s


# AB17 with slots 10 and 12 converged as well: the batch whose first pass runs LONGER than its repeat (25 iterations against 24 on the MI355X:
# measured, the test prints both) -- the first pass then has written a trace row that no iteration of the repeat overwrites
AB17_SHORT_REPEAT = _kinds(17, (0, 5, 10, 12, 15, 16), "B", "A")


@pytest.mark.parametrize("kinds", [AB17, AB17_SHORT_REPEAT], ids=["S17", "S17_short_repeat"])
def test_trace_of_a_mixed_batch(radial, kinds):
    """1d: trace.  The whole trace of the batch = the block_pivoting = 1 handle's, rows nobody wrote (NaN) included: no first-pass state is left
    in a repeated scenario's rows, nor in a row beyond the last iteration of the repeat.  B repeats its entering state in every row written."""
    b = mb.compose(radial, kinds)
    r = mb.run(radial, b, LIMIT0, trace=True)
    ref = mb.run(radial, b, PIVOTED, trace=True)
    first = mb.run(radial, b, LIMIT0 + (("auto_repivot", 0),))
    A, B = mb.where(b, "A"), mb.where(b, "B")
    print("\nMIXED 1d: iterations of A: first pass %s, repeat %s" % (first["it"][A].tolist(), r["it"][A].tolist()))
    _check_A(r, ref, b, "trace")
    last = int(r["it"].max())
    assert np.isnan(r["Vt"][:, last + 1:]).all() and np.isnan(r["At"][:, last + 1:]).all(), "rows beyond the last iteration of the returned pass"
    assert np.isfinite(r["Vt"][:, :last + 1]).all()
    np.testing.assert_array_equal(r["Vt"], ref["Vt"])
    np.testing.assert_array_equal(r["At"], ref["At"])
    for s in B:
        for k in range(last + 1):
            assert bits_equal(r["Vt"][s, k], b["Vm"][s]) and bits_equal(r["At"][s, k], b["Va"][s]), (s, k)
    for s in A:
        assert bits_equal(r["Vt"][s, 0], b["Vm"][s]) and bits_equal(r["Vt"][s, r["it"][s]], r["Vm"][s]) and bits_equal(r["Vt"][s, last], r["Vm"][s])


def test_accumulators_after_a_mixed_solve(radial):
    """1d: distortion_add and branch_stats_add after the solve: A and B all converged, nothing skipped or deferred; maxima and args from
    tests/distortion_ref.py and tests/branch_ref.py on the returned voltages."""
    b = mb.compose(radial, AB17)
    dm = mb.model(radial, b["S"], opts=LIMIT0)
    try:
        r = mb.solve_on(dm, b, accum=True)
        arrays = (dm.rowptr, dm.col, dm.Yval)
    finally:
        dm.close()
    ids, flags, n, Hn = np.arange(b["S"]), r["stats"]["flags"], radial["n"], radial["Hn"]
    assert (flags & 1).all()
    mb.check_distortion(r["dist"], r["Vm"], ids, flags, n, Hn, counts=[b["S"], 0, 0])
    mb.check_branches(r["br"], arrays, r["Vm"], r["Va"], ids, flags, n, Hn, counts=[b["S"], 0, 0])


def _separating(dm, b, option, values, bit):
    """the first value of `option` at which the flagged set (record bit `bit`, nothing repeated) is a proper non-empty subset -> (value, set)"""
    seen = {}
    for v in values:
        dm.set_option(option, v)
        flagged = np.nonzero(mb.solve_on(dm, b)["stats"]["flags"] & bit)[0].tolist()
        seen[v] = flagged
        if 0 < len(flagged) < b["S"]:
            print("\nMIXED 1e: %s = %d separates: flagged %s of %d (tried %s)" % (option, v, flagged, b["S"], seen))
            return v, flagged
    print("\nMIXED 1e: no value of %s separates: %s" % (option, seen))
    return None, None


def test_flagged_and_unflagged_scenarios_in_one_batch(radial):
    """1e: A + C in ONE batch -- a limit that flags some scenarios and not others, searched here over the integer options (the growth values of
    a feeder cannot be derived): pivot_growth_limit_log10 0..10, and step_residual_limit_log10 -16..-10 with the residual check on.  The
    scenarios are spread on purpose (load levels 0.6 .. 1.3, entering states after 0 .. 3 default iterations).  With the value found and the
    repeat on: flagged = the block_pivoting = 1 handle of the same composition, unflagged = the auto_repivot = 0 run, both bit for bit.
    The same runs with trace: no scenario's rows hold states of a pass its result does not come from."""
    S = 8
    b = mb.compose(radial, "C" * S, iters=[s % 4 for s in range(S)], gscale=[0.6 + 0.1 * s for s in range(S)])
    found = []
    for base, option, values, bit in (((), "pivot_growth_limit_log10", range(0, 11), 8),
                                      ((("step_residual_check", 1),), "step_residual_limit_log10", range(-16, -9), 64)):
        dm = mb.model(radial, S, opts=base + (("auto_repivot", 0),))
        try:
            v, flagged = _separating(dm, b, option, values, bit)
        finally:
            dm.close()
        if v is not None:
            found.append((base + ((option, v),), flagged, bit))
    assert found, "neither knob separates the scenarios of this batch"
    for opts, flagged, bit in found:
        eta = bit == 64
        r = mb.run(radial, b, opts, eta=eta)
        piv = mb.run(radial, b, PIVOTED + opts, eta=eta)
        static = mb.run(radial, b, opts + (("auto_repivot", 0),), eta=eta)
        assert np.nonzero(static["stats"]["flags"] & bit)[0].tolist() == flagged
        for s in range(S):
            rep = s in flagged
            assert bool(r["stats"]["flags"][s] & 16) == rep and bool(r["stats"]["flags"][s] & bit) == rep, (opts, s, r["stats"]["flags"][s])
            mb.assert_same(r, piv if rep else static, s, what="1e %s %s" % (opts[-1], "repeated" if rep else "left alone"))
            if eta:
                other = piv if rep else static
                assert bits_equal(r["eta_last"][s], other["eta_last"][s]) and bits_equal(r["eta_max"][s], other["eta_max"][s]), (opts, s)
            if not rep:
                assert r["stats"]["flags"][s] == static["stats"]["flags"][s]
        # the trace of such a batch: every scenario's rows are those of the pass its result comes from, then its final state up to the last
        # iteration any returned result took; nothing beyond
        rt, pt, st = (mb.run(radial, b, o, trace=True) for o in (opts, PIVOTED + opts, opts + (("auto_repivot", 0),)))
        last = int(rt["it"].max())
        assert np.isnan(rt["Vt"][:, last + 1:]).all() and np.isnan(rt["At"][:, last + 1:]).all(), opts
        for s in range(S):
            other, k = (pt if s in flagged else st), int(rt["it"][s])
            mb.assert_same(rt, r, s, what="traced solve")
            for key in ("Vt", "At"):
                assert bits_equal(rt[key][s, :k + 1], other[key][s, :k + 1]), (opts, key, s, "flagged" if s in flagged else "left alone")
                assert bits_equal(rt[key][s, k:last + 1], np.broadcast_to(rt[key][s, k], (last + 1 - k, rt[key].shape[2]))), (opts, key, s)


# ---- 2. meshed and dense handles ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kinds", ["BAABA", "NBANB"])
def test_meshed_handle_reports_and_walks_past_holes(meshed, kinds):
    """The factor-once bordered step has no repeat: A is reported with bit 3 at limit 0, and every stepping scenario equals the same scenario
    alone from the same entering state bit for bit (the host walks the running scenarios: holes at slot 0).  B and N as everywhere."""
    b = mb.compose(meshed, kinds)
    dm = mb.model(meshed, b["S"], opts=LIMIT0)
    try:
        assert dm.tree_census()["ties"] == 2
        r = mb.solve_on(dm, b)
    finally:
        dm.close()
    A = mb.where(b, "A")
    alone = mb.run_alone(meshed, b, A, LIMIT0)
    for s in A:
        assert (r["stats"]["flags"][s] & ~mb.MODE_BITS) == (1 | 8), (s, r["stats"]["flags"][s])
        assert r["it"][s] >= 1
        mb.assert_same(r, alone[s], s, 0, what="meshed alone")
    for s in mb.where(b, "B"):
        mb.check_B(r, b, s)
    for s in mb.where(b, "N"):
        mb.check_N(r, b, s, repeated=False)


@pytest.mark.parametrize("kinds", ["BAABA", "NBANB"])
def test_dense_handle_neighbours_of_holes(radial, kinds):
    """rocSOLVER's batch with matrices nobody assembled (B, N) in it: the neighbours match the batch in which those slots hold an ordinary
    scenario -- n_iter equal, |dU| <= 1e-10 -- and no HPF_E_SINGULAR comes back (it would raise)."""
    b = mb.compose(radial, kinds)
    plain = mb.compose(radial, "A" * len(kinds))
    r = mb.run(radial, b, solver="dense")
    ref = mb.run(radial, plain, solver="dense")
    worst = 0.0
    for s in mb.where(b, "A"):
        assert (r["stats"]["flags"][s] & ~mb.MODE_BITS) == 1 and r["it"][s] == ref["it"][s] >= 1, (s, r["it"][s], ref["it"][s])
        worst = max(worst, float(np.abs(r["Vm"][s] * np.exp(1j * r["Va"][s]) - ref["Vm"][s] * np.exp(1j * ref["Va"][s])).max()))
    print("\nMIXED dense %s: worst |dU| of a stepping neighbour %.3e" % (kinds, worst))
    assert worst <= 1e-10
    for s in mb.where(b, "B"):
        mb.check_B(r, b, s)
    for s in mb.where(b, "N"):
        mb.check_N(r, b, s, repeated=False)


# ---- 3. hpf_solve_queue, radial, with a start state -----------------------------------------------------------------------------------------------

QUEUE = "PAPAAPNAPAPA"              # P: the base loads (converged at the start state), A: scaled loads (step, flagged at limit 0), N: NaN load


def _queue_input(net):
    from harmonic_power_flow_amd import synth
    if "queue" in net["cache"]:
        return net["cache"]["queue"]
    n = net["n"]
    k = np.array(list(QUEUE))
    scale = np.stack([np.ones(n) if c != "A" else synth.scenario_scale(n, g) for g, c in enumerate(k)])
    P, Q = net["P0"] * scale, net["Q0"] * scale
    dm = mb.model(net, 1)
    try:
        dm.set_loads(net["P0"], net["Q0"])
        dm.set_state(None, None, n_scen=1)
        dm.fund_pf(1e-6, 30)
        _, err, _ = dm.solve(mb.THRESH, mb.MAX_ITER)
        assert err[0] <= mb.THRESH
        dm.mismatch(want_f=False)
        dm.iterate(2)
        dm.sync()
        Vm0, Va0 = dm.get_state()
        P[k == "N", mb.nan_bus(net, dm.m)] = np.nan
    finally:
        dm.close()
    net["cache"]["queue"] = (k, P, Q, Vm0[0].copy(), Va0[0].copy())
    return net["cache"]["queue"]


def _queue(net, slots, P, Q, start):
    dm = mb.model(net, slots, opts=LIMIT0)
    try:
        dm.set_start(*start)
        dm.distortion_begin()
        dm.branch_stats_begin()
        rec, Vm, Va = dm.solve_queue(P, Q, want_voltages=True)
        return rec, Vm, Va, dm.distortion_get(), dm.branch_stats_get()
    finally:
        dm.close()


@pytest.mark.parametrize("slots", [3, 8])
def test_queue_with_slots_that_free_at_once_beside_slots_that_run(radial, slots):
    """hpf_solve_queue from a start state at limit 0: base-load rows converge at iteration 0 and free their slot at once, scaled rows step
    and are reported (bit 3, never bit 4), the NaN row is reported with bit 2 -- every record and voltage as from a one-slot handle; the
    accumulators add the base rows and defer the rest.  Then the sweep: the reported rows re-solved from the start state, each added once."""
    from harmonic_power_flow_amd import sweep
    net = radial
    k, P, Q, Vm0, Va0 = _queue_input(net)
    n, Hn, G = net["n"], net["Hn"], len(k)
    base, flg, nan = (np.nonzero(k == c)[0] for c in "PAN")
    rec, Vm, Va, dist, br = _queue(net, slots, P, Q, (Vm0, Va0))
    for g in base:
        assert rec["n_iter"][g] == 0 and rec["flags"][g] == (1 | 256), (g, rec[g])
        assert bits_equal(Vm[g], Vm0) and bits_equal(Va[g], Va0), g
    for g in flg:
        assert rec["n_iter"][g] >= 1 and (rec["flags"][g] & (8 | 16 | 256)) == (8 | 256), (g, rec[g])
    for g in nan:
        assert rec["n_iter"][g] == 0 and (rec["flags"][g] & (1 | 4 | 16)) == 4 and np.isnan(rec["err"][g]), (g, rec[g])
        assert bits_equal(Vm[g], Vm0) and bits_equal(Va[g], Va0), g
    one = _queue(net, 1, P, Q, (Vm0, Va0))
    assert np.array_equal(rec.view(np.uint8), one[0].view(np.uint8)) and bits_equal(Vm, one[1]) and bits_equal(Va, one[2])
    counts = [len(base), 0, len(flg) + len(nan)]
    assert dist.counts.tolist() == counts and br.counts.tolist() == counts, (dist.counts, br.counts, counts)
    assert np.isin(dist.thd_arg, base).all() and np.isin(br.irms_arg, base).all()

    dm = mb.model(net, slots, opts=LIMIT0)
    try:
        srec, sVm, sVa, sdist, sbr = sweep.solve_scenarios(dm, P, Q, want_voltages=True, distortion={}, branches={}, start=(Vm0, Va0))
        arrays = (dm.rowptr, dm.col, dm.Yval)
    finally:
        dm.close()
    dm = mb.model(net, 1, opts=LIMIT0)
    try:
        dm.set_start(Vm0, Va0)
        for g in flg:
            dm.apply_start(1)
            dm.set_loads(P[g], Q[g])
            it1, err1, _ = dm.solve(mb.THRESH, mb.MAX_ITER)
            st1 = dm.stats()
            Vm1, Va1 = dm.get_state()
            assert (st1["flags"][0] & (1 | 8 | 16 | 256)) == (1 | 8 | 16 | 256), (g, st1)
            for f in ("n_iter", "flags"):
                assert srec[f][g] == st1[f][0], (g, f, srec[g], st1)
            assert bits_equal(srec["err"][g], st1["err"][0]) and bits_equal(srec["thd_max"][g], st1["thd_max"][0]), (g, srec[g], st1)
            assert bits_equal(sVm[g], Vm1[0]) and bits_equal(sVa[g], Va1[0]), g
    finally:
        dm.close()
    assert np.array_equal(srec[base].view(np.uint8), rec[base].view(np.uint8)) and bits_equal(sVm[base], Vm[base])
    assert ((srec["flags"][nan] & (1 | 4)) == 4).all()
    resolved = len(flg) + len(nan)
    for c in (sdist.counts, sbr.counts):
        assert c[0] + c[1] == G and c[0] == len(base) + len(flg) and c[2] >= resolved, (c, G)
    assert not np.isin(sdist.thd_arg, nan).any() and not np.isin(sdist.x_arg, nan).any() and not np.isin(sbr.irms_arg, nan).any()
    mb.check_distortion(sdist, sVm, np.arange(G), srec["flags"], n, Hn)
    mb.check_branches(sbr, arrays, sVm, sVa, np.arange(G), srec["flags"], n, Hn)
