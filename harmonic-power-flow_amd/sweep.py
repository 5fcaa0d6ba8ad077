"""Scenario sweeps across GPUs: one process per GPU, scenarios dealt round-robin, NO collective on the data path —
independent feeders / Monte-Carlo load cases share nothing during the NR loop.  The only exchange
is one all-gather of the 24-byte per-scenario records (`hpf_stat`: n_iter, flags, err, thd_max) at the end of a
sweep (`torch.distributed`, backend "nccl" = RCCL on ROCm; "gloo" in the CPU tests)."""
import numpy as np

STAT_DTYPE = np.dtype([("n_iter", "<i4"), ("flags", "<i4"), ("err", "<f8"), ("thd_max", "<f8")])
assert STAT_DTYPE.itemsize == 24


def scenario_ids(rank, world, per_rank):
    """Round-robin deal: iteration counts differ per scenario, interleaving balances the ranks."""
    return rank + world * np.arange(per_rank)


def gather_stats(rec, world):
    """rec: uint8 tensor [S_local, 24] on this rank's device -> uint8 tensor [S_local*world, 24] ordered by global
    scenario id (id = rank + world*i)."""
    if world == 1:
        return rec
    import torch
    import torch.distributed as dist
    parts = [torch.empty_like(rec) for _ in range(world)]
    dist.all_gather(parts, rec.contiguous())
    return torch.stack(parts, dim=1).reshape(-1, rec.shape[1])


class _SweepStats:
    """What the statistics containers of the three device accumulators share: plain NumPy arrays, per quantity `pre` of
    QUANTITIES the five arrays pre_max / pre_arg / pre_sum / pre_sumsq (/ pre_over) of the device's statistic slot.  A subclass names its ARRAYS
    and DTYPES (the order is the order of the C call and of pack()), its QUANTITIES, and supplies _settings() -- what two accumulators must have
    been opened with alike to be merged -- and _same(**arrays): a container with this one's settings."""

    @property
    def added(self):
        return int(self.counts[0])

    def _mean(self, what):
        with np.errstate(invalid="ignore", divide="ignore"):
            return getattr(self, what + "_sum") / self.added

    def _std(self, what):
        m = self._mean(what)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.sqrt(np.maximum(getattr(self, what + "_sumsq") / self.added - m * m, 0.0))

    def _worst(self, v, what, k):
        order = np.argsort(-v, kind="stable")[:k]
        return [(int(i), int(getattr(self, what + "_arg")[i]), float(v[i])) for i in order]

    def merge(self, other):
        """Statistics of the union of two disjoint sets of scenarios (another GPU's share, another piece of a sweep): max with the smaller-id
        tie rule, integer adds, float adds.  Refuses different settings (limits, harmonics, samples, bins) or shapes with ValueError."""
        if (type(other) is not type(self) or any(getattr(self, name).shape != getattr(other, name).shape for name in self.ARRAYS) or
                not all(np.array_equal(a, b) for a, b in zip(self._settings(), other._settings()))):
            raise ValueError("%s.merge: the two accumulators were opened with different settings or shapes" % type(self).__name__)
        out = {}
        for pre in self.QUANTITIES:
            ma, aa, mb, ab = (getattr(o, pre + f) for o in (self, other) for f in ("_max", "_arg"))
            take = (ab >= 0) & ((aa < 0) | (mb > ma) | ((mb == ma) & (ab < aa)))
            out[pre + "_max"], out[pre + "_arg"] = np.where(take, mb, ma), np.where(take, ab, aa)
        for name in self.ARRAYS:                             # counts, sums, sums of squares, over, histogram
            if name not in out:
                out[name] = getattr(self, name) + getattr(other, name)
        return self._same(**out)

    def with_ids(self, ids):
        """The same statistics with every scenario id k in the arg arrays replaced by ids[k] (-1 stays)."""
        ids = np.asarray(ids)
        out = {name: getattr(self, name) for name in self.ARRAYS}
        for pre in self.QUANTITIES:
            a = out[pre + "_arg"]
            out[pre + "_arg"] = np.where(a >= 0, ids[np.maximum(a, 0)], -1)
        return self._same(**out)

    def pack(self):
        """-> one uint8 array holding every array (the payload of the gather_* functions)."""
        return np.concatenate([getattr(self, name).reshape(-1).view(np.uint8) for name in self.ARRAYS])

    def unpack(self, raw):
        """A container with this one's settings and shapes and the arrays of `raw` (what pack() of a peer produced)."""
        raw = np.ascontiguousarray(raw, dtype=np.uint8)
        out, o = {}, 0
        for name in self.ARRAYS:
            a = getattr(self, name)
            out[name] = raw[o:o + a.nbytes].view(a.dtype).reshape(a.shape).copy()
            o += a.nbytes
        assert o == raw.size
        return self._same(**out)


class DistortionStats(_SweepStats):
    """Per-bus / per-harmonic distortion statistics of a sweep, as the device accumulated them (hpf_distortion_*, include/hpf.h) -- a plain
    container of NumPy arrays.  x [Hn][n]: the fundamental magnitude |V_1| (p.u.) at harmonic position 0, the individual harmonic distortion
    |V_h| / |V_1| above; thd [n]: THD_F per bus.
    counts [3] int64: scenarios added, skipped (not converged, or a non-finite THD), deferred (reported by the queue, added by their re-solve);
    x_max / x_arg, thd_max / thd_arg: largest value and the scenario id it came from (ties: the smallest id; -1: nothing added);
    x_sum / x_sumsq, thd_sum / thd_sumsq: sums over the added scenarios; x_over / thd_over: scenarios above `limit[q]` / `thd_limit`;
    thd_hist [n][bins + 1]: `bins` uniform bins on [0, hist_max), the last one counts thd >= hist_max (merge adds it)."""
    ARRAYS = ("counts", "x_max", "x_arg", "x_sum", "x_sumsq", "x_over", "thd_max", "thd_arg", "thd_sum", "thd_sumsq", "thd_over", "thd_hist")
    DTYPES = (np.int64, np.float64, np.int32, np.float64, np.float64, np.uint32, np.float64, np.int32, np.float64, np.float64, np.uint32,
              np.uint32)
    QUANTITIES = ("x", "thd")

    def __init__(self, harmonics, limit, thd_limit, hist_max, **arrays):
        self.harmonics = list(harmonics)
        self.limit = np.full(len(self.harmonics), np.inf) if limit is None else np.array(limit, dtype=np.float64)
        self.thd_limit, self.hist_max = float(thd_limit), float(hist_max)
        for name, dt in zip(self.ARRAYS, self.DTYPES):
            setattr(self, name, np.ascontiguousarray(arrays[name], dtype=dt))
        assert self.x_max.ndim == 2 and self.x_max.shape[0] == len(self.harmonics) and self.thd_hist.shape[0] == self.x_max.shape[1]

    def _settings(self):
        return self.harmonics, self.limit, self.thd_limit, self.hist_max

    def _same(self, **arrays):
        return DistortionStats(self.harmonics, self.limit, self.thd_limit, self.hist_max, **arrays)

    @property
    def bins(self):
        return self.thd_hist.shape[1] - 1

    def mean(self):
        """-> (mean of x [Hn][n], mean of thd [n]) over the added scenarios (NaN when nothing was added)."""
        return self._mean("x"), self._mean("thd")

    def std(self):
        """-> (population standard deviation of x [Hn][n], of thd [n]) from sum and sum of squares."""
        return self._std("x"), self._std("thd")

    def thd_percentile(self, p):
        """Per bus [n]: an UPPER BOUND of the p-th percentile of THD over the added scenarios, from the histogram -- the upper edge of the bin
        that holds the sample np.percentile(..., method="higher") would return (sorted sample number ceil(p/100 (added - 1)) + 1), so it
        exceeds that sample by at most one bin width hist_max / bins; inf when the sample sits in the overflow bin (thd >= hist_max).
        Conservative by construction: a limit check against it never passes a bus the exact percentile would fail."""
        if self.added < 1:
            return np.full(self.thd_hist.shape[0], np.nan)
        rank = int(np.ceil((self.added - 1) * (p / 100.0))) + 1
        b = (np.cumsum(self.thd_hist.astype(np.int64), axis=1) >= rank).argmax(axis=1)
        edges = np.append((np.arange(self.bins) + 1) * (self.hist_max / self.bins), np.inf)
        return edges[b]

    def worst(self, k=1):
        """The k buses with the largest thd_max -> list of (bus, scenario id, value), largest first."""
        return self._worst(self.thd_max, "thd", k)


def _gather_merge(stats, world, ids):
    """ids applied on the host, one all_gather of stats.pack(), unpack + merge in rank order (any _SweepStats)."""
    if ids is not None:
        stats = stats.with_ids(ids)
    if world == 1:
        return stats
    import torch
    import torch.distributed as dist
    mine = torch.from_numpy(stats.pack())
    backend = dist.get_backend()
    if backend == "nccl":
        mine = mine.cuda()
    parts = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(parts, mine)
    out = None
    for p in parts:
        s = stats.unpack(p.cpu().numpy())
        out = s if out is None else out.merge(s)
    return out


def gather_distortion(stats, world, ids=None):
    """Distortion statistics of a multi-GPU sweep.  The device numbers the scenarios of a rank locally (`distortion_id_base` + index in the call,
    `first_id` + s); `ids[k]` = global id of local scenario k (`scenario_ids(rank, world, per_rank)`) is applied to x_arg / thd_arg on the host
    first, then ONE all_gather of the packed arrays (a few hundred KB per rank) and a merge in rank order -- every rank returns the same
    statistics, bit for bit.  world == 1 returns its argument (ids applied), like gather_stats.  Every rank must have opened its accumulator
    with the same settings."""
    return _gather_merge(stats, world, ids)


class BranchStats(_SweepStats):
    """Per-branch statistics of a sweep, as the device accumulated them (hpf_branch_stats_*, include/hpf.h) -- a plain container of NumPy arrays
    [nb] over the branches of the handle (DeviceModel.branches()).  Three quantities per scenario and branch: irms (RMS current over all harmonics,
    p.u.: the thermal loading), loss (series loss over all harmonics) and lossh (the harmonics' share, q >= 1).
    counts [3] int64: scenarios added, skipped, deferred (the rules of DistortionStats); x_max / x_arg: largest value and the scenario id it came
    from (ties: the smallest id; -1: nothing added); x_sum / x_sumsq: sums over the added scenarios; irms_over: scenarios with irms above
    `rating[e]` (strictly)."""
    ARRAYS = ("counts", "irms_max", "irms_arg", "irms_sum", "irms_sumsq", "irms_over", "loss_max", "loss_arg", "loss_sum", "loss_sumsq",
              "lossh_max", "lossh_arg", "lossh_sum", "lossh_sumsq")
    DTYPES = (np.int64, np.float64, np.int32, np.float64, np.float64, np.uint32, np.float64, np.int32, np.float64, np.float64,
              np.float64, np.int32, np.float64, np.float64)
    QUANTITIES = ("irms", "loss", "lossh")

    def __init__(self, rating, **arrays):
        for name, dt in zip(self.ARRAYS, self.DTYPES):
            setattr(self, name, np.ascontiguousarray(arrays[name], dtype=dt))
        nb = self.irms_max.shape[0]
        self.rating = np.full(nb, np.inf) if rating is None else np.array(rating, dtype=np.float64)
        assert self.counts.shape == (3,) and self.rating.shape == (nb,) and all(getattr(self, a).shape == (nb,) for a in self.ARRAYS[1:])

    def _settings(self):
        return (self.rating,)

    def _same(self, **arrays):
        return BranchStats(self.rating, **arrays)

    def mean(self, what="irms"):
        """-> mean [nb] of irms / loss / lossh over the added scenarios (NaN when nothing was added)."""
        return self._mean(what)

    def std(self, what="irms"):
        """-> population standard deviation [nb] from sum and sum of squares."""
        return self._std(what)

    def worst(self, k=1, what="irms", relative=False):
        """The k branches with the largest maximum of `what` (relative=True: of irms_max / rating) -> list of (branch, scenario id, value),
        largest first."""
        v = getattr(self, what + "_max")
        if relative:
            with np.errstate(invalid="ignore", divide="ignore"):
                v = np.where(np.isfinite(self.rating), v / self.rating, 0.0)
        return self._worst(v, what, k)


def gather_branch_stats(stats, world, ids=None):
    """Branch statistics of a multi-GPU sweep, like gather_distortion: `ids[k]` = global id of local scenario k is applied to the arg arrays on the
    host, then ONE all_gather of the packed arrays (108 bytes per branch and rank) and a merge in rank order -- every rank returns the same
    statistics, bit for bit.  world == 1 returns its argument (ids applied).  Every rank must have opened its accumulator with the same ratings."""
    return _gather_merge(stats, world, ids)


class WaveformStats(_SweepStats):
    """Per-bus statistics of the voltage waveforms of a sweep, as the device accumulated them (hpf_waveform_stats_*, include/hpf.h) -- a plain
    container of NumPy arrays [n] over the buses.  Two quantities per scenario and bus: peak (largest |v(t)| over the `samples` samples of one
    fundamental period, p.u. of the nominal peak voltage) and crest (peak / rms; sqrt 2 for a pure sine).
    counts [3] int64: scenarios added, skipped, deferred (the rules of DistortionStats); x_max / x_arg: largest value and the scenario id it came
    from (ties: the smallest id; -1: nothing added); x_sum / x_sumsq: sums over the added scenarios; peak_over / crest_over: scenarios strictly
    above `peak_limit[i]` / `crest_limit`."""
    ARRAYS = ("counts", "peak_max", "peak_arg", "peak_sum", "peak_sumsq", "peak_over", "crest_max", "crest_arg", "crest_sum", "crest_sumsq",
              "crest_over")
    DTYPES = (np.int64, np.float64, np.int32, np.float64, np.float64, np.uint32, np.float64, np.int32, np.float64, np.float64, np.uint32)
    QUANTITIES = ("peak", "crest")

    def __init__(self, samples, peak_limit, crest_limit, **arrays):
        for name, dt in zip(self.ARRAYS, self.DTYPES):
            setattr(self, name, np.ascontiguousarray(arrays[name], dtype=dt))
        n = self.peak_max.shape[0]
        self.samples, self.crest_limit = int(samples), float(crest_limit)
        self.peak_limit = np.full(n, np.inf) if peak_limit is None else np.array(peak_limit, dtype=np.float64)
        assert self.counts.shape == (3,) and self.peak_limit.shape == (n,) and all(getattr(self, a).shape == (n,) for a in self.ARRAYS[1:])

    def _settings(self):
        return self.samples, self.peak_limit, self.crest_limit

    def _same(self, **arrays):
        return WaveformStats(self.samples, self.peak_limit, self.crest_limit, **arrays)

    def mean(self, what="peak"):
        """-> mean [n] of peak / crest over the added scenarios (NaN when nothing was added)."""
        return self._mean(what)

    def std(self, what="peak"):
        """-> population standard deviation [n] from sum and sum of squares."""
        return self._std(what)

    def worst(self, k=1, what="peak"):
        """The k buses with the largest maximum of `what` -> list of (bus, scenario id, value), largest first."""
        return self._worst(getattr(self, what + "_max"), what, k)


def gather_waveform_stats(stats, world, ids=None):
    """Waveform statistics of a multi-GPU sweep, like gather_distortion: `ids[k]` = global id of local scenario k is applied to the arg arrays on
    the host, then ONE all_gather of the packed arrays (64 bytes per bus and rank) and a merge in rank order -- every rank returns the same
    statistics, bit for bit.  world == 1 returns its argument (ids applied).  Every rank must have opened its accumulator with the same settings."""
    return _gather_merge(stats, world, ids)


def source_currents(I_N_bus, scale, shift, orders, cs=None):
    """Host expansion of the scale-and-shift form of the source currents (include/hpf.h "Source currents", csrc/hpf_sources.hpp):
    I_src[..., b, q] = (scale[..., b] e^(j orders[q] shift[..., b])) I_N_bus[b, q] -- scale units of the device of nonlinear bus b, their waveform
    shifted in time by shift rad at the fundamental.  I_N_bus [n-m][Hn] complex (the model's I_N of every nonlinear bus's device), scale / shift
    [..., n-m], orders [Hn] -> [..., n-m][Hn] complex.  Written with real-array operations in the device's order -- ang = h * phi; w = (a cos, a sin);
    (w.re in.re - w.im in.im, w.re in.im + w.im in.re) -- so that every product and sum is rounded on its own (a complex array multiply would be
    free to fuse).  cs = (cos, sin) [..., n-m][Hn]: taken instead of numpy's own values of ang (tests: two implementations bit for bit)."""
    I_N_bus = np.asarray(I_N_bus, dtype=np.complex128)
    a = np.asarray(scale, dtype=np.float64)[..., None]
    phi = np.asarray(shift, dtype=np.float64)[..., None]
    if cs is None:
        ang = np.asarray(orders).astype(np.float64) * phi
        c, sn = np.cos(ang), np.sin(ang)
    else:
        c, sn = (np.asarray(x, dtype=np.float64) for x in cs)
    wre, wim = a * c, a * sn
    inr, ini = I_N_bus.real, I_N_bus.imag
    out = np.empty(np.broadcast(wre, inr).shape, dtype=np.complex128)
    out.real = wre * inr - wim * ini
    out.imag = wre * ini + wim * inr
    return out


def sources_argument(sources, n_scen, nnl, Hn, where="solve_scenarios"):
    """The `sources` dict of solve_scenarios / hpf -> None, or (form, array) as DeviceModel.set_sources takes them: {"currents": [n_scen][n-m][Hn]}
    -> ("currents", complex array); {"scale": [n_scen][n-m], "shift": [n_scen][n-m]} (either may be missing: 1 / 0) -> ("scale_shift",
    [n_scen][n-m][2]).  ValueError for anything else, on the host."""
    if sources is None:
        return None
    if not isinstance(sources, dict) or not sources or not (set(sources) <= {"currents"} or set(sources) <= {"scale", "shift"}):
        raise ValueError("%s: sources=%r ({'currents': ..} or {'scale': .., 'shift': ..})" % (where, sources))
    if "currents" in sources:
        a = np.asarray(sources["currents"], dtype=np.complex128)
        if a.shape != (n_scen, nnl, Hn):
            raise ValueError("%s: sources['currents'] must be [%d][%d][%d], got %s" % (where, n_scen, nnl, Hn, a.shape))
        return "currents", np.ascontiguousarray(a)
    ab = np.empty((n_scen, nnl, 2))
    for k, (name, default) in enumerate((("scale", 1.0), ("shift", 0.0))):
        v = np.asarray(sources.get(name, default), dtype=np.float64)
        if name in sources and v.shape != (n_scen, nnl):
            raise ValueError("%s: sources[%r] must be [%d][%d], got %s" % (where, name, n_scen, nnl, v.shape))
        ab[:, :, k] = v
    return "scale_shift", ab


def solve_scenarios(dm, P, Q, thresh_f=1e-6, max_iter_f=30, thresh_h=1e-4, max_iter_h=50, want_voltages=False, refill=True, distortion=None,
                    branches=None, start=None, update="polar", sources=None, waveform=None):
    """Monte-Carlo / what-if sweep on ONE GPU: every row of P, Q [n_scen][n] (p.u. loads, HG:197,372) is one scenario of the
    network `dm` (a DeviceModel) holds -- the reference's counterpart is one hpf() call per load case (HG:511).  Per scenario:
    reference start (HG:174-184), fundamental pf (HG:244), harmonic NR with the reference's stop rule (HG:536).
    refill=True (default): `hpf_solve_queue` -- the `dm.S_max` slots of the model stay full: scenarios that meet the stop rule are
    harvested between chunks of Newton iterations and their slots take the next pending scenarios, so a sweep of many more scenarios
    than slots runs at the lock-step rate of a full handle instead of paying every wave's convergence tail (size the model for as
    many live scenarios as fit: 72 MB of solver state per scenario of the 1 000-bus x 25-harmonic feeder; larger batches amortise the
    latency-bound upper tree levels).  A scenario the static-pivot monitor flags (flags bit 3), whose mismatch turned non-finite in the
    static-pivot kernels (bit 2), or whose step missed the residual check (bit 6, option "step_residual_check"), is solved again on its own through
    `hpf_solve`, which repeats exactly those with partial pivoting on a radial block-tree handle; a meshed handle has no pivoted repeat (its re-solve
    runs the same static-pivot step again), a dense handle pivots in every solve.
    refill=False: fixed waves of up to S_max scenarios (each through fund_pf + solve).
    -> structured array of per-scenario records (n_iter, flags, err, thd_max: the 24-byte record of the multi-GPU gather)
    [+ raw Vm, Va [n_scen][Hn*n]]; every record and voltage is bit-identical to the scenario solved alone.
    distortion: None (default), or a dict {"limit": [Hn] or None, "thd_limit": x, "hist_max": x, "bins": 1..256} (missing keys: no limits,
    hist_max 1.0, 64 bins): the handle's distortion accumulator is opened for the sweep, every converged scenario is folded in on the device
    under its row number in P (queue pieces through "distortion_id_base", re-solved flagged scenarios and the waves of refill=False through
    distortion_add), and the DistortionStats are returned as an additional last element; records and voltages are unchanged.
    branches: None (default), or a dict {"rating": [nb] or None}: likewise for the handle's branch statistics (hpf_branch_stats_*: per line
    the RMS current over all harmonics against its rating, series loss, harmonic loss); the BranchStats are returned as a further last element,
    after the DistortionStats when both are asked for.
    waveform: None (default), or a dict {"samples": T, "peak_limit": [n] or None, "crest_limit": x} (missing keys: 1024 samples, no limits):
    likewise for the handle's waveform statistics (hpf_waveform_stats_*: per bus the peak of the time-domain voltage over one fundamental
    period and its crest factor, the quantities that depend on the harmonics' phase angles); the WaveformStats are returned as a further last
    element, after the DistortionStats and the BranchStats.
    start: None (default): the reference's flat start + pf for every scenario, today's behaviour bit for bit (a handle on which the caller
    has set a start state of its own is refused with ValueError: clear it, or pass it as `start`).  Otherwise a WARM START -- every
    scenario begins at one solved state of the feeder (the handle's start state, hpf_start_*), the pf phase is skipped (thresh_f / max_iter_f
    then only serve cold re-solves), and the harmonic NR of a Monte-Carlo sweep around a base case needs 2 - 3 iterations instead of 20 - 30
    (DESIGN.md 6.3).  A pair (Vm0, Va0) [Hn*n] (raw, as get_state returns them): used as given.  A dict {"P": P0, "Q": Q0} [n]: the base case
    with these loads is solved cold on the handle first (one scenario, reference start, pf, harmonic NR to min(thresh_h, 1e-9)) and captured on
    the device; RuntimeError if it does not converge.  "mean": shorthand for the column means of this call's P, Q -- which DEPENDS on the
    scenarios this call holds: a multi-GPU sweep whose results must not depend on the number of GPUs passes the same {"P", "Q"} on every rank.
    Records of warm scenarios carry flags bit 8, and each is bit-identical to apply_start(1) + set_loads + solve of the scenario alone.  A warm
    scenario that does not converge (bit 8 without bit 0) is solved again cold, exactly as with start=None (its final record has no bit 8); the
    flagged ones (bits 2, 3, 6) are repeated from the start state through apply_start + solve first and go the cold way if that leaves them
    not converged.  The accumulators count a scenario that is solved again as deferred and add it once, from the solve whose record is returned.
    The start state is taken off the handle for the cold re-solves and put back after them, and cleared when the call returns.
    update: "polar" (default): the reference's state update, today's behaviour bit for bit.  "rectangular": every harmonic Newton step is applied
    to U = Vm e^(j Va) instead of being added to (Va, Vm) (option "rectangular_update", include/hpf.h) -- 3 - 4 iterations from
    the reference's start instead of 20 - 30, the same fixed point; the base case of a warm start is solved in the same mode.  Records carry flags
    bit 9.  A scenario that does not converge this way (bit 9 without bit 0, after the re-solves above) is solved again with the reference's
    update, cold: its final record carries neither bit 9 nor bit 8 and is what update="polar" returns for it; the accumulators count it as deferred
    and add it once.  The handle's option is put back to what it was when the call returns.  ValueError for any other string.
    sources: None (default): every scenario has the model's Norton source currents I_N, today's behaviour bit for bit.  Otherwise per-scenario
    source currents of the nonlinear buses (include/hpf.h "Source currents"): {"scale": [n_scen][n-m], "shift": [n_scen][n-m]}
    (either may be missing: 1 / 0) -- scale units of each bus's device in service, their waveform shifted in time by shift rad at the fundamental,
    expanded on the device with dm.harmonics -- or {"currents": [n_scen][n-m][Hn]} complex, used as given.  Row s belongs to row s of P, Q: every
    path that solves a scenario (queue pieces, waves, the re-solves of flagged / not converged scenarios) sets its sources with its loads.  Records
    carry flags bit 10.  The base case of a warm start {"P", "Q"} is solved with the model's I_N unless the dict carries its own one-row
    "sources".  ValueError for wrong shapes, before any device call."""
    from .device import DeviceModel
    if not (isinstance(update, str) and update in DeviceModel.UPDATES):
        raise ValueError("solve_scenarios: update=%r ('polar' or 'rectangular')" % (update,))
    src = sources_argument(sources, np.atleast_2d(np.asarray(P)).shape[0], dm.n - dm.m, dm.Hn)
    if isinstance(start, dict) and start.get("sources") is not None:
        sources_argument(start["sources"], 1, dm.n - dm.m, dm.Hn, "solve_scenarios: start")
    with dm.update_mode(update):
        return _solve_scenarios_started(dm, P, Q, thresh_f, max_iter_f, thresh_h, max_iter_h, want_voltages, refill, distortion, branches, start,
                                        update == "rectangular", src, waveform)


def _solve_scenarios_started(dm, P, Q, thresh_f, max_iter_f, thresh_h, max_iter_h, want_voltages, refill, distortion, branches, start, rect,
                             src=None, waveform=None):
    """solve_scenarios inside the scope of its update mode: start state, accumulators, the sweep"""
    if start is None:
        if dm.has_start():
            raise ValueError("solve_scenarios(start=None) on a handle that holds a start state: clear_start() first, or pass start=dm.get_start()")
    else:
        _set_start(dm, P, Q, start, thresh_f, max_iter_f, thresh_h, max_iter_h)
    try:
        if distortion is None and branches is None and waveform is None:
            return _solve_scenarios(dm, P, Q, thresh_f, max_iter_f, thresh_h, max_iter_h, want_voltages, refill, False, False, start is not None,
                                    rect, src)
        if distortion is not None:
            dm.distortion_begin(distortion.get("limit"), distortion.get("thd_limit", np.inf), distortion.get("hist_max", 1.0),
                                distortion.get("bins", 64))
        try:
            if branches is not None:
                dm.branch_stats_begin(branches.get("rating"))
            if waveform is not None:
                dm.waveform_stats_begin(waveform.get("samples", 1024), waveform.get("peak_limit"), waveform.get("crest_limit", np.inf))
            res = _solve_scenarios(dm, P, Q, thresh_f, max_iter_f, thresh_h, max_iter_h, want_voltages, refill, distortion is not None,
                                   branches is not None, start is not None, rect, src, waveform is not None)
            extra = ((() if distortion is None else (dm.distortion_get(),)) + (() if branches is None else (dm.branch_stats_get(),)) +
                     (() if waveform is None else (dm.waveform_stats_get(),)))
        finally:
            dm.set_option("distortion_id_base", 0)
            if distortion is not None:
                dm.distortion_end()
            if branches is not None:
                dm.branch_stats_end()
            if waveform is not None:
                dm.waveform_stats_end()
        return (res if want_voltages else (res,)) + extra
    finally:
        if start is not None:
            dm.clear_start()


def _set_start(dm, P, Q, start, thresh_f, max_iter_f, thresh_h, max_iter_h):
    """the handle's start state from the `start` argument of solve_scenarios"""
    if isinstance(start, (tuple, list)) and len(start) == 2:
        dm.set_start(*start)
        return
    if isinstance(start, str) and start == "mean":
        P2, Q2 = np.atleast_2d(np.asarray(P, dtype=np.float64)), np.atleast_2d(np.asarray(Q, dtype=np.float64))
        start = {"P": P2.mean(axis=0), "Q": Q2.mean(axis=0)}
    if not (isinstance(start, dict) and "P" in start and "Q" in start):
        raise ValueError("solve_scenarios: start=%r (None, a pair (Vm0, Va0), {'P': .., 'Q': ..} or 'mean')" % (start,))
    dm.set_loads(np.asarray(start["P"], dtype=np.float64).reshape(1, -1), np.asarray(start["Q"], dtype=np.float64).reshape(1, -1))
    base_src = sources_argument(start.get("sources"), 1, dm.n - dm.m, dm.Hn, "solve_scenarios: start")
    if base_src:                                         # (else the base case has the model's I_N)
        dm.set_sources(base_src[1], base_src[0])
    dm.set_state(None, None, n_scen=1)
    dm.fund_pf(thresh_f, max_iter_f)
    dm.solve(min(thresh_h, 1e-9), max_iter_h)
    st = dm.stats()[0]
    if not (st["flags"] & 1):
        raise RuntimeError("solve_scenarios: the base case of the warm start did not converge (n_iter %d, flags %d, err %.3e)"
                           % (st["n_iter"], st["flags"], st["err"]))
    dm.capture_start(0)


def _solve_scenarios(dm, P, Q, thresh_f, max_iter_f, thresh_h, max_iter_h, want_voltages, refill, distortion, branches, warm=False, rect=False,
                     src=None, waveform=False):
    P = np.ascontiguousarray(np.atleast_2d(P), dtype=np.float64)
    Q = np.ascontiguousarray(np.atleast_2d(Q), dtype=np.float64)
    n_scen = P.shape[0]
    out = np.zeros(n_scen, dtype=STAT_DTYPE)
    Vm = Va = None
    if want_voltages:
        Vm = np.empty((n_scen, dm.n * dm.Hn))
        Va = np.empty_like(Vm)

    def wave(a, b, from_start=False, keep_unconverged=True):
        """scenarios a..b-1 as one batch: cold (reference start + pf) or from the start state.  keep_unconverged=False (one scenario): a result that did not converge is dropped, neither
        stored nor added -- the caller solves the scenario again -> False"""
        dm.set_loads(P[a:b], Q[a:b])
        if src:                                          # (every path that sets the loads of rows a..b sets their sources right after)
            dm.set_sources(src[1][a:b], src[0])
        if from_start:
            dm.apply_start(b - a)
        else:
            dm.set_state(None, None, n_scen=b - a)
            dm.fund_pf(thresh_f, max_iter_f)
        dm.solve(thresh_h, max_iter_h)
        st = dm.stats()
        if not keep_unconverged and not (st["flags"] & 1).all():
            return False
        if distortion:
            dm.distortion_add(a)
        if branches:
            dm.branch_stats_add(a)
        if waveform:
            dm.waveform_stats_add(a)
        for k in STAT_DTYPE.names:
            out[k][a:b] = st[k]
        if want_voltages:
            Vm[a:b], Va[a:b] = dm.get_state()
        return True

    def cold_resolves(more=()):
        # started from the start state (bit 8) and not converged, and the scenarios of `more`: each alone from the reference's start, as a sweep
        # without a start solves it -- with the start state off the handle meanwhile, so that nothing of that solve can read it
        todo = sorted(set(np.nonzero(((out["flags"] & 256) != 0) & ((out["flags"] & 1) == 0))[0].tolist()) | set(more))
        if not todo:
            return
        kept = dm.get_start()
        dm.clear_start()
        try:
            for s in todo:
                wave(s, s + 1)
        finally:
            dm.set_start(*kept)

    def polar_resolves():
        # applied in rectangular form (bit 9) and not converged, after everything above: each alone with the reference's update from the
        # reference's start, as update="polar" without a start solves it
        todo = np.nonzero(((out["flags"] & 512) != 0) & ((out["flags"] & 1) == 0))[0].tolist()
        if not (rect and todo):
            return
        kept = dm.get_start() if warm else None
        dm.set_option("rectangular_update", 0)
        try:
            if warm:
                dm.clear_start()
            for s in todo:
                wave(s, s + 1)
        finally:
            dm.set_option("rectangular_update", 1)
            if warm:
                dm.set_start(*kept)

    if not refill:
        for a in range(0, n_scen, dm.S_max):
            wave(a, min(a + dm.S_max, n_scen), from_start=warm)
        if warm:
            cold_resolves()
        polar_resolves()
        return (out, Vm, Va) if want_voltages else out
    # the device keeps the voltages of a whole call: bound a call by ~8 GB of result buffers when they are asked for
    per_call = n_scen if not want_voltages else max(dm.S_max, int(8e9 // (16 * dm.n * dm.Hn)))
    for a in range(0, n_scen, per_call):
        b = min(a + per_call, n_scen)
        if distortion or branches or waveform:
            dm.set_option("distortion_id_base", a)
        if src:
            dm.queue_sources(src[1][a:b], src[0])
        res = dm.solve_queue(P[a:b], Q[a:b], thresh_f, max_iter_f, thresh_h, max_iter_h, want_voltages=want_voltages)
        if want_voltages:
            rec, Vm[a:b], Va[a:b] = res
        else:
            rec = res
        for k in STAT_DTYPE.names:
            out[k][a:b] = rec[k]
    # static pivot order flagged (bit 3), non-finite mismatch (bit 2) or a step over the residual limit (bit 6) -- the conditions hpf_solve's
    # repeat pass looks at (k_mark_repeat): the scenario alone, hpf_solve repeats it pivoted on a radial block-tree handle (a meshed handle has
    # no pivoted repeat: the re-solve runs the same static-pivot step again)
    failed = []                                          # repeated from the start state without converging: the cold way below
    for s in np.nonzero((out["flags"] & (8 | 4 | 64)) != 0)[0]:
        if not warm:
            wave(int(s), int(s) + 1)
        elif not wave(int(s), int(s) + 1, from_start=True, keep_unconverged=False):
            failed.append(int(s))
    if warm:
        cold_resolves(failed)
    polar_resolves()
    return (out, Vm, Va) if want_voltages else out


def summarize(raw):
    """raw: uint8 array [n, 24] -> convergence statistics of the sweep."""
    st = np.ascontiguousarray(raw).view(STAT_DTYPE).reshape(-1)
    conv = (st["flags"] & 1) != 0
    out = {"scenarios": int(len(st)), "converged": int(conv.sum()), "hit_max_iter": int(((st["flags"] & 2) != 0).sum()),
           "non_finite": int(((st["flags"] & 4) != 0).sum()),
           "step_flagged": int(((st["flags"] & 64) != 0).sum()), "step_flagged_in_result": int(((st["flags"] & 128) != 0).sum()),
           "iters_min": int(st["n_iter"].min()), "iters_max": int(st["n_iter"].max()),
           "iters_mean": float(st["n_iter"].mean()), "iters_total": int(st["n_iter"].sum())}
    if conv.any():
        out["err_max_converged"] = float(st["err"][conv].max())
        thd = st["thd_max"][conv]
        thd = thd[np.isfinite(thd)]
        if len(thd):
            out["thd_max"] = float(thd.max())
            # distribution over scenarios of the worst-bus THD_F (each record carries the max over buses, HG:563-572)
            for q in (50, 95, 99):
                out["thd_p%d" % q] = float(np.percentile(thd, q))
    return out


def pack_stats(n_iter, flags, err, thd):
    """Host-side packing of the record layout (tests)."""
    st = np.zeros(len(n_iter), dtype=STAT_DTYPE)
    st["n_iter"], st["flags"], st["err"], st["thd_max"] = n_iter, flags, err, thd
    return st.view(np.uint8).reshape(len(n_iter), 24)
