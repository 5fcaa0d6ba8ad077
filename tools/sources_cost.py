#!/usr/bin/env python3
"""Cost of per-scenario source currents (hpf_set_sources / hpf_queue_sources) on the headline feeder (1 000 buses x 26 harmonics):
(b) time per step of hpf_iterate for S scenarios with the sources unset / set (form 1) and the mismatch kernel's own span (timing class 0);
(c) the 1 024-scenario queue through S slots without / with hpf_queue_sources.

python tools/sources_cost.py [--S 128] [--blocks 5] [--iters 40] [--queue 1024] [--json out.json]

One process measures one library (env HPF_LIB_PATH selects another build): an A/B against another commit interleaves processes."""
import argparse, json, os, sys, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench
import harmonic_power_flow_amd as hp
from harmonic_power_flow_amd import synth

ap = argparse.ArgumentParser()
ap.add_argument("--S", type=int, default=128)
ap.add_argument("--blocks", type=int, default=5)
ap.add_argument("--iters", type=int, default=40)
ap.add_argument("--queue", type=int, default=1024)
ap.add_argument("--json", default=None)
a = ap.parse_args()
inp = bench.build_inputs(argparse.Namespace(buses=1000, hmax=51), hp)
n, m = inp["n"], inp["m"]
P0, Q0 = inp["buses"]["P"].to_numpy(float), inp["buses"]["Q"].to_numpy(float)
S = a.S
dm = hp.DeviceModel(n, m, inp["c"], inp["st"].HARMONICS, inp["Y"].rowptr, inp["Y"].col, inp["Y"].Yval, inp["dev"], inp["Y_N"], inp["I_N"],
                    inp["n_dev"], True, solver="block_tree", max_scenarios=S)
rng = np.random.default_rng(7)
nq = max(a.queue, S)
# a few per cent of scale and shift: the steps stay the steps of a sweep that converges (the timing does not depend on the values)
ab = np.stack([rng.uniform(0.97, 1.03, (nq, n - m)), rng.uniform(-0.01, 0.01, (nq, n - m))], axis=2)
scale = np.stack([synth.scenario_scale(n, s) for s in range(nq)])
out = {"S": S, "iters": a.iters, "blocks": a.blocks, "lib": os.environ.get("HPF_LIB_PATH", "in-tree")}
dm.set_loads(P0 * scale[:S], Q0 * scale[:S])
dm.set_state(None, None, n_scen=S)
dm.fund_pf(1e-6, 30)
seed = dm.get_state()
for mode in ("unset", "set", "unset_again"):
    if mode == "set":
        dm.set_sources(ab[:S], "scale_shift")
    if mode == "unset_again":
        dm.clear_sources()
    per = []
    for blk in range(a.blocks + 1):                      # (block 0: warm-up, dropped)
        dm.set_state(*seed)
        dm.mismatch(want_f=False)
        dm.iterate(3)
        dm.sync()
        t0 = time.perf_counter()
        dm.iterate(a.iters)
        dm.sync()
        per.append(1e3 * (time.perf_counter() - t0) / a.iters)
    per = per[1:]
    dm.set_state(*seed)
    dm.mismatch(want_f=False)
    dm.timing(True)
    dm.timing_reset()
    dm.iterate(a.iters)
    dm.sync()
    mm, cnt = dm.timing_get()["mismatch"]
    dm.timing(False)
    out[mode] = {"ms_per_step_median": float(np.median(per)), "min": min(per), "max": max(per), "mismatch_us_per_launch": 1e3 * mm / max(cnt, 1),
                 "mismatch_launches": cnt}
    print("S=%d sources %-11s: %.4f ms per step (median of %d blocks of %d; min %.4f max %.4f); mismatch span %.2f us per launch (%d launches)"
          % (S, mode, out[mode]["ms_per_step_median"], a.blocks, a.iters, min(per), max(per), out[mode]["mismatch_us_per_launch"], cnt), flush=True)
if a.queue > 0:
    Pq, Qq = P0 * scale[:a.queue], Q0 * scale[:a.queue]
    for mode in ("plain", "sources", "plain", "sources"):
        if mode == "sources":
            dm.queue_sources(ab[:a.queue], "scale_shift")
        t0 = time.perf_counter()
        rec = dm.solve_queue(Pq, Qq)
        ms = 1e3 * (time.perf_counter() - t0)
        out.setdefault("queue_" + mode, []).append({"ms": ms, "iters_total": int(rec["n_iter"].sum()), "converged": int((rec["flags"] & 1).sum())})
        print("queue of %d through %d slots, %-7s: %.1f ms, %d iterations in all, %d converged" % (a.queue, S, mode, ms, rec["n_iter"].sum(),
                                                                                             (rec["flags"] & 1).sum()), flush=True)
dm.close()
if a.json:
    json.dump(out, open(a.json, "w"), indent=1)
