#!/usr/bin/env python3
"""End-to-end gain of the warm start: the headline sweep -- 1 024 Monte-Carlo scenarios (synth.scenario_scale) of the 1 000-bus x
26-harmonic feeder through a 128-slot handle, records only -- timed end to end, five runs after a warm-up, median and spread: cold (no start
state), and warm from the nominal-load base case with "queue_chunk" 1, 2 and 4.  A warm run's time INCLUDES the cold solve of the base case on
the same handle (solve_scenarios(start={"P", "Q"})).  Reported per leg: median (min .. max) ms, iters_total, scenarios solved again cold.
Optionally the cold sweep of another checkout (the parent commit) as the yardstick for "a handle without a start state costs nothing"; plus
one rocprofv3 --kernel-trace --stats run of the warm sweep (no counters in it) for what dominates once a scenario takes 2 - 3 iterations.

    python tools/sweep_warm_start.py all --out DIR [--parent-tree PATH]      every leg below as its own process, JSON -> DIR/warm_start.json
    python tools/sweep_warm_start.py leg --mode cold|warm [--chunk 4] [--tree PATH] [--runs 5]      one leg, one JSON line

Every leg that touches the GPU runs as a fresh child process under its own time limit (timeout -k 10); `all` stops at the first leg that
fails.

Recommendation (profiles/warm_start/warm_start.json): a warm sweep sets "queue_chunk" to 2 -- 28.3 ms against 29.4 (1) and 31.3 (4)
at the headline shape, where the cold sweep takes 241.0: a warm scenario needs 2 iterations, and a chunk of 4 keeps its slot for two more steps
of empty launches before the next scenario moves in.  1 and 2 lie within a millisecond of each other and changed places between two sessions
(28.7 / 28.9 in an earlier one); both beat 4 by about 10 %.  The library's default stays 4 (cold sweeps: 20 - 30 iterations per scenario)."""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def leg(args):
    tree = os.path.abspath(args.tree or REPO)
    sys.path.insert(0, tree)
    import numpy as np
    import bench
    import harmonic_power_flow_amd as hp
    from harmonic_power_flow_amd import sweep, synth
    inp = bench.build_inputs(bench.parse([]), hp)
    n = inp["n"]
    P0, Q0 = inp["buses"]["P"].to_numpy(float), inp["buses"]["Q"].to_numpy(float)
    scale = np.stack([synth.scenario_scale(n, s) for s in range(args.scenarios)])
    P, Q = P0 * scale, Q0 * scale
    dm = hp.DeviceModel(n, inp["m"], inp["c"], inp["st"].HARMONICS, inp["Y"].rowptr, inp["Y"].col, inp["Y"].Yval, inp["dev"], inp["Y_N"],
                        inp["I_N"], inp["n_dev"], True, solver="block_tree", max_scenarios=args.slots)
    kw = {}
    if args.mode == "warm":
        kw["start"] = {"P": P0, "Q": Q0}
        dm.set_option("queue_chunk", args.chunk)
    times, rec, raw = [], None, None
    for r in range(args.runs + 1):                       # (run 0: warm-up)
        t0 = time.perf_counter()
        rec = sweep.solve_scenarios(dm, P, Q, **kw)
        t = time.perf_counter() - t0
        if r:
            times.append(1e3 * t)
    if args.mode == "warm":                              # what the queue itself reported, before the re-solves (one more, untimed run)
        dm.set_loads(P0, Q0)
        dm.set_state(None, None, n_scen=1)
        dm.fund_pf(1e-6, 30)
        dm.solve(1e-9, 50)
        dm.capture_start(0)
        raw = dm.solve_queue(P, Q)
        dm.clear_start()
    dm.close()
    times.sort()
    out = {"mode": args.mode, "queue_chunk": args.chunk if args.mode == "warm" else 4, "tree": "this checkout" if tree == REPO else "other checkout (--tree)",
           "scenarios": args.scenarios, "slots": args.slots, "runs_ms": times, "median_ms": times[len(times) // 2], "min_ms": times[0],
           "max_ms": times[-1], "iters_total": int(rec["n_iter"].sum()), "iters_max": int(rec["n_iter"].max()),
           "converged": int(((rec["flags"] & 1) != 0).sum()), "started_warm": int(((rec["flags"] & 256) != 0).sum())}
    if raw is not None:
        out["cold_resolves"] = int((((raw["flags"] & 256) != 0) & ((raw["flags"] & 1) == 0)).sum())
        out["flagged_resolves"] = int(((raw["flags"] & (4 | 8 | 64)) != 0).sum())
        out["queue_iters_total"] = int(raw["n_iter"].sum())
    print(json.dumps(out), flush=True)


def _child(cmd, limit, log):
    """one GPU step: a fresh process under its own time limit -> (exit status, stdout)"""
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True, cwd=REPO)
    with open(log, "a") as f:
        f.write("$ %s\n%s\n%s\n[exit %d]\n" % (" ".join(cmd), p.stdout, p.stderr[-4000:], p.returncode))
    return p.returncode, p.stdout


def _kernel_rows(trace_dir):
    rows = {}
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = r["Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
            rows[name] = {"calls": int(r["Calls"]), "total_us": float(r["TotalDurationNs"]) / 1e3, "average_us": float(r["AverageNs"]) / 1e3,
                          "percent": float(r["Percentage"])}
    return rows


def run_all(args):
    out = os.path.abspath(args.out)
    os.makedirs(out, exist_ok=True)
    log = os.path.join(out, "warm_start.log")
    open(log, "w").close()
    me = [sys.executable, os.path.abspath(__file__), "leg", "--scenarios", str(args.scenarios), "--slots", str(args.slots)]
    runs = ["--runs", str(args.runs)]
    result = {"legs": [], "trace": {}}
    parent = ["--mode", "cold", "--tree", args.parent_tree] if args.parent_tree else None
    legs = ([("parent_cold", parent)] if parent else []) + [("cold", ["--mode", "cold"])] + \
        [("warm_chunk%d" % c, ["--mode", "warm", "--chunk", str(c)]) for c in (1, 2, 4)] + \
        ([("parent_cold_again", parent)] if parent else []) + [("cold_again", ["--mode", "cold"])]
    for name, extra in legs:
        rc, txt = _child(me + runs + extra, 400, log)
        if rc != 0:
            print("leg %s failed with exit status %d: stopping (see %s)" % (name, rc, log))
            return rc
        rec = json.loads(txt.strip().splitlines()[-1])
        rec["leg"] = name
        result["legs"].append(rec)
        print("%-18s median %8.1f ms  (min %8.1f .. max %8.1f)  iters_total %6d  converged %d  cold re-solves %s"
              % (name, rec["median_ms"], rec["min_ms"], rec["max_ms"], rec["iters_total"], rec["converged"], rec.get("cold_resolves", "-")),
              flush=True)
    tdir = os.path.join(out, "trace_warm")                 # kernel trace: a run of its own, kernel trace only, the program behind `--`
    shutil.rmtree(tdir, ignore_errors=True)
    rc, _ = _child(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tdir, "--"] + me +
                   ["--runs", "1", "--mode", "warm", "--chunk", str(args.trace_chunk)], 500, log)
    if rc != 0:
        print("trace failed with exit status %d: stopping (see %s)" % (rc, log))
        return rc
    rows = _kernel_rows(tdir)
    shutil.rmtree(tdir, ignore_errors=True)
    total = sum(v["total_us"] for v in rows.values())
    top = sorted(rows.items(), key=lambda kv: -kv[1]["total_us"])[:12]
    result["trace"] = {"queue_chunk": args.trace_chunk, "what": "warm-up + 1 timed + 1 untimed warm sweep, three base solves", "kernels_seen": len(rows),
                       "all_kernels_total_us": total, "top": {k: v for k, v in top},
                       "start_kernels": {k: v for k, v in rows.items() if k.startswith("k_start_") or k.startswith("k_queue_")}}
    for k, v in top:
        print("trace  %-40s %7d calls %10.0f us  %5.1f %%" % (k[:40], v["calls"], v["total_us"], 100 * v["total_us"] / total), flush=True)
    with open(os.path.join(out, "warm_start.json"), "w") as f:
        json.dump(result, f, indent=1)
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["all", "leg"])
    ap.add_argument("--mode", default="cold", choices=["cold", "warm"])
    ap.add_argument("--chunk", type=int, default=4, help="option queue_chunk of a warm leg")
    ap.add_argument("--trace-chunk", type=int, default=1, help="queue_chunk of the traced warm sweep")
    ap.add_argument("--tree", default=None, help="checkout whose package and library run the leg (default: this one)")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: its cold sweep is the yardstick")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "warm_start"))
    ap.add_argument("--scenarios", type=int, default=1024)
    ap.add_argument("--slots", type=int, default=128)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    sys.exit(leg(a) if a.what == "leg" else run_all(a))
