#!/usr/bin/env python3
"""End-to-end effect of the rectangular state update (option "rectangular_update"): the headline sweep -- 1 024 Monte-Carlo scenarios
(synth.scenario_scale) of the 1 000-bus x 26-harmonic feeder through a 128-slot handle, records only -- timed end to end, five runs after a
warm-up, median and spread.  Legs: the parent commit cold (another checkout, --parent-tree; twice, around the others: its own run-to-run spread
is the margin for "off costs nothing"), this checkout cold with the option off, cold with the option on at "queue_chunk" 1 / 2 / 4, warm
(start = the nominal-load base case, solved in the same mode; its solve is inside the time) with the option on at "queue_chunk" 1 / 2.
Reported per leg: median (min .. max) ms, iters_total, scenarios solved again with the polar update, and -- from one more, untimed pair of
sweeps with voltages -- the largest |dU| of the leg's voltages against the option-off cold sweep of the same handle.  Plus one
rocprofv3 --kernel-trace --stats run of an option-on sweep (no counters in it).

    python tools/sweep_rect_update.py all --out DIR [--parent-tree PATH]      every leg as its own process, JSON -> DIR/rect_update.json
    python tools/sweep_rect_update.py leg [--update rectangular] [--warm] [--chunk 4] [--tree PATH] [--runs 5]      one leg, one JSON line

Every leg that touches the GPU runs as a fresh child process under its own time limit (timeout -k 10); `all` stops at the first leg that
fails."""
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
    rect = args.update == "rectangular"
    kw = {}
    if rect:
        kw["update"] = "rectangular"                     # (a parent checkout has no such argument: its legs never pass it)
    if args.warm:
        kw["start"] = {"P": P0, "Q": Q0}
    dm.set_option("queue_chunk", args.chunk)
    times, rec = [], None
    for r in range(args.runs + 1):                       # (run 0: warm-up)
        t0 = time.perf_counter()
        rec = sweep.solve_scenarios(dm, P, Q, **kw)
        t = time.perf_counter() - t0
        if r:
            times.append(1e3 * t)
    times.sort()
    out = {"update": args.update, "warm": bool(args.warm), "queue_chunk": args.chunk,
           "tree": "this checkout" if tree == REPO else "other checkout (--tree)", "scenarios": args.scenarios, "slots": args.slots,
           "runs_ms": times, "median_ms": times[len(times) // 2], "min_ms": times[0], "max_ms": times[-1],
           "iters_total": int(rec["n_iter"].sum()), "iters_max": int(rec["n_iter"].max()), "converged": int(((rec["flags"] & 1) != 0).sum()),
           "rectangular_records": int(((rec["flags"] & 512) != 0).sum()),
           "polar_resolves": int((((rec["flags"] & 512) == 0).sum()) if rect else 0)}
    if rect:                                             # untimed: the same sweep and the option-off cold sweep, with voltages
        on = sweep.solve_scenarios(dm, P, Q, want_voltages=True, **kw)
        off = sweep.solve_scenarios(dm, P, Q, want_voltages=True)
        du = 0.0
        for a in range(0, args.scenarios, 64):
            b = a + 64
            du = max(du, float(np.abs(on[1][a:b] * np.exp(1j * on[2][a:b]) - off[1][a:b] * np.exp(1j * off[2][a:b])).max()))
        out["max_dU_against_off"] = du
        out["off_iters_total"] = int(off[0]["n_iter"].sum())
    dm.close()
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
    log = os.path.join(out, "rect_update.log")
    open(log, "w").close()
    me = [sys.executable, os.path.abspath(__file__), "leg", "--scenarios", str(args.scenarios), "--slots", str(args.slots)]
    runs = ["--runs", str(args.runs)]
    result = {"legs": [], "trace": {}}
    parent = ["--tree", args.parent_tree] if args.parent_tree else None
    on = ["--update", "rectangular"]
    legs = ([("parent_cold", parent)] if parent else []) + [("cold_off", [])] + \
        [("cold_on_chunk%d" % c, on + ["--chunk", str(c)]) for c in (1, 2, 4)] + \
        [("warm_on_chunk%d" % c, on + ["--warm", "--chunk", str(c)]) for c in (1, 2)] + \
        ([("parent_cold_again", parent)] if parent else []) + [("cold_off_again", [])]
    for name, extra in legs:
        rc, txt = _child(me + runs + extra, 400, log)
        if rc != 0:
            print("leg %s failed with exit status %d: stopping (see %s)" % (name, rc, log))
            return rc
        rec = json.loads(txt.strip().splitlines()[-1])
        rec["leg"] = name
        result["legs"].append(rec)
        print("%-18s median %8.1f ms  (min %8.1f .. max %8.1f)  iters_total %6d  converged %d  polar re-solves %d  |dU| %s"
              % (name, rec["median_ms"], rec["min_ms"], rec["max_ms"], rec["iters_total"], rec["converged"], rec["polar_resolves"],
                 "%.2e" % rec["max_dU_against_off"] if "max_dU_against_off" in rec else "-"), flush=True)
    tdir = os.path.join(out, "trace_on")                   # kernel trace: a run of its own, kernel trace only, the program behind `--`
    shutil.rmtree(tdir, ignore_errors=True)
    rc, _ = _child(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tdir, "--"] + me +
                   ["--runs", "1"] + on + ["--chunk", str(args.trace_chunk)], 500, log)
    if rc != 0:
        print("trace failed with exit status %d: stopping (see %s)" % (rc, log))
        return rc
    rows = _kernel_rows(tdir)
    shutil.rmtree(tdir, ignore_errors=True)
    total = sum(v["total_us"] for v in rows.values())
    top = sorted(rows.items(), key=lambda kv: -kv[1]["total_us"])[:12]
    result["trace"] = {"queue_chunk": args.trace_chunk,
                       "what": "cold sweeps of one process: 3 with the option on (warm-up, timed, with voltages), 1 with it off (voltages)",
                       "kernels_seen": len(rows), "all_kernels_total_us": total, "top": {k: v for k, v in top},
                       "update_kernels": {k: v for k, v in rows.items() if k.startswith("k_update")}}
    for k, v in top:
        print("trace  %-40s %7d calls %10.0f us  %5.1f %%" % (k[:40], v["calls"], v["total_us"], 100 * v["total_us"] / total), flush=True)
    for k, v in result["trace"]["update_kernels"].items():
        print("trace  %-40s %7d calls %10.0f us  average %.2f us" % (k[:40], v["calls"], v["total_us"], v["average_us"]), flush=True)
    with open(os.path.join(out, "rect_update.json"), "w") as f:
        json.dump(result, f, indent=1)
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["all", "leg"])
    ap.add_argument("--update", default="polar", choices=["polar", "rectangular"])
    ap.add_argument("--warm", action="store_true", help="start every scenario from the nominal-load base case (solved in the same mode)")
    ap.add_argument("--chunk", type=int, default=4, help="option queue_chunk of the leg")
    ap.add_argument("--trace-chunk", type=int, default=1, help="queue_chunk of the traced option-on sweep")
    ap.add_argument("--tree", default=None, help="checkout whose package and library run the leg (default: this one)")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: its cold sweep is the yardstick")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "rect_update"))
    ap.add_argument("--scenarios", type=int, default=1024)
    ap.add_argument("--slots", type=int, default=128)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    sys.exit(leg(a) if a.what == "leg" else run_all(a))
