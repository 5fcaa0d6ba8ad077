#!/usr/bin/env python3
"""Cost of the device-side sweep accumulators (DESIGN.md 6.1 distortion, 6.2 branch statistics, 6.6 waveform statistics): the headline sweep -- 1 024 Monte-Carlo
scenarios of the 1 000-bus x 26-harmonic feeder through a 128-slot handle, records only -- timed end to end, five runs after a warm-up, median
and spread, with every accumulator closed and with the accumulators of each leg open (--modes: distortion, branches, both = those two, waveform,
three = all of them); optionally the same sweep of another checkout (the parent commit) as the yardstick; plus rocprofv3 --kernel-trace --stats
runs (no counters) for the per-launch time of k_distortion_add / k_branch_add / k_wave_peaks / k_wave_add and for the proof that no accumulator
kernel is launched while closed.  The runs behind DESIGN.md 6.1 / 6.2 wrote profiles/accumulators (the default --out), those behind 6.6
--out profiles/waveform.

    python tools/sweep_accumulators.py all --out DIR [--parent-tree PATH]     every leg below as its own process, JSON -> DIR/accumulators.json
    python tools/sweep_accumulators.py leg --mode closed|distortion|branches|both|waveform|three [--tree PATH] [--runs 5]      one leg, one JSON line
    --modes closed,waveform,three: the legs of `all` (default: closed,distortion,branches,both; the last one is traced beside `closed`)
    --warm: every scenario from the base case solved at the nominal loads (solve_scenarios(start={"P", "Q"})) instead of cold

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
DIST = {"limit": None, "thd_limit": 0.08, "hist_max": 0.2, "bins": 64}


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
    if args.mode in ("distortion", "both", "three"):
        kw["distortion"] = DIST
    if args.mode in ("branches", "both", "three"):
        kw["branches"] = {"rating": None}
    if args.mode in ("waveform", "three"):
        kw["waveform"] = {"samples": 1024}
    acc = len(kw)
    if args.warm:
        kw["start"] = {"P": P0, "Q": Q0}
    times, iters, added = [], 0, None
    for r in range(args.runs + 1):                       # (run 0: warm-up)
        t0 = time.perf_counter()
        res = sweep.solve_scenarios(dm, P, Q, **kw)
        t = time.perf_counter() - t0
        rec = res[0] if acc else res
        iters = int(rec["n_iter"].sum())
        added = [int(s.added) for s in res[1:]] if acc else []
        if r:
            times.append(1e3 * t)
    dm.close()
    times.sort()
    print(json.dumps({"mode": args.mode, "warm": bool(args.warm), "tree": os.path.relpath(tree, REPO), "scenarios": args.scenarios, "slots": args.slots, "runs_ms": times,
                      "median_ms": times[len(times) // 2], "min_ms": times[0], "max_ms": times[-1], "nr_iterations": iters, "added": added,
                      "converged": int(((rec["flags"] & 1) != 0).sum())}), flush=True)


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
                          "min_us": float(r["MinNs"]) / 1e3, "max_us": float(r["MaxNs"]) / 1e3, "percent": float(r["Percentage"])}
    return rows


def run_all(args):
    out = os.path.abspath(args.out)
    os.makedirs(out, exist_ok=True)
    log = os.path.join(out, "accumulators.log")
    open(log, "w").close()
    me = [sys.executable, os.path.abspath(__file__), "leg", "--scenarios", str(args.scenarios), "--slots", str(args.slots), "--runs", str(args.runs)] + \
        (["--warm"] if args.warm else [])
    modes = args.modes.split(",")
    result = {"legs": [], "trace": {}}
    legs = ([("parent", ["--mode", "closed", "--tree", args.parent_tree])] if args.parent_tree else []) + \
        [(m, ["--mode", m]) for m in modes] + \
        ([("parent_again", ["--mode", "closed", "--tree", args.parent_tree])] if args.parent_tree else []) + [("closed_again", ["--mode", "closed"])]
    for name, extra in legs:
        rc, txt = _child(me + extra, 240, log)
        if rc != 0:
            print("leg %s failed with exit status %d: stopping (see %s)" % (name, rc, log))
            return rc
        rec = json.loads(txt.strip().splitlines()[-1])
        rec["leg"] = name
        result["legs"].append(rec)
        print("%-13s median %8.1f ms  (min %8.1f, max %8.1f)  %d NR iterations, added %s"
              % (name, rec["median_ms"], rec["min_ms"], rec["max_ms"], rec["nr_iterations"], rec["added"]), flush=True)
    for mode in ("closed", modes[-1]):                    # kernel traces: a run of their own, kernel trace only, the program behind `--`
        tdir = os.path.join(out, "trace_" + mode)
        shutil.rmtree(tdir, ignore_errors=True)
        rc, _ = _child(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tdir, "--"] + me[:2] +
                       ["leg", "--mode", mode, "--scenarios", str(args.scenarios), "--slots", str(args.slots), "--runs", "1"] +
                       (["--warm"] if args.warm else []), 400, log)
        if rc != 0:
            print("trace %s failed with exit status %d: stopping (see %s)" % (mode, rc, log))
            return rc
        rows = _kernel_rows(tdir)
        shutil.rmtree(tdir, ignore_errors=True)
        acc = {k: v for k, v in rows.items() if k in ("k_distortion_add", "k_branch_add", "k_branch_flows", "k_branch_loss_h", "k_wave_add") or
               k.startswith("k_wave_peaks")}
        result["trace"][mode] = {"accumulator_kernels": acc, "kernels_seen": len(rows),
                                 "all_kernels_total_us": sum(v["total_us"] for v in rows.values())}
        print("trace %-7s %d kernel names; accumulator kernels: %s" % (mode, len(rows), json.dumps(acc)), flush=True)
    result["closed_launches_no_branch_kernel"] = bool(result["trace"]["closed"]["kernels_seen"] > 0 and
                                                      not result["trace"]["closed"]["accumulator_kernels"])
    with open(os.path.join(out, "accumulators.json"), "w") as f:
        json.dump(result, f, indent=1)
    print("closed run launches no accumulator kernel: %s" % result["closed_launches_no_branch_kernel"])
    return 0 if result["closed_launches_no_branch_kernel"] else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["all", "leg"])
    ap.add_argument("--mode", default="closed", choices=["closed", "distortion", "branches", "both", "waveform", "three"])
    ap.add_argument("--modes", default="closed,distortion,branches,both", help="all: the legs of this checkout, in order")
    ap.add_argument("--warm", action="store_true", help="warm start from the base case at the nominal loads")
    ap.add_argument("--tree", default=None, help="checkout whose package and library run the leg (default: this one)")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: its closed sweep is the yardstick")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "accumulators"))
    ap.add_argument("--scenarios", type=int, default=1024)
    ap.add_argument("--slots", type=int, default=128)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    sys.exit(leg(a) if a.what == "leg" else run_all(a))
