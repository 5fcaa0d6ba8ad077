#!/usr/bin/env python3
"""Cost of the residual check of the Newton steps (option "step_residual_check") on the headline feeder (1 000 buses x 26 harmonics):
time per step of hpf_iterate with the check off / on, the check's own span (timing class 7) and its bytes / flops model.

python tools/step_residual_cost.py [S ...] [--mode off|on|both] [--blocks 5] [--iters 40]

One process measures one library (env HPF_LIB_PATH selects another build): an A/B against another commit interleaves processes.  Prints one
line per (S, mode): the median over the blocks of the time per step, and the blocks' spread."""
import argparse, os, sys, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench
import harmonic_power_flow_amd as hp
from harmonic_power_flow_amd import synth

ap = argparse.ArgumentParser()
ap.add_argument("S", nargs="*", type=int, default=[128, 1])
ap.add_argument("--mode", default="both")
ap.add_argument("--blocks", type=int, default=5)
ap.add_argument("--iters", type=int, default=40)
ap.add_argument("--tag", default="")
a = ap.parse_args()
inp = bench.build_inputs(argparse.Namespace(buses=1000, hmax=51), hp)
n = inp["n"]
P0, Q0 = inp["buses"]["P"].to_numpy(float), inp["buses"]["Q"].to_numpy(float)
for S in a.S:
    dm = hp.DeviceModel(n, inp["m"], inp["c"], inp["st"].HARMONICS, inp["Y"].rowptr, inp["Y"].col, inp["Y"].Yval, inp["dev"], inp["Y_N"], inp["I_N"],
                        inp["n_dev"], True, solver="block_tree", max_scenarios=S)
    scale = np.stack([synth.scenario_scale(n, s) for s in range(S)])
    dm.set_loads(P0 * scale, Q0 * scale)
    dm.set_state(None, None, n_scen=S)
    dm.fund_pf(1e-6, 30)
    seed = dm.get_state()
    for mode in (("off", "on") if a.mode == "both" else (a.mode,)):
        if mode == "on":
            dm.set_option("step_residual_check", 1)
        per = []
        for blk in range(a.blocks + 1):                      # (block 0: warm-up, dropped)
            dm.set_state(*seed)
            dm.mismatch(want_f=False)
            dm.iterate(3)
            dm.sync()
            t0 = time.perf_counter()
            dm.iterate(a.iters)
            dm.sync()
            per.append(1e6 * (time.perf_counter() - t0) / a.iters)
        per = per[1:]
        line = "%s S=%4d check %-3s: %9.2f us per step (median of %d blocks of %d steps; min %.2f max %.2f)" % (
            a.tag, S, mode, float(np.median(per)), a.blocks, a.iters, min(per), max(per))
        if mode == "on":
            dm.set_state(*seed)
            dm.mismatch(want_f=False)
            dm.timing(True)
            dm.timing_reset()
            dm.iterate(a.iters)
            dm.sync()
            tim = dm.timing_get()
            dm.timing(False)
            by, fl, ln = dm.kernel_model("step_residual")
            ms, cnt = tim["step_residual"]
            mm, mcnt = tim["mismatch"]
            line += "\n%s S=%4d   check span (class 7, HIP events): %.2f us per launch pair, %d spans; mismatch span %.2f us, %d spans; model %.3f MB, %.3f Mflop per scenario and step, %d launches; eta_max %.2e" % (
                a.tag, S, 1e3 * ms / max(cnt, 1), cnt, 1e3 * mm / max(mcnt, 1), mcnt, by / 1e6, fl / 1e6, ln, float(np.nanmax(dm.step_residuals()[1])))
        print(line, flush=True)
    dm.close()
