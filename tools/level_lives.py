#!/usr/bin/env python3
"""Which elimination levels of one scenario group end on a scenario-batched workgroup: workgroup lives of the batched bordered buses and of the
Gauss-Jordan buses per level, from the in-kernel stamps (diagnostic build: build.py --stamps, HPF_DEBUG_ABLATE=16), next to the launch durations
of a tools/timeline_run.sh timeline.
    on the GPU box:  HPF_GROUPS=1 python tools/level_lives.py collect <scenarios> <stamps.npy>
    anywhere:        python tools/level_lives.py table <stamps.npy> [<timeline.txt>]
(levels: the heights of the planner's dump, tools/tree_plan.py -- the headline feeder, 1 000 buses, H_MAX 51)"""
import os
import re
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
NBUS, HMAX = 1000, 51


def collect(S, out):
    import ctypes as C
    import tempfile
    os.environ.setdefault("HPF_ENV_SWITCHES", "1")
    os.environ.setdefault("HPF_DEBUG_ABLATE", "16")
    os.environ.setdefault("HPF_LIB_PATH", os.path.join(REPO, "harmonic-power-flow_amd", "libhpf_stamps.so"))
    import harmonic_power_flow_amd as hp
    from harmonic_power_flow_amd import ingest, synth
    inputs = os.path.join(REPO, "tests", "golden", "inputs")
    fb, fl = synth.gen(NBUS, seed=0, outdir=tempfile.mkdtemp())
    st = hp.Settings(H_MAX=HMAX)
    buses, lines, m, n, c = hp.init_network(fb, fl, settings=st)
    Y = hp.build_admittance_matrices(buses, lines, st.HARMONICS)
    NE = hp.import_Norton_Equivalents(buses, True, st, inputs)
    dev, Y_N, I_N, n_dev = ingest.norton_arrays(buses, NE, True, len(st.HARMONICS))
    dm = hp.DeviceModel(n, m, c, st.HARMONICS, Y.rowptr, Y.col, Y.Yval, dev, Y_N, I_N, n_dev, True, solver="block_tree", max_scenarios=S)
    P0, Q0 = buses["P"].to_numpy(float), buses["Q"].to_numpy(float)
    dm.set_loads(P0 * np.stack([synth.scenario_scale(n, s) for s in range(S)]), Q0 * np.stack([synth.scenario_scale(n, s) for s in range(S)]))
    dm.set_state(None, None, n_scen=S)
    dm.fund_pf()
    dm.mismatch(want_f=False)
    dm.iterate(3)
    dm.sync()
    buf = np.zeros(S * n * 8, dtype=np.int64)
    dm._chk(dm.lib.hpf_debug_stamps(dm._h, buf.ctypes.data_as(C.POINTER(C.c_longlong)), buf.size), "hpf_debug_stamps")
    print("census", dm.tree_census())
    dm.close()
    np.save(out, buf.reshape(S, n, 8))


def table(stamps, timeline=None):
    import tree_plan
    level = {r[0]: r[2] for r in tree_plan.plan(NBUS, HMAX)}
    d = np.load(stamps)
    durs = []
    for ln in (open(timeline) if timeline else ()):
        m = re.match(r"k_level\s+grid\s+(\d+) x\s+\d+\s+start\s+[\d.]+ us\s+dur\s+([\d.]+) us", ln)
        if m:
            durs.append((int(m.group(1)), float(m.group(2))))
    print("level  launch us (grid)   batched buses: n, median life, longest bus (median over scenarios), rows, harmonics | "
          "Gauss-Jordan buses: n, median life, longest bus | ends on      (lives and phases in ticks)")
    for l in range(max(level.values()) + 1):
        ks = [k for k, v in level.items() if v == l]
        sl = [k for k in ks if d[0, k, 6] >= 1000]                                     # sleaf_batch_body: o[6] = 1000 + m, o[5] its life
        gj = [k for k in ks if d[0, k, 6] < 1000 and d[:, k, 3].sum() > 0]             # factor_q_body: assembly + Gauss-Jordan + push
        bl = np.array([np.median(d[:, k, 5]) for k in sl]) if sl else np.zeros(1)
        gl = np.array([np.median(d[:, k, 0] + d[:, k, 3] + d[:, k, 5]) for k in gj]) if gj else np.zeros(1)
        du = "%5.1f (%4d)" % (durs[l][1], durs[l][0]) if l < len(durs) else "     -     "
        ends = "-" if not sl and not gj else ("batched" if bl.max() > gl.max() else "Gauss-Jordan")
        print("%3d    %s   %3d  %6.0f  %6.0f  %6.0f  %6.0f | %3d  %6.0f  %6.0f | %s"
              % (l, du, len(sl), np.median(bl), bl.max(), np.median(d[:, sl, 0]) if sl else 0, np.median(d[:, sl, 1]) if sl else 0, len(gj),
                 np.median(gl), gl.max(), ends))


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "collect":
        collect(int(sys.argv[2]), sys.argv[3])
    elif len(sys.argv) >= 3 and sys.argv[1] == "table":
        table(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
    else:
        sys.exit(__doc__)
