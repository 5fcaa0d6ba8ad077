#!/usr/bin/env python3
"""sha256 digests of what the three sweep accumulators return -- distortion, branch and waveform statistics, all open together -- over sweeps that
take every path into them (the queue with refill, fixed waves, a harvest round per iteration, skipped scenarios, warm-started scenarios that are
deferred and solved again): the bit-identity check of two library builds on one box, as tools/driver_hash.py:
HPF_LIB_PATH=<lib.so> python tools/accum_hash.py > out.txt      # one line per (run, accumulator); two builds agree when the files are equal
python tools/accum_hash.py --probe                              # counts only, over a range of iteration caps (how CAP_SKIP / CAP_WARM were chosen)"""
import hashlib
import os
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402
import harmonic_power_flow_amd as hp  # noqa: E402
from harmonic_power_flow_amd import ingest, sweep, synth  # noqa: E402

HMAX = 11
SLOTS, SCENARIOS = 20, 60
# harmonic iteration caps, chosen on the parent library with --probe (radial | meshed feeder, 60 scenarios, counts added / skipped / deferred):
# cold, cap 22: 33 / 27 / 0 | 39 / 21 / 0 (18: 2 / 58 / 0, 30: everything converges); warm from the base case, cap 1: 0 / 60 / 60 | 1 / 59 / 59 --
# the queue defers the warm scenarios that missed the stop rule, their cold re-solve under the same cap is skipped (cap 2: everything converges)
CAP_SKIP = 22
CAP_WARM = 1


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def feeder(buses, ties):
    tmp = tempfile.mkdtemp(prefix="hpf_accum_hash_")
    fb, fl = synth.gen(buses, seed=0, outdir=tmp)
    if ties:
        synth.add_ties(fl, buses, ties)
    st = hp.Settings(H_MAX=HMAX)
    bus, lines, m, n, c = hp.init_network(fb, fl, settings=st)
    Y = hp.build_admittance_matrices(bus, lines, st.HARMONICS)
    NE = hp.import_Norton_Equivalents(bus, True, st, bench.INPUTS)
    dev, Y_N, I_N, n_dev = ingest.norton_arrays(bus, NE, True, len(st.HARMONICS))
    return dict(n=n, m=m, c=c, harmonics=st.HARMONICS, Y=Y, dev=dev, Y_N=Y_N, I_N=I_N, n_dev=n_dev,
                P=bus["P"].to_numpy(float), Q=bus["Q"].to_numpy(float))


def model(f):
    return hp.DeviceModel(f["n"], f["m"], f["c"], f["harmonics"], f["Y"].rowptr, f["Y"].col, f["Y"].Yval, f["dev"], f["Y_N"], f["I_N"], f["n_dev"],
                          True, solver="block_tree", max_scenarios=SLOTS)


def sweep_once(dm, f, samples, **kw):
    scale = np.stack([synth.scenario_scale(f["n"], s) for s in range(SCENARIOS)])
    P, Q = f["P"] * scale, f["Q"] * scale
    thd_limit = 0.05
    return sweep.solve_scenarios(dm, P, Q, distortion={"limit": np.full(len(f["harmonics"]), 0.02), "thd_limit": thd_limit, "hist_max": 0.2,
                                                       "bins": 32},
                                 branches={"rating": np.full(dm.nb, 0.5)},
                                 waveform={"samples": samples, "peak_limit": np.full(f["n"], 1.0), "crest_limit": 1.42}, **kw)


def base_case(dm, f):
    """the state of the feeder at its nominal loads, solved with the default iteration cap: the start of the warm runs -> (Vm0, Va0)"""
    dm.set_loads(f["P"].reshape(1, -1), f["Q"].reshape(1, -1))
    dm.set_state(None, None, n_scen=1)
    dm.fund_pf(1e-6, 30)
    dm.solve(1e-9, 50)
    assert dm.stats()[0]["flags"] & 1
    Vm, Va = dm.get_state()
    return Vm[0].copy(), Va[0].copy()


def run(name, f, samples=64, chunk=None, warm=False, **kw):
    dm = model(f)
    if warm:
        kw["start"] = base_case(dm, f)
    if chunk is not None:
        dm.set_option("queue_chunk", chunk)
    rec, *stats = sweep_once(dm, f, samples, **kw)
    print("%-22s records %s" % (name, sha(rec)))
    for st in stats:
        print("%-22s %-15s counts %s  %s" % (name, type(st).__name__, st.counts.tolist(),
                                             "  ".join("%s %s" % (a, sha(getattr(st, a))) for a in st.ARRAYS[1:])))
    dm.close()


def probe(f):
    for warm, caps in ((False, (18, 20, 22, 24, 26, 30)), (True, (1, 2, 3, 4, 6))):
        for cap in caps:
            dm = model(f)
            kw = {"start": base_case(dm, f)} if warm else {}
            rec, dist, _, _ = sweep_once(dm, f, 64, max_iter_h=cap, **kw)
            print("%s max_iter_h %2d: counts %s  converged %d of %d" % ("warm" if warm else "cold", cap, dist.counts.tolist(),
                                                                         int(((rec["flags"] & 1) != 0).sum()), len(rec)), flush=True)
            dm.close()


if __name__ == "__main__":
    radial, meshed = feeder(120, 0), feeder(100, 4)
    if "--probe" in sys.argv:
        probe(radial)
        probe(meshed)
        sys.exit(0)
    for tag, f in (("radial", radial), ("meshed", meshed)):
        run(tag + " refill", f)
        run(tag + " refill T1024", f, samples=1024)
        run(tag + " waves", f, refill=False)
        run(tag + " chunk1", f, chunk=1)
        run(tag + " skipped", f, max_iter_h=CAP_SKIP)
        run(tag + " warm deferred", f, warm=True, max_iter_h=CAP_WARM)
