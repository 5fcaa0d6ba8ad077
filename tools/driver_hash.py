#!/usr/bin/env python3
"""sha256 digests of what each driver of the harmonic Newton iteration leaves -- hpf_iterate, hpf_solve and the queued sweep -- on handles that
take every branch of the shared enqueue (bit-identity check of two library builds on one box, as tools/state_hash.py):
HPF_LIB_PATH=<lib.so> python tools/driver_hash.py > out.txt      # one line per (handle, driver); two builds agree when the files are equal"""
import hashlib
import os
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402
import harmonic_power_flow_amd as hp  # noqa: E402
from harmonic_power_flow_amd import ingest, synth  # noqa: E402

HMAX = 11


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


def feeder(buses, ties):
    tmp = tempfile.mkdtemp(prefix="hpf_driver_hash_")
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


def run(name, f, slots, solver, options=()):
    n = f["n"]
    dm = hp.DeviceModel(n, f["m"], f["c"], f["harmonics"], f["Y"].rowptr, f["Y"].col, f["Y"].Yval, f["dev"], f["Y_N"], f["I_N"], f["n_dev"], True,
                        solver=solver, max_scenarios=slots)
    for o in options:
        dm.set_option(o, 1)
    scale = np.stack([synth.scenario_scale(n, s) for s in range(3 * slots)])
    P, Q = f["P"] * scale, f["Q"] * scale
    head = "%-12s groups %d" % (name, dm.scenario_groups(slots))

    def seed():
        dm.set_loads(P[:slots], Q[:slots])
        dm.set_state(None, None, n_scen=slots)
        dm.fund_pf(1e-6, 30)

    seed()
    dm.mismatch(want_f=False)
    dm.iterate(3)
    dm.sync()
    fm, err = dm.mismatch()
    print("%s  iterate(3)   state %s  mismatch %s" % (head, sha(*dm.get_state()), sha(fm, err)))
    seed()
    n_iter, err, hist = dm.solve(1e-4, 50)
    st = dm.stats()
    print("%s  solve        state %s  n_iter %s  err %s  hist %s  stats %s  iters %d..%d" %
          (head, sha(*dm.get_state()), sha(n_iter), sha(err), sha(hist), sha(st), n_iter.min(), n_iter.max()))
    rec, Vm, Va = dm.solve_queue(P, Q, 1e-6, 30, 1e-4, 50, want_voltages=True)
    print("%s  solve_queue  state %s  stats %s  flags %s" % (head, sha(Vm, Va), sha(rec), sorted(set(int(x) for x in rec["flags"]))))
    dm.close()


radial = feeder(120, 0)
run("radial-20", radial, 20, "block_tree")
run("radial-80", radial, 80, "block_tree")
run("radial-80-opt", radial, 80, "block_tree", ("keep_previous_state", "step_residual_check", "rectangular_update"))
run("meshed-20", feeder(100, 4), 20, "block_tree")
run("dense-20", radial, 20, "dense")
