"""Wall time of one resonance mode analysis (hpf_resonance_modes through api.resonance_modes_arrays) of the 1 000-bus synthetic feeder with three
capacitor banks over 4 096 frequency points at 32 steps -- with the participation factors returned, and without -- next to the host route on the
same machine: numpy.linalg.eig of the dense Y(h) (from line_model) on --dense-points points of the same grid; the figure for the whole grid is
that time scaled, reported as such.  Host clock around whole calls that end in a device synchronise; one warm-up call per variant.  Also prints
the depth of the BFS tree and the launches one step costs (the two walks, the two pivot stages, the scaling).  Not measured: kernel times,
bandwidth, meshed networks.  Prints one JSON line.   python tools/rma_time.py [--n 1000] [--points 4096] [--iters 32] [--reps 5] [--dense-points 4]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dense-points", type=int, default=4)
    a = ap.parse_args()
    import harmonic_power_flow_amd as hp
    from harmonic_power_flow_amd import admittance, api, synth
    import zscan_emul as ze
    import zscan_ref as ref
    fb, fl = synth.gen(a.n, seed=0, outdir=tempfile.mkdtemp())
    buses, lines, m, n, c = hp.init_network(fb, fl, settings=hp.Settings())
    model = admittance.line_model(buses, lines)
    h = np.linspace(0.5, 50.5, a.points)
    yx = np.zeros((a.points, n), dtype=np.complex128)
    for i, b in ((n // 3, 0.01), (n // 2, 0.004), (n - 1, 0.02)):
        yx[:, i] += 1j * h * b
    _, _, depth, ties = ze.plan(model)
    depths = int(depth.max()) + 1
    out = {"n": n, "points": a.points, "iters": a.iters, "reps": a.reps, "tree_depths": depths, "ties": len(ties),
           "launches_per_step": 2 * depths - 1 + 3 + (2 if len(ties) else 0)}
    for name, full in (("with_pf", True), ("peaks_only", False)):
        api.resonance_modes_arrays(model, h, yx, a.iters, 0, full)              # warm-up: code objects, first allocations
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            rc, lam, zm, res, top, pf = api.resonance_modes_arrays(model, h, yx, a.iters, 0, full)
            ts.append(1e3 * (time.perf_counter() - t0))
        out[name + "_ms"] = [round(t, 2) for t in ts]
        out[name + "_rc"] = rc
        if full:
            keep = lam, res
    out["converged_1e-8"] = int((keep[1] <= 1e-8).sum())
    pick = np.linspace(0, a.points - 1, a.dense_points).astype(int)
    np.linalg.eig(ref.dense_Y(model, h[pick[0]], yx[pick[0]]))
    t0 = time.perf_counter()
    lam1 = []
    for f in pick:
        w, v = np.linalg.eig(ref.dense_Y(model, h[f], yx[f]))
        lam1.append(w[np.abs(w).argmin()])
    dt = time.perf_counter() - t0
    out["dense_eig_points"] = len(pick)
    out["dense_eig_s_per_point"] = round(dt / len(pick), 3)
    out["dense_eig_s_scaled_to_grid"] = round(dt / len(pick) * a.points, 1)
    out["lam_rel_diff_at_those_points"] = [float(abs(keep[0][f] - l) / abs(l)) for f, l in zip(pick, lam1)]
    out["res_at_those_points"] = [float(keep[1][f]) for f in pick]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
