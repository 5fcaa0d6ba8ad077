"""Wall time of one impedance scan (hpf_impedance_scan through api.impedance_scan_arrays) of the 1 000-bus synthetic feeder with three capacitor
banks over 4 096 frequency points -- full Z returned, and peaks only -- next to the host's dense route (Y(h) from line_model, numpy.linalg.inv) on
the same machine.  The dense route would take minutes over the whole grid: it is timed on --dense-points points of the same grid and the figure
for the whole grid is that time scaled, reported as such.  Host clock around calls that end in a device synchronise; one warm-up call per variant.
Prints one JSON line.   python tools/zscan_time.py [--n 1000] [--points 4096] [--reps 5] [--dense-points 8]"""
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dense-points", type=int, default=8)
    a = ap.parse_args()
    import harmonic_power_flow_amd as hp
    from harmonic_power_flow_amd import admittance, api, synth
    import zscan_ref as ref
    fb, fl = synth.gen(a.n, seed=0, outdir=tempfile.mkdtemp())
    buses, lines, m, n, c = hp.init_network(fb, fl, settings=hp.Settings())
    model = admittance.line_model(buses, lines)
    h = np.linspace(0.5, 50.5, a.points)
    yx = np.zeros((a.points, n), dtype=np.complex128)
    for i, b in ((n // 3, 0.01), (n // 2, 0.004), (n - 1, 0.02)):
        yx[:, i] += 1j * h * b
    out = {"n": n, "points": a.points, "reps": a.reps}
    for name, full in (("full", True), ("peaks_only", False)):
        api.impedance_scan_arrays(model, h, yx, (), 0, full)                    # warm-up: code objects, first allocations
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            rc, Z, _, zpeak, fpeak = api.impedance_scan_arrays(model, h, yx, (), 0, full)
            ts.append(1e3 * (time.perf_counter() - t0))
        out[name + "_ms"] = [round(t, 3) for t in ts]
        out[name + "_rc"] = rc
        if full:
            keep = Z, zpeak
    pick = np.linspace(0, a.points - 1, a.dense_points).astype(int)
    ref.dense_scan(model, h[pick[:1]], yx[pick[:1]])
    t0 = time.perf_counter()
    Zd, kappa, _ = ref.dense_scan(model, h[pick], yx[pick])
    dt = time.perf_counter() - t0
    out["dense_host_points"] = len(pick)
    out["dense_host_s_per_point"] = round(dt / len(pick), 4)                    # (includes the condition number of the point: one SVD)
    t0 = time.perf_counter()
    for f in pick:
        np.linalg.inv(ref.dense_Y(model, h[f], yx[f]))
    dt = time.perf_counter() - t0
    out["dense_inv_only_s_per_point"] = round(dt / len(pick), 4)
    out["dense_inv_only_s_scaled_to_grid"] = round(dt / len(pick) * a.points, 1)
    want = np.diagonal(Zd, axis1=1, axis2=2)
    err = np.abs(keep[0][pick] - want).max(axis=1) / np.abs(want).max(axis=1)
    out["kappa_max"] = float(kappa.max())
    out["err_over_bound_max"] = float((err / (ref.EPS * kappa)).max())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
