"""Wall time of one harmonic penetration (hpf_penetration through hp.penetration) of the 1 000-bus synthetic feeder: the 25 odd harmonics 3 .. 51,
1 024 scenarios of currents="norton" with scale / shift sources, shunts="norton", statistics only (full=False) -- next to the host route on the
same machine: scipy.sparse.linalg.splu of Y(h) + diag(Y_N) per harmonic and one solve with all 1 024 right-hand sides, then the same statistics
in NumPy.  Host clock around whole calls (the device call ends in a device synchronise and includes the host expansion of the sources and the
upload of the currents); one warm-up call per route.  Prints one JSON line.   python tools/pen_time.py [--n 1000] [--scenarios 1024] [--reps 5]"""
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
    ap.add_argument("--scenarios", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import scipy.sparse as sp
    from scipy.sparse.linalg import splu
    import harmonic_power_flow_amd as hp
    from harmonic_power_flow_amd import api, sweep, synth
    ne_dir = os.path.join(REPO, "tests", "golden", "inputs")
    st = hp.Settings()
    fb, fl = synth.gen(a.n, seed=0, outdir=tempfile.mkdtemp())
    buses, lines, m, n, c = hp.init_network(fb, fl, settings=st)
    h = np.array(list(st.HARMONICS)[1:], dtype=float)
    F, S = len(h), a.scenarios
    rng = np.random.default_rng(0)
    sources = {"scale": rng.uniform(0.0, 2.0, (S, n - m)), "shift": rng.uniform(-np.pi, np.pi, (S, n - m))}
    out = {"n": n, "nonlinear": n - m, "points": F, "scenarios": S, "reps": a.reps}

    def device():
        return hp.penetration(buses, lines, h, "norton", shunts="norton", sources=sources, full=False, settings=st, ne_dir=ne_dir)
    device()                                                                      # warm-up: code objects, first allocations
    ts = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        res = device()
        ts.append(1e3 * (time.perf_counter() - t0))
    out["device_ms"] = [round(t, 2) for t in ts]
    # the part of those calls that is hpf_penetration alone (network, Norton data and currents prepared outside the clock)
    model, hh, ids, yx = api._scan_network(buses, lines, h, "norton", None, st, ne_dir, True)
    dev, _, I_N, q = api._norton_on_grid(buses, hh, "currents", st, ne_dir, True)
    inj = np.nonzero(dev >= 0)[0]
    I_bus = I_N[dev[inj]][:, q]
    I = np.ascontiguousarray(sweep.source_currents(I_bus, sources["scale"], sources["shift"], hh).transpose(0, 2, 1))
    ts = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        rc, arrays = api.penetration_arrays(model, hh, I, inj, yx, 0, 0, False)
        ts.append(1e3 * (time.perf_counter() - t0))
    out["device_call_only_ms"] = [round(t, 2) for t in ts]
    out["rc"] = rc

    # the host route: sparse LU per harmonic, one multi-right-hand-side solve, the statistics in NumPy
    fr, to = np.asarray(model["fr"]), np.asarray(model["to"])

    def host():
        V = np.empty((S, F, n), dtype=np.complex128)
        for f, x in enumerate(hh):
            y = 1.0 / (model["R"] + 1j * x * model["X"])
            d = model["gsh"] + 1j * x * model["bsh"] + yx[f]
            nz = model["xsh"] != 0
            if x != 1:
                d[nz] += 1.0 / (1j * model["xsh"][nz] * x)
            Y = sp.coo_matrix((np.concatenate([-y, -y, y, y, d]), (np.concatenate([fr, to, fr, to, np.arange(n)]),
                                                                   np.concatenate([to, fr, fr, to, np.arange(n)]))), shape=(n, n)).tocsc()
            b = np.zeros((n, S), dtype=np.complex128)
            b[inj] = I[:, f, :].T
            V[:, f, :] = splu(Y).solve(b).T
        mag = np.abs(V)
        return mag.max(axis=0), mag.argmax(axis=0), mag.mean(axis=0), mag.std(axis=0), np.sqrt((mag * mag).sum(axis=1))
    host()
    ts = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        vmax, varg, vmean, vstd, rss = host()
        ts.append(1e3 * (time.perf_counter() - t0))
    out["host_splu_ms"] = [round(t, 2) for t in ts]
    out["vmax_rel_diff"] = float((np.abs(res.vmax - vmax) / vmax.max()).max())
    out["rss_rel_diff"] = float((np.abs(res.rss - rss) / rss.max()).max())
    out["varg_equal"] = float((res.varg == varg).mean())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
