"""Norton tables of four nonlinear device types, derived at test time from the committed `smps_NE.csv` (test infrastructure, like
tests/wide_ne.py), and feeders whose nonlinear buses carry more than one of them: everything the device code reads through dev_of_bus -- the
staged Y_N^T of a mismatch tile and its other-type branch, the type-dependent CSR row lengths, the per-bus images of the tree planner, I_N of
the form-1 sources -- sees one table only on the feeders of synth.gen.  Nothing is committed: write() puts the files into a directory of the
caller's.

The rules, q and p the harmonic positions 0 .. 49 of the committed table:
    smps   the committed table, copied unchanged (it reads back bit for bit)
    led    every array times 0.6 e^{0.3j} (the rule of test_gpu_parity.test_two_nonlinear_device_types_vs_oracle)
    vfd    row-scaled by a(q) = (0.5 + 0.4 cos^2(0.9 q)) e^{0.3j sin(0.5 q)}: Y_N_c[q][p] a(q), I_N_c[q] a(q), Y_N_uc[q] a(q), I_N_uc[q] a(q) --
           no scalar multiple of smps, so a wrong type, a wrong row and a transposed read all show
    band   smps with Y_N_c[q][p] = 0 for |q - p| > BAND: structural zeros, hence CSR rows of another length than the other types' rows

Chosen with the CPU oracle (synth.scenario_scale scenarios 0 - 2, the reference's stop rule, both arrangements), iterations to convergence:
    gen(24, seed=0)   four types   H_MAX 11, 51       14 - 25
    gen(24, seed=0)   three types  H_MAX 51, 99       16 - 28
    gen(90, seed=0)   three types  H_MAX 11, 51, 99   15 - 28
    gen(300, seed=2)  three types  H_MAX 27, 51       21 - 34
    gen(40, seed=1)   three types  H_MAX 51           19 - 25
Not to be used for step tests: an entrywise perturbation 1 + 0.1 cos(0.7 q + 1.3 p) of Y_N (diverges on the 90-bus feeder at H_MAX 51), and
the band type on the 90- and 300-bus feeders (diverges): band only on the 24-bus feeder."""
import os
import shutil

import numpy as np

from harmonic_power_flow_amd import ingest

K = 50                   # harmonics of the committed table
NET_FREQ = 50
BAND = 3
LED_FACTOR = 0.6 * np.exp(0.3j)
TYPES3 = ("vfd", "smps", "led")
TYPES4 = ("vfd", "band", "smps", "led")
ARRANGEMENTS = ("interleaved", "blocked")


def vfd_scale(q):
    q = np.asarray(q, dtype=np.float64)
    return (0.5 + 0.4 * np.cos(0.9 * q) ** 2) * np.exp(0.3j * np.sin(0.5 * q))


def derive(name, Ycc, Ic, Yuc, Iuc):
    """the four arrays of type `name` from those of smps (SI units, as the file holds them)"""
    if name == "smps":
        return Ycc.copy(), Ic.copy(), Yuc.copy(), Iuc.copy()
    if name == "led":
        return Ycc * LED_FACTOR, Ic * LED_FACTOR, Yuc * LED_FACTOR, Iuc * LED_FACTOR
    if name == "vfd":
        a = vfd_scale(np.arange(len(Ic)))
        return Ycc * a[:, None], Ic * a, Yuc * a, Iuc * a
    if name == "band":
        q = np.arange(len(Ic))
        Y = Ycc.copy()
        Y[np.abs(q[:, None] - q[None, :]) > BAND] = 0.0
        return Y, Ic.copy(), Yuc.copy(), Iuc.copy()
    raise ValueError(name)


def write(outdir, golden_inputs, types=TYPES4):
    """Write `<type>_NE.csv` for every type into `outdir` from `<golden_inputs>/smps_NE.csv`; -> outdir (the ne_dir of the multi-type cases)."""
    src = os.path.join(golden_inputs, "smps_NE.csv")
    freqs, Ycc, Ic, Yuc, Iuc = ingest.read_Norton_file(src)
    assert freqs == [NET_FREQ * (2 * k + 1) for k in range(K)], "the committed table: 50 odd harmonics of 50 Hz"
    for name in types:
        dst = os.path.join(str(outdir), name + "_NE.csv")
        if name == "smps":
            shutil.copy(src, dst)
        else:
            ingest.export_Norton_Equivalents(dst, freqs, *derive(name, Ycc, Ic, Yuc, Iuc))
    return str(outdir)


def type_index(arrangement, j, n_nl, T):
    """type (index into the type order) of the j-th nonlinear bus, in bus order"""
    if arrangement == "interleaved":
        return j % T                      # every mismatch tile is mixed, and the first nonlinear bus is not smps
    if arrangement == "blocked":
        return (T * j) // n_nl            # whole tiles stage a table with index > 0
    raise ValueError(arrangement)


def assign(fb, types, arrangement):
    """Rewrite the `component` column of the synth.gen bus file `fb` in place -> the type index of every nonlinear bus, in bus order (that
    is dev_of_bus of those buses: ingest numbers the types in first-seen order, and both arrangements begin with type 0)."""
    rows = open(fb).read().splitlines()
    nl = [i for i in range(1, len(rows)) if rows[i].split(";")[1] == "nonlinear"]
    T = len(types)
    assert len(nl) >= T, "fewer nonlinear buses than types"
    out = []
    for j, i in enumerate(nl):
        cols = rows[i].split(";")
        out.append(type_index(arrangement, j, len(nl), T))
        cols[2] = types[out[-1]]
        rows[i] = ";".join(cols)
    open(fb, "w").write("\n".join(rows) + "\n")
    return np.array(out, dtype=np.int32)


def feeder(outdir, n, seed, types, arrangement, ties=0):
    """synth.gen(n, seed) into `outdir` with the component column rewritten (and `ties` loop-closing lines) -> (buses.csv, lines.csv), type indices"""
    from harmonic_power_flow_amd import synth
    fb, fl = synth.gen(n, seed=seed, outdir=str(outdir))
    if ties:
        synth.add_ties(fl, n, ties, seed=seed)
    return (fb, fl), assign(fb, types, arrangement)


def host_case(outdir, golden_inputs, n=24, seed=0, types=TYPES4, arrangement="interleaved", hmax=11, coupled=True):
    """The feeder as the package and as the oracle see it, for the host tests -> dict: ne_dir, files, ti (type indices), st, buses, m / n / c, Y, NE,
    dev / Y_N / I_N / n_dev (ingest.norton_arrays), em (the device arithmetic on the host, tests/emul.py), net and mdl (the oracle's)."""
    import hpf_oracle as o
    from emul import Emul
    import harmonic_power_flow_amd as hp
    ne_dir = write(outdir, golden_inputs, types)
    (fb, fl), ti = feeder(outdir, n, seed, types, arrangement)
    st = hp.Settings(H_MAX=hmax)
    buses, lines, m, nn, c = hp.init_network(fb, fl, settings=st)
    Y = hp.build_admittance_matrices(buses, lines, st.HARMONICS)
    NE = hp.import_Norton_Equivalents(buses, coupled, st, ne_dir)
    dev, Y_N, I_N, n_dev = ingest.norton_arrays(buses, NE, coupled, len(st.HARMONICS))
    em = Emul(nn, m, c, len(st.HARMONICS), Y.rowptr, Y.col, Y.Yval, dev, Y_N, I_N, n_dev, coupled)
    net = o.init_network(fb, fl)
    rowptr, col, Yval = o.build_admittance_matrices(net, st.HARMONICS)
    mdl = o.Model(net, st.HARMONICS, rowptr, col, Yval, o.import_Norton_Equivalents(net, st.HARMONICS, coupled, ne_dir), coupled)
    return dict(ne_dir=ne_dir, files=(fb, fl), ti=ti, st=st, buses=buses, m=m, n=nn, c=c, Y=Y, NE=NE, dev=dev, Y_N=Y_N, I_N=I_N, n_dev=n_dev, em=em,
                net=net, mdl=mdl, mats=(rowptr, col, Yval), coupled=coupled)


def oracle_states(case, iters=(0, 1, 3)):
    """states of the oracle's own iteration from its pf seed, after the given numbers of Newton steps -> [(Vm, Va)]"""
    import hpf_oracle as o
    Vm, Va, _, _ = o.pf(case["net"], *case["mats"])
    r = o.hpf_from_model(case["mdl"], Vm, Va, thresh_h=0.0, max_iter_h=max(iters), record=True)
    return [(r["traj"][it][0].copy(), r["traj"][it][1].copy()) for it in iters]
