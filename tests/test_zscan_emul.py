"""Impedance scan without a GPU: admittance.line_model against the package's own admittance matrices, the host emulation of the scan
(tests/zscan_emul.py: the functions of csrc/hpf_zscan.hpp in the kernels' order) against the references of tests/zscan_ref.py, and the host
argument checks of hpf_impedance_scan through libhpf.so.

Bound of every comparison of impedances: the error, relative to max_i |Z_ii| of the frequency point, is at most 2^-52 kappa_2(Y(h)) -- the
forward-error scale of a backward-stable solve; derived, not tuned.  So that the bound hides nothing, kappa_2 <= 1e7 is asserted at every point
of every grid used here."""
import ctypes as C
import os

import numpy as np
import pytest

import zscan_emul as ze
import zscan_ref as ref

GRID = np.linspace(0.5, 50.5, 257)
KAPPA_MAX = 1e7


def _hp():
    import harmonic_power_flow_amd as hp
    return hp


def _feeder12_with_line_shunts(tmp_path):
    from harmonic_power_flow_amd import synth
    fb, fl = synth.gen(12, seed=0, outdir=str(tmp_path))
    rows = open(fl).read().splitlines()
    out = [rows[0]]
    for k, r in enumerate(rows[1:]):
        c = r.split(";")
        c[5], c[6] = "%.6g" % (2e-5 * (k + 1)), "%.6g" % (3e-4 * (1 + k % 3))
        out.append(";".join(c))
    open(fl, "w").write("\n".join(out) + "\n")
    return fb, fl


@pytest.mark.parametrize("net", ["net1", "net2", "syn12_GB"])
def test_line_model_reproduces_the_admittance_matrices(net, tmp_path):
    hp = _hp()
    from harmonic_power_flow_amd import admittance
    st = hp.Settings()
    if net == "syn12_GB":
        fb, fl = _feeder12_with_line_shunts(tmp_path)
    else:
        fb, fl = os.path.join(ze.INPUTS, net + "_buses.csv"), os.path.join(ze.INPUTS, net + "_lines.csv")
    buses, lines, m, n, c = hp.init_network(fb, fl, settings=st)
    model = admittance.line_model(buses, lines)
    if net == "syn12_GB":
        assert np.any(model["gsh"] != 0) and np.any(model["bsh"] != 0) and model["gsh"][0] == 0 and model["bsh"][0] == 0
    harmonics = list(st.HARMONICS)[1:]
    Y = hp.build_admittance_matrices(buses, lines, harmonics)
    from branch_ref import branches
    fr, to, _ = branches(Y.rowptr, Y.col)
    assert np.array_equal(fr, model["fr"]) and np.array_equal(to, model["to"]) and model["nb"] == len(fr)
    for h in harmonics:
        want, got = Y.dense(h), ref.dense_Y(model, float(h))
        rowmax = np.abs(want).max(axis=1, keepdims=True)
        assert np.all(np.abs(got - want) <= 4 * np.spacing(rowmax)), (net, h, float((np.abs(got - want) / np.spacing(rowmax)).max()))


def _radial_cases():
    syn12 = ze.network("syn12")["model"]
    syn40 = ze.network("syn40")["model"]
    return {"chain9": (ze.chain(9), None), "star9": (ze.star(9), None),
            "syn12_caps": (syn12, ze.capacitors(syn12, GRID, {5: 0.002, 9: 0.02})),
            "syn40_cap": (syn40, ze.capacitors(syn40, GRID, {17: 0.01}))}


def _rel_err(Z, Zref):
    """max over the buses of |Z - Zref|, relative to max_i |Zref_ii| of the point -> [F]"""
    Zref = np.asarray(Zref)
    return (np.abs(Z - Zref).max(axis=1) / np.abs(Zref).max(axis=1)).astype(float)


@pytest.mark.parametrize("case", ["chain9", "star9", "syn12_caps", "syn40_cap"])
def test_emulation_matches_the_longdouble_recurrence_on_radial_feeders(case):
    model, yx = _radial_cases()[case]
    rc, Z, _, zpeak, fpeak = ze.scan(model, GRID, yx)
    assert rc == 0
    Zl = ref.tree_scan_longdouble(model, GRID, yx)
    Zd, kappa, _ = ref.dense_scan(model, GRID, yx)
    assert kappa.max() <= KAPPA_MAX, kappa.max()
    err = _rel_err(Z.astype(np.clongdouble), Zl)
    print(case, "kappa max %.3g" % kappa.max(), "share of the bound used %.3g" % (err / (ref.EPS * kappa)).max())
    assert np.all(err <= ref.EPS * kappa)
    # the longdouble recurrence and the dense inverse are the same function
    assert np.all(_rel_err(np.diagonal(Zd, axis1=1, axis2=2), Zl.astype(np.complex128)) <= 4 * ref.EPS * kappa)
    a = np.sqrt(Z.real * Z.real + Z.imag * Z.imag)            # (every operation rounded on its own, like the header's)
    assert np.array_equal(zpeak, a.max(axis=0)) and np.array_equal(fpeak, a.argmax(axis=0))


def test_emulation_matches_the_dense_inverse_on_net1_with_its_four_ties():
    model = ze.network("net1")["model"]
    parent, pbranch, depth, ties = ze.plan(model)
    assert len(ties) == 4 and model["nb"] == model["n"] - 1 + 4
    rc, Z, _, _, _ = ze.scan(model, GRID)
    assert rc == 0
    Zd, kappa, _ = ref.dense_scan(model, GRID)
    assert kappa.max() <= KAPPA_MAX, kappa.max()
    err = _rel_err(Z, np.diagonal(Zd, axis1=1, axis2=2))
    print("net1 kappa max %.3g" % kappa.max(), "share of the bound used %.3g" % (err / (ref.EPS * kappa)).max())
    assert np.all(err <= ref.EPS * kappa)


@pytest.mark.parametrize("case", ["syn12_caps", "net1", "ring6"])
def test_transfer_columns(case):
    if case == "net1":
        model, yx = ze.network("net1")["model"], None
    elif case == "ring6":
        model, yx = ze.raw_model(6, [(i, (i + 1) % 6) for i in range(6)] + [(1, 4)]), None
    else:
        model, yx = _radial_cases()[case]
    n = model["n"]
    parent, _, depth, _ = ze.plan(model)
    leaf = int(max(range(n), key=lambda i: (depth[i], i)))
    inner = int(parent[leaf])
    sel = [0, leaf, inner]
    rc, Z, Zt, _, _ = ze.scan(model, GRID, yx, sel)
    assert rc == 0
    Zd, kappa, Y = ref.dense_scan(model, GRID, yx)
    assert kappa.max() <= KAPPA_MAX
    bound = ref.EPS * kappa
    scale = np.abs(np.diagonal(Zd, axis1=1, axis2=2)).max(axis=1)
    for s, j in enumerate(sel):
        res = np.einsum("fik,fk->fi", Y, Zt[:, s, :])
        res[:, j] -= 1
        assert np.all(np.abs(res).max(axis=1) <= bound), (case, j, float((np.abs(res).max(axis=1) / bound).max()))
        assert np.array_equal(Zt[:, s, j].copy().view(np.uint64), Z[:, j].copy().view(np.uint64))
        assert np.all(np.abs(Zt[:, s, :] - Zd[:, :, j]).max(axis=1) / scale <= bound)
    for s, j in enumerate(sel):
        for s2, j2 in enumerate(sel):
            assert np.all(np.abs(Zt[:, s, j2] - Zt[:, s2, j]) / scale <= bound)


def test_emulation_does_not_depend_on_the_chunk_length_and_folds_peaks_across_chunks():
    model = ze.network("net1")["model"]
    h = np.concatenate([GRID[:130], GRID[40:60]])             # repeated points: equal values in different chunks
    base = ze.scan(model, h, None, [0, 7], 0)
    for chunk in (64, 17, 1):
        got = ze.scan(model, h, None, [0, 7], chunk)
        for a, b in zip(base[1:], got[1:]):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    a = np.sqrt(base[1].real * base[1].real + base[1].imag * base[1].imag)
    assert np.array_equal(base[4], a.argmax(axis=0))           # ties go to the smallest grid index
    assert base[4].max() < 130


def test_a_floating_network_is_reported_singular_with_the_outputs_written():
    model = ze.raw_model(1, [], xsh0=0.0)
    rc, Z, _, zpeak, fpeak = ze.scan(model, np.array([0.5, 1.0, 2.0]))
    assert rc == 3 and not np.isfinite(zpeak[0]) and fpeak[0] == 0


def test_planner_and_emulation_under_asan_ubsan(tmp_path):
    """tests/cpu_emul/zscan_main.cpp: a stand-alone program, exactly sized buffers, on the CPU"""
    import subprocess
    exe = str(tmp_path / "zscan.bin")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", ze.CSRC, os.path.join(ze.HERE, "cpu_emul", "zscan_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "zscan clean" in r.stdout


# ---- hpf_impedance_scan: host checks through libhpf.so, before any HIP call ------------------------------------------------------------------
def _call(model, h, y_extra=None, sel=(), chunk=0, nulls=(), F=None, n_sel=None):
    from harmonic_power_flow_amd import _lib
    lib = _lib.load()
    ip, dp = _lib.c_int_p, _lib.c_dbl_p
    n = int(model["n"])
    a = {k: np.ascontiguousarray(model[k], dtype=np.int32 if k in ("fr", "to") else np.float64) for k in ("fr", "to", "R", "X", "gsh", "bsh", "xsh")}
    ptr = {k: (None if k in nulls else v.ctypes.data_as(ip if k in ("fr", "to") else dp)) for k, v in a.items()}
    net = _lib.hpf_zscan_net(n, int(model["nb"]), ptr["fr"], ptr["to"], ptr["R"], ptr["X"], ptr["gsh"], ptr["bsh"], ptr["xsh"])
    h = np.ascontiguousarray(h, dtype=np.float64)
    F = len(h) if F is None else F
    sel = np.ascontiguousarray(sel, dtype=np.int32)
    n_sel = len(sel) if n_sel is None else n_sel
    yx = None if y_extra is None else np.ascontiguousarray(y_extra, dtype=np.complex128)
    Z = np.empty((max(len(h), 1), n), dtype=np.complex128)
    Zt = np.empty((max(len(h), 1), max(len(sel), 1), n), dtype=np.complex128)
    zp, fp = np.empty(n), np.empty(n, dtype=np.int32)
    return lib.hpf_impedance_scan(0, None if "net" in nulls else C.byref(net), F, None if "h" in nulls else h.ctypes.data_as(dp),
                                  None if yx is None else yx.ctypes.data_as(dp), n_sel, sel.ctypes.data_as(ip), chunk, Z.ctypes.data_as(dp),
                                  None if "Zt" in nulls else Zt.ctypes.data_as(dp), zp.ctypes.data_as(dp), fp.ctypes.data_as(ip))


def test_impedance_scan_checks_its_arguments_on_the_host():
    ring = ze.raw_model(4, [(0, 1), (1, 2), (2, 3), (0, 3)])
    h = np.array([0.5, 2.0, 3.0])
    assert _call(ring, h) not in (-1, -3)                      # a valid ring passes the analysis (no GPU here: the first HIP call ends it)
    assert _call(ring, h, nulls=("net",)) == -1
    assert _call(ring, h, nulls=("h",)) == -1
    assert _call(dict(ring, n=0), h) == -1
    assert _call(ring, h, F=0) == -1
    assert _call(ring, h, F=2 ** 20 + 1) == -1

    def with_(**kw):
        m = {k: np.array(v, copy=True) if isinstance(v, np.ndarray) else v for k, v in ring.items()}
        for k, (pos, val) in kw.items():
            m[k][pos] = val
        return m
    assert _call(with_(fr=(1, 3)), h) == -1                    # from == to
    assert _call(with_(fr=(2, 3), to=(2, 2)), h) == -1         # from > to
    assert _call(with_(to=(3, 4)), h) == -1                    # end bus outside 0 .. n-1
    assert _call(with_(fr=(0, -1)), h) == -1
    assert _call(with_(fr=(3, 0), to=(3, 1)), h) == -1         # duplicate pair (0, 1)
    assert _call(with_(R=(1, 0.0), X=(1, 0.0)), h) == -1       # R = X = 0
    for key in ("R", "X", "gsh", "bsh", "xsh"):
        for bad in (np.nan, np.inf):
            assert _call(with_(**{key: (0, bad)}), h) == -1
    for bad in (np.nan, np.inf, 0.0, -1.0):
        assert _call(ring, np.array([0.5, bad, 3.0])) == -1    # non-finite h, h <= 0
    yx = np.zeros((3, 4), dtype=np.complex128)
    yx[1, 2] = complex(0.0, np.nan)
    assert _call(ring, h, y_extra=yx) == -1
    assert _call(ring, h, sel=[4]) == -1
    assert _call(ring, h, sel=[-1]) == -1
    assert _call(ring, h, n_sel=-1) == -1
    assert _call(ring, h, sel=[0] * 65) == -1
    assert _call(ring, h, sel=[0], nulls=("Zt",)) == -1
    assert _call(ring, h, chunk=-1) == -1
    assert _call(ring, h, sel=[0] * 64, chunk=2) not in (-1, -3)


def test_impedance_scan_classifies_the_topology_on_the_host():
    h = np.array([0.5, 2.0])
    assert _call(ze.raw_model(4, [(0, 1), (2, 3)]), h) == -3                              # not connected from bus 0
    assert _call(ze.raw_model(2, []), h) == -3
    ring10 = [(i, i + 1) for i in range(9)] + [(0, 9)]
    chords = [(0, 2), (1, 3), (2, 4), (3, 5), (4, 6), (5, 7), (6, 8), (7, 9)]
    assert _call(ze.raw_model(10, ring10 + chords[:7]), h) not in (-1, -3)                # 8 ties
    assert _call(ze.raw_model(10, ring10 + chords), h) == -3                              # 9 ties
    assert ze.plan(ze.raw_model(10, ring10 + chords)) == -3
    assert len(ze.plan(ze.raw_model(10, ring10 + chords[:7]))[3]) == 8
