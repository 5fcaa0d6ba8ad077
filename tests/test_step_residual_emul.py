"""The row arithmetic of the device-side residual check (csrc/hpf_assembly.hpp: step_residual_row, what k_step_residual runs per thread),
executed serially on the host against f - J dx with the J of the CSR walk (Emul.jacobian_csr).  No GPU involved.

Bound: every product is one fma into its sum, so with k stored entries in a real row the computed r differs from f - J dx by at most
(k + 1) 2^-53 (|J| |dx| + |f|); the test allows (k + 4) 2^-53, the same for the row sums of |J|."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse.linalg as spl

from conftest import GOLD, INPUTS
from emul import Emul, _p

import harmonic_power_flow_amd as hp
from harmonic_power_flow_amd import ingest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpu_emul", "residual_emul.cpp")
LIB = os.path.join(HERE, "cpu_emul", "libhpf_residual_emul.so")
HDR = os.path.join(os.path.dirname(HERE), "harmonic-power-flow_amd", "csrc", "hpf_assembly.hpp")
U53 = 2.0 ** -53

CASES = ["net1_H11_c", "net1_H11_uc", "net1_H51_c", "net3_H11_c", "net3_H11_uc", "net3_H51_c", "net3_H51_uc", "lin4_H11_c", "lin4_H11_uc"]


def _load():
    if (not os.path.exists(LIB)) or os.path.getmtime(LIB) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-mfma", "-fPIC", "-shared", "-I", os.path.dirname(HDR), SRC, "-o", LIB])
    return C.CDLL(LIB)


def _setup(name):
    net_name, hs, cs = name.split("_")
    st = hp.Settings(H_MAX=int(hs[1:]))
    coupled = cs == "c"
    buses, lines, m, n, c = hp.init_network(os.path.join(INPUTS, net_name + "_buses.csv"), os.path.join(INPUTS, net_name + "_lines.csv"), settings=st)
    Y = hp.build_admittance_matrices(buses, lines, st.HARMONICS)
    NE = hp.import_Norton_Equivalents(buses, coupled, st, INPUTS)
    dev, Y_N, I_N, n_dev = ingest.norton_arrays(buses, NE, coupled, len(st.HARMONICS))
    em = Emul(n, m, c, len(st.HARMONICS), Y.rowptr, Y.col, Y.Yval, dev, Y_N, I_N, n_dev, coupled)
    return em, buses["P"].to_numpy(float), buses["Q"].to_numpy(float)


def _residual(lib, em, Vm, Va, P, Q, dx, form):
    """(r, a, w, f) [N] of the row function; form 1: the step as a bus-major image whose non-unknown slots hold NaN (they must never be read
    into a sum)."""
    U, E = em.polar(Vm, Va)
    n, c, Hn = em.n, em.c, em.Hn
    Nc = n * Hn - 1
    N = 2 * Nc - (c - 1)
    Bst = 2 * Hn + 2
    if form:
        img = np.full((n, Bst), np.nan)
        for k in range(1, n * Hn):
            q, i = divmod(k, n)
            img[i, 2 * q] = dx[k - 1]
            if k >= c:
                img[i, 2 * q + 1] = dx[Nc + k - c]
        step = np.ascontiguousarray(img.ravel())
    else:
        step = np.ascontiguousarray(dx, np.float64)
    out = [np.zeros(N) for _ in range(4)]
    P, Q = np.ascontiguousarray(P, np.float64), np.ascontiguousarray(Q, np.float64)
    lib.emul_step_residual(*em._model_args(), _p(U.view(np.float64)), _p(E.view(np.float64)), _p(P), _p(Q), _p(step), int(form), Bst,
                           *[_p(o) for o in out])
    return out


def test_cases_cover_pv_buses_and_both_couplings():
    cs = [_setup(name)[0] for name in ("net3_H11_c", "net1_H11_uc")]
    assert cs[0].c > 1 and cs[0].coupled and not cs[1].coupled


@pytest.mark.parametrize("form", [0, 1], ids=["stacked", "bus_major"])
@pytest.mark.parametrize("name", CASES)
def test_residual_rows_equal_f_minus_J_dx(name, form):
    lib = _load()
    em, P, Q = _setup(name)
    g = np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=True)
    traj = g["V_traj"]
    rng = np.random.default_rng(7)
    worst = 0.0
    for it in sorted({0, 1, len(traj) // 2}):
        Vm, Va = traj[it][:, 0].copy(), traj[it][:, 1].copy()
        J = em.jacobian_csr(Vm, Va)
        if not np.isfinite(J.data).all():
            continue                                        # (lin4's tail: magnitudes of exactly 0, U / V_m = 0 / 0 in the reference as well)
        f = em.mismatch(Vm, Va, P, Q)
        k = np.diff(J.indptr)
        steps = [rng.standard_normal(J.shape[0]) * 10.0 ** rng.uniform(-6, 0, J.shape[0])]
        steps.append(spl.spsolve(J.tocsc(), f))
        Jl, aJ = J.astype(np.longdouble), abs(J)
        for dx in steps:
            r, a, w, f_e = _residual(lib, em, Vm, Va, P, Q, dx, form)
            assert np.array_equal(f_e, f)                   # the mismatch the solver was given, bit for bit
            scale = np.asarray(aJ @ np.abs(dx)).ravel() + np.abs(f)
            tol = (k + 4) * U53 * scale
            r_ref = f.astype(np.longdouble) - Jl @ dx.astype(np.longdouble)
            miss = np.abs(r - r_ref).astype(np.float64) - tol
            assert (miss <= 0).all(), (name, it, int(np.argmax(miss)), float(miss.max()))
            assert (np.abs(a - np.asarray(aJ @ np.abs(dx)).ravel()) <= (k + 4) * U53 * scale).all(), (name, it)
            w_ref = np.asarray(aJ.sum(axis=1)).ravel()
            assert (np.abs(w - w_ref) <= (k + 4) * U53 * w_ref).all(), (name, it)
            with np.errstate(invalid="ignore", divide="ignore"):
                worst = max(worst, float(np.nanmax(np.where(scale > 0, np.abs(r - r_ref).astype(np.float64) / (U53 * scale), 0.0))))
    print("\nRESIDUAL EMUL %-14s form %d: worst |r - (f - J dx)| = %.2f x 2^-53 (|J||dx| + |f|)" % (name, form, worst))
    assert worst > 0.0 or em.Hn == 1


@pytest.mark.parametrize("form", [0, 1], ids=["stacked", "bus_major"])
@pytest.mark.parametrize("arrangement", ["interleaved", "blocked"])
@pytest.mark.parametrize("coupled", [True, False], ids=["c", "uc"])
def test_residual_rows_with_four_device_types(coupled, arrangement, form, tmp_path):
    """The four-type 24-bus feeder of tests/multi_ne.py (H_MAX 11): step_residual_row reads Y_N of the row's own type and skips the zeros of a
    band bus as the CSR walk does, in both forms of the step, at the bound of the file."""
    import multi_ne
    lib = _load()
    case = multi_ne.host_case(tmp_path, INPUTS, arrangement=arrangement, coupled=coupled)
    em = case["em"]
    P, Q = case["buses"]["P"].to_numpy(float), case["buses"]["Q"].to_numpy(float)
    rng = np.random.default_rng(7)
    worst = 0.0
    for Vm, Va in multi_ne.oracle_states(case):
        J = em.jacobian_csr(Vm, Va)
        f = em.mismatch(Vm, Va, P, Q)
        k = np.diff(J.indptr)
        assert len(set(k[case["m"] - 1:case["m"] - 1 + em.Hn * em.n])) > (2 if coupled else 1)       # rows of several lengths
        Jl, aJ = J.astype(np.longdouble), abs(J)
        for dx in (rng.standard_normal(J.shape[0]) * 10.0 ** rng.uniform(-6, 0, J.shape[0]), spl.spsolve(J.tocsc(), f)):
            r, a, w, f_e = _residual(lib, em, Vm, Va, P, Q, dx, form)
            assert np.array_equal(f_e, f)
            scale = np.asarray(aJ @ np.abs(dx)).ravel() + np.abs(f)
            r_ref = f.astype(np.longdouble) - Jl @ dx.astype(np.longdouble)
            miss = np.abs(r - r_ref).astype(np.float64) - (k + 4) * U53 * scale
            assert (miss <= 0).all(), (int(np.argmax(miss)), float(miss.max()))
            assert (np.abs(a - np.asarray(aJ @ np.abs(dx)).ravel()) <= (k + 4) * U53 * scale).all()
            w_ref = np.asarray(aJ.sum(axis=1)).ravel()
            assert (np.abs(w - w_ref) <= (k + 4) * U53 * w_ref).all()
            with np.errstate(invalid="ignore", divide="ignore"):
                worst = max(worst, float(np.nanmax(np.where(scale > 0, np.abs(r - r_ref).astype(np.float64) / (U53 * scale), 0.0))))
    print("\nRESIDUAL EMUL four types %s %s form %d: worst |r - (f - J dx)| = %.2f x 2^-53 (|J||dx| + |f|)" % ("c" if coupled else "uc", arrangement, form, worst))
    assert worst > 0.0
