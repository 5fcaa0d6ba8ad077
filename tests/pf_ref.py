"""The fundamental power flow of the reference (HG:195-275; oracle/hpf_oracle.py: pf) restated in plain numpy long double (test
infrastructure, like tests/stepcheck.py): the mismatch

    mis = V conj(Y1 V) + (P + jQ),   f = [Re(mis)[1:], Im(mis)[c:]]                                          (HG:196-200)

and its analytic Jacobian in the state order x = [V_a[1:], V_m[c:]] (HG:205-223), with V = V_m e^(j V_a), E = V / V_m, I = Y1 V:

    dS/dV_a = j diag(V) conj(diag(I) - Y1 diag(V)),   dS/dV_m = diag(E) conj(diag(I)) + diag(V) conj(Y1 diag(E))
    J = [[Re dS/dV_a [1:, 1:], Re dS/dV_m [1:, c:]], [Im dS/dV_a [c:, 1:], Im dS/dV_m [c:, c:]]]

Nothing here follows the oracle's operation order: it is the yardstick the device's pf assembly (hpf_fund_mismatch, hpf_fund_jacobian) and
every form of its pf Newton step are judged by, pinned to the oracle's pf in tests/test_pf_ref_host.py."""
import numpy as np

LD = np.longdouble
CLD = np.clongdouble


def dense_Y1(rowptr, col, yval, n):
    """the fundamental admittance matrix (CSR arrays, yval = the values at harmonic position 0) as a dense long-double array"""
    Y = np.zeros((n, n), dtype=CLD)
    for i in range(n):
        for e in range(rowptr[i], rowptr[i + 1]):
            Y[i, col[e]] = yval[e]
    return Y


def _phasors(Vm, Va):
    Vm, Va = np.asarray(Vm, dtype=LD), np.asarray(Va, dtype=LD)
    E = np.cos(Va) + 1j * np.sin(Va)
    return Vm * E, E


def mismatch(Y1, Vm, Va, P, Q, c):
    """-> f [2n - 1 - c] in long double; Vm, Va [n]: the fundamental voltages"""
    V, _ = _phasors(Vm, Va)
    mis = V * np.conj(Y1 @ V) + (np.asarray(P, dtype=LD) + 1j * np.asarray(Q, dtype=LD))
    return np.concatenate([mis.real[1:], mis.imag[c:]])


def jacobian(Y1, Vm, Va, c):
    """-> J [2n - 1 - c][2n - 1 - c] in long double"""
    V, E = _phasors(Vm, Va)
    I = Y1 @ V
    dSdA = 1j * V[:, None] * np.conj(np.diag(I) - Y1 * V[None, :])
    dSdV = np.diag(E * np.conj(I)) + V[:, None] * np.conj(Y1 * E[None, :])
    return np.block([[dSdA[1:, 1:].real, dSdV[1:, c:].real], [dSdA[c:, 1:].imag, dSdV[c:, c:].imag]])


def state(Vm, Va, c):
    """x = [V_a[1:], V_m[c:]] of the fundamental voltages (HG:191)"""
    return np.append(np.asarray(Va)[1:], np.asarray(Vm)[c:])


def solve(J, f, rounds=3):
    """J^-1 f: float64 LU, then `rounds` refinement steps with the residual in long double (stepcheck.refined_solve on a dense matrix)"""
    import scipy.linalg as sl
    lu = sl.lu_factor(np.asarray(J, dtype=np.float64))
    x = sl.lu_solve(lu, np.asarray(f, dtype=np.float64)).astype(LD)
    for _ in range(rounds):
        x = x + sl.lu_solve(lu, np.asarray(f - J @ x, dtype=np.float64))
    return x


def pf(Y1, P, Q, c, thresh_f=1e-6, max_iter_f=30):
    """HG:244-275 from the flat start -> (Vm [n], Va [n], err_f history, n_iter_f), all in long double"""
    n = Y1.shape[0]
    Vm, Va = np.ones(n, dtype=LD), np.zeros(n, dtype=LD)
    f = mismatch(Y1, Vm, Va, P, Q, c)
    err = np.abs(f).max() if f.size else LD(0)
    hist, it = [], 0
    while err > thresh_f and it < max_iter_f:
        x = state(Vm, Va, c) - solve(jacobian(Y1, Vm, Va, c), f)
        Va[1:] = x[:n - 1]
        Vm[c:] = x[n - 1:]
        f = mismatch(Y1, Vm, Va, P, Q, c)
        err = np.abs(f).max()
        hist.append(err)
        it += 1
    return Vm, Va, np.array(hist, dtype=LD), it
