"""NumPy restatement of the state update of the harmonic Newton loop (csrc/hpf_update.hpp; include/hpf.h, option "rectangular_update";
DESIGN.md 6.4), and a Newton loop with the rectangular update built from the CPU oracle's own functions (oracle/hpf_oracle.py is imported,
not modified).  Test infrastructure only.

Entry (bus i, harmonic position q), stacked index k = q*n + i, state (vm, va), U = vm e^(j va), E = U / vm, step (dtheta, dV):
  k <  c: va' = va - dtheta (k >= 1), vm' = vm                                   (the reference's update, HG:484-485)
  k >= c: b = vm dtheta, dU = (E.re dV - E.im b, E.re b + E.im dV), U' = U - dU, vm' = sqrt(U'.re^2 + U'.im^2), va' = atan2(U'.im, U'.re)
          (U' = 0: vm' = 0, va' = 0)
NumPy's real element-wise ufuncs round every product and sum on their own, like the library (-ffp-contract=off)."""
import numpy as np


def polar_update(vm, va, k, c, dth, dv):
    """the reference's update of entries with stacked indices k -> (vm', va')"""
    return np.where(k >= c, vm - dv, vm), np.where(k >= 1, va - dth, va)


def rect_target(vm, u, e, dth, dv):
    """U' (re, im) of every entry, from its state and the U, E the handle holds for it"""
    b = vm * dth
    dre = e.real * dv - e.imag * b
    dim = e.real * b + e.imag * dv
    return u.real - dre, u.imag - dim


def rect_update(vm, va, u, e, k, c, dth, dv):
    """-> (vm', va', U'.re, U'.im); U' of the entries with k < c is NaN (they take the polar update)"""
    vm, va, dth, dv = (np.asarray(a, dtype=np.float64) for a in (vm, va, dth, dv))
    tre, tim = rect_target(vm, u, e, dth, dv)
    vr = np.sqrt(tre * tre + tim * tim)
    ar = np.where(vr == 0.0, 0.0, np.arctan2(tim, tre))
    vp, ap = polar_update(vm, va, k, c, dth, dv)
    rect = k >= c
    return np.where(rect, vr, vp), np.where(rect, ar, ap), np.where(rect, tre, np.nan), np.where(rect, tim, np.nan)


def split_step(dx, n, Hn, c):
    """the stacked Newton step dx [N] -> (dtheta [n*Hn], dV [n*Hn]) with zeros where the entry has no such unknown"""
    Nc = n * Hn - 1
    dth, dv = np.zeros(n * Hn), np.zeros(n * Hn)
    dth[1:] = dx[:Nc]
    dv[c:] = dx[Nc:]
    return dth, dv


def apply_step(Vm, Va, dx, n, Hn, c, rectangular=True):
    """one update of a whole state [n*Hn] (stacked order) with U, E formed as the library forms them (U = vm e^(j va), E = U (1 / vm))"""
    k = np.arange(n * Hn)
    dth, dv = split_step(dx, n, Hn, c)
    if not rectangular:
        return polar_update(Vm, Va, k, c, dth, dv)
    u = Vm * np.cos(Va) + 1j * (Vm * np.sin(Va))
    e = u * (1.0 / Vm)
    return rect_update(Vm, Va, u, e, k, c, dth, dv)[:2]


def hpf_rect_from_model(o, mdl, Vm, Va, thresh_h=1e-4, max_iter_h=50):
    """hpf_oracle.hpf_from_model with the update replaced: mismatch, Jacobian and linear solve are the oracle's own (o = the imported
    hpf_oracle module); the step dx = J^-1 f is applied in rectangular form to the entries with k >= c.  Vm, Va modified in place."""
    n_iter = 0
    f, err = o.harmonic_mismatch(mdl, Vm, Va)
    hist = [err]
    zero = np.zeros(mdl.N)
    while err > thresh_h and n_iter < max_iter_h:
        J = o.build_harmonic_jacobian(mdl, Vm, Va)
        dx = -o.update_harmonic_state_vec(J, zero, f)                    # (0 - J^-1 f: exact negation)
        Vm[:], Va[:] = apply_step(Vm, Va, dx, mdl.n, mdl.Hn, mdl.c)
        f, err = o.harmonic_mismatch(mdl, Vm, Va)
        hist.append(err)
        n_iter += 1
    return {"Vm_raw": Vm, "Va_raw": Va, "err_h": err, "n_iter_h": n_iter, "err_hist": np.array(hist)}
