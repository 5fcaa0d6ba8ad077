"""The yardstick of a Newton step: SciPy's SuperLU (the reference's solver, HG:478) plus iterative refinement with a long-double residual, and
the backward error of any step against it.  Test infrastructure only (like tests/emul.py): the GPU paths are judged by what they return for the
SAME J and f, never by another GPU path."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spl

ETA_MAX = 1e-12              # bound of the normwise backward error of a step: ~4 500 unit roundoffs
STEP_MAX = 1e-9              # bound of |dx - dx_ref|_inf / max(1, |dx_ref|_inf), the normalisation of the existing step gates
REFINE_ROUNDS = 3


def _ld(J):
    return J.astype(np.longdouble)


def residual_ld(J, dx, f):
    """f - J dx accumulated in long double (scipy's CSR matvec runs in the operand type)."""
    return np.asarray(f, dtype=np.longdouble) - _ld(J) @ np.asarray(dx, dtype=np.longdouble)


def refined_solve(J, f, lu=None, rounds=REFINE_ROUNDS):
    """splu, then `rounds` refinement steps x <- x + LU^-1 (f - J x) with the residual in long double -> dx_ref (float64).  `lu` may be a
    factorisation of J kept by the caller (one per matrix)."""
    J = sp.csr_matrix(J)
    if lu is None:
        lu = spl.splu(J.tocsc())
    x = lu.solve(np.asarray(f, dtype=np.float64))
    for _ in range(rounds):
        x = x + lu.solve(np.asarray(residual_ld(J, x, f), dtype=np.float64))
    return x


def backward_error(J, dx, f):
    """eta = |f - J dx|_inf / (| |J| |_inf |dx|_inf + |f|_inf), in long double."""
    J = sp.csr_matrix(J)
    r = np.abs(residual_ld(J, dx, f)).max()
    absJ = np.asarray(abs(_ld(J)).sum(axis=1)).ravel().max()
    den = absJ * np.abs(np.asarray(dx, dtype=np.longdouble)).max() + np.abs(np.asarray(f, dtype=np.longdouble)).max()
    return float(r / den) if den > 0 else float(r)


def step_error(dx, dx_ref):
    """|dx - dx_ref|_inf / max(1, |dx_ref|_inf)."""
    return float(np.abs(np.asarray(dx) - np.asarray(dx_ref)).max() / max(1.0, float(np.abs(dx_ref).max())))


def stacked(Vm, Va, c):
    """The reference's state vector x = [V_a[1:], V_m[c:]] (HG:393-398) of one scenario."""
    return np.append(Va[1:], Vm[c:])


def newton_steps(dm, c):
    """One Newton step of every scenario of the DeviceModel's batch from its current state -> [(J_s, f_s, dx_s)]: f from hpf_mismatch, J from
    hpf_jacobian_csr (pinned to the reference's J0 at 1e-12), dx = x0 - x1 across hpf_iterate(1).  hpf_get_state does not wrap angles."""
    f, _ = dm.mismatch()
    S = f.shape[0]
    Js = [dm.jacobian_csr(s) for s in range(S)]
    Vm0, Va0 = dm.get_state()
    dm.iterate(1)
    Vm1, Va1 = dm.get_state()
    return [(Js[s], f[s].copy(), stacked(Vm0[s], Va0[s], c) - stacked(Vm1[s], Va1[s], c)) for s in range(S)]


def cond_inf(J, lu=None):
    """kappa_inf(J) = | |J| |_inf |J^-1|_inf, the inverse's norm estimated (scipy onenormest on J^-T, one factorisation).  Reported next to a
    step that misses STEP_MAX; never part of a gate."""
    J = sp.csr_matrix(J)
    if lu is None:
        lu = spl.splu(J.tocsc())
    N = J.shape[0]
    op = spl.LinearOperator((N, N), matvec=lambda v: lu.solve(np.asarray(v, dtype=np.float64).ravel(), trans="T"),
                            rmatvec=lambda v: lu.solve(np.asarray(v, dtype=np.float64).ravel()), dtype=np.float64)
    return float(np.asarray(abs(J).sum(axis=1)).max() * spl.onenormest(op))


def judge(J, f, dx, lu=None):
    """(eta, step error, dx_ref) of the step dx of the system J dx = f."""
    ref = refined_solve(J, f, lu=lu)
    return backward_error(J, dx, f), step_error(dx, ref), ref
