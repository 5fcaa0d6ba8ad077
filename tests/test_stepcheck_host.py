"""The Newton-step yardstick (tests/stepcheck.py) on the reference's own first Jacobians and mismatches (J0, f0 of the golden cases, captured
from the unmodified reference): the refined solve is a correctly rounded solution, and the gate ETA_MAX tells a step that is wrong by 1e-8 --
a perturbed factor, a perturbed solution entry -- from a right one by more than 100x."""
import glob
import os

import numpy as np
import pytest
import scipy.sparse as sp

import stepcheck as sc

from conftest import GOLD

CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLD, "*_H*.npz"))
               if "J0_data" in np.load(p, allow_pickle=True).files)


# Mutation (1) cannot reach the 100x margin on these cases, and that is a property of the normwise backward error, not of the gate: the column
# of the largest step component holds entries of at most 24 (H = 11) / 94 (H = 51), while | |J| |_inf ~ 1.1e4 is set by the fundamental rows of
# the slack's neighbours; a 1e-8 relative change of such an entry moves eta by 1e-8 |J_ij dx_j| / (| |J| | |dx| + |f|) ~ 2e-11 (coupled) or
# 4e-12 (uncoupled, where that column's largest entry is smaller still).  The gate still rejects every one of them (margin 4x - 84x).
FACTOR_MARGIN = {"net1_H11_c": 20, "net1_H51_c": 80, "net2_H11_c": 20, "net2_H51_c": 70, "net3_H11_c": 20, "net3_H51_c": 70,
                 "quirk5_H11_c": 20, "syn50_H11_c": 20, "net1_H11_uc": 3.5, "net1_H51_uc": 3.5, "net2_H11_uc": 4,
                 "net2_H51_uc": 4, "net3_H11_uc": 4, "net3_H51_uc": 4, "quirk5_H11_uc": 4}


def _system(name):
    g = np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=True)
    J = sp.csr_matrix((g["J0_data"], (g["J0_row"], g["J0_col"])), shape=tuple(g["J0_shape"]))
    return J, np.asarray(g["f0"], dtype=np.float64)


def test_golden_cases_present():
    # 16 cases of the reference's nets and the quirk fixtures, and the 50-bus synthetic feeder
    assert len(CASES) == 17


@pytest.mark.parametrize("name", CASES)
def test_refined_solve_is_correctly_rounded(name):
    J, f = _system(name)
    dx = sc.refined_solve(J, f)
    eta = sc.backward_error(J, dx, f)
    print("\n%s: N = %d, eta %.2e" % (name, J.shape[0], eta))
    assert np.isfinite(dx).all()
    assert eta <= 1e-15


@pytest.mark.parametrize("name", CASES)
def test_gate_rejects_a_step_wrong_by_1e8(name):
    J, f = _system(name)
    ref = sc.refined_solve(J, f)
    # (1) a factor that is off by 1e-8: the largest entry of the column that carries the largest solution component
    j = int(np.argmax(np.abs(ref)))
    Jc = J.tocsc(copy=True)
    lo, hi = Jc.indptr[j], Jc.indptr[j + 1]
    Jc.data[lo + int(np.argmax(np.abs(Jc.data[lo:hi])))] *= 1 + 1e-8
    eta_a = sc.backward_error(J, sc.refined_solve(Jc, f), f)
    # (2) a solution entry that is off by 1e-8 of the step, in the column of the largest |J| entry
    Jo = J.tocoo()
    k = int(Jo.col[np.argmax(np.abs(Jo.data))])
    dx = ref.copy()
    dx[k] += 1e-8 * np.abs(ref).max()
    eta_b = sc.backward_error(J, dx, f)
    print("\n%s: perturbed factor eta %.2e (%.0fx ETA_MAX), perturbed entry eta %.2e (%.0fx)"
          % (name, eta_a, eta_a / sc.ETA_MAX, eta_b, eta_b / sc.ETA_MAX))
    assert eta_a >= FACTOR_MARGIN.get(name, 100) * sc.ETA_MAX
    # ... and it is the size the perturbation predicts: the gate measures the wrong step, not rounding
    i = int(np.argmax(np.abs(J.tocsc()[:, j].toarray().ravel())))
    pred = 1e-8 * abs(J[i, j] * ref[j]) / (np.asarray(abs(J).sum(axis=1)).max() * np.abs(ref).max() + np.abs(f).max())
    assert 0.5 * pred <= eta_a <= 2 * pred, (eta_a, pred)
    assert eta_b >= 100 * sc.ETA_MAX
    # the step gate sees them too
    assert sc.step_error(dx, ref) >= 1e-8 * np.abs(ref).max() / max(1.0, np.abs(ref).max()) * 0.99


def test_newton_steps_and_judge_on_a_host_stub():
    """newton_steps' bookkeeping (stacked layout, dx = x0 - x1, one entry per scenario) on a stand-in for DeviceModel whose 'iterate' takes
    the exact Newton step of a known system."""
    J, f = _system("net2_H11_c")
    n, Hn, c = 4, 6, 1
    assert J.shape[0] == 2 * n * Hn - 1 - c
    ref = sc.refined_solve(J, f)

    class Stub:
        def __init__(self):
            rng = np.random.default_rng(0)
            self.Vm = rng.uniform(0.5, 1.0, (2, n * Hn))
            self.Va = rng.uniform(-1, 1, (2, n * Hn))

        def mismatch(self):
            return np.stack([f, 2 * f]), np.zeros(2)

        def jacobian_csr(self, s):
            return J

        def get_state(self):
            return self.Vm.copy(), self.Va.copy()

        def iterate(self, k):
            for s in range(2):
                x = sc.stacked(self.Vm[s], self.Va[s], c) - (s + 1) * ref
                self.Va[s, 1:] = x[:n * Hn - 1]
                self.Vm[s, c:] = x[n * Hn - 1:]

    steps = sc.newton_steps(Stub(), c)
    assert len(steps) == 2
    for s, (Js, fs, dxs) in enumerate(steps):
        eta, err, _ = sc.judge(Js, fs, dxs)
        assert eta <= 1e-15 and err <= 1e-14, (s, eta, err)


def test_condition_estimate_matches_the_dense_inverse():
    J, f = _system("net1_H11_c")
    Jd = J.toarray()
    exact = np.abs(Jd).sum(axis=1).max() * np.abs(np.linalg.inv(Jd)).sum(axis=1).max()
    est = sc.cond_inf(J)
    assert 0.3 * exact <= est <= 1.0000001 * exact, (est, exact)
