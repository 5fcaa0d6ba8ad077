"""tests/pf_ref.py (the long-double yardstick of the fundamental power flow) pinned without a GPU: it reproduces the oracle's pf -- the
restatement of the reference's HG:195-275 that the golden vectors pin -- and its analytic Jacobian is the derivative of its own mismatch."""
import os

import numpy as np
import pytest

import pf_ref
from conftest import INPUTS


def _oracle_net(fb, fl):
    import hpf_oracle as o
    net = o.init_network(fb, fl)
    rowptr, col, Yval = o.build_admittance_matrices(net, [1])
    return o, net, rowptr, col, Yval


def _pv(fb, n_pv):
    """buses 2 .. 1 + n_pv become PV buses (the dialect of test_gpu_step_accuracy._net)"""
    rows = open(fb).read().splitlines()
    for bid in range(2, 2 + n_pv):
        cols = rows[bid].split(";")
        cols[1], cols[2], cols[4], cols[5] = "PV", "gen_%d" % bid, "-120", "0"
        rows[bid] = ";".join(cols)
    open(fb, "w").write("\n".join(rows) + "\n")


def _cases(tmp_path):
    from harmonic_power_flow_amd import synth
    yield "net1", os.path.join(INPUTS, "net1_buses.csv"), os.path.join(INPUTS, "net1_lines.csv")
    yield "net3", os.path.join(INPUTS, "net3_buses.csv"), os.path.join(INPUTS, "net3_lines.csv")
    fb, fl = synth.gen(90, seed=0, outdir=str(tmp_path))
    yield "syn90", fb, fl
    d = tmp_path / "pv"
    d.mkdir()
    fb, fl = synth.gen(90, seed=0, outdir=str(d))
    _pv(fb, 2)
    yield "syn90 2 PV", fb, fl


def test_pf_ref_reproduces_the_oracle_pf(tmp_path):
    """Iteration count equal; every entry of the err_f history within 1e-12, relative to the largest mismatch of the run (the flat start's:
    the scale the rounding of a mismatch evaluation is proportional to -- the last entries of a quadratically converging history lie
    ten orders below it and carry no more correct digits than that in either implementation); the pf state within 1e-13."""
    for name, fb, fl in _cases(tmp_path):
        o, net, rowptr, col, Yval = _oracle_net(fb, fl)
        Vm_o, Va_o, err_o, it_o = o.pf(net, rowptr, col, Yval)
        Y1 = pf_ref.dense_Y1(rowptr, col, Yval[0], net.n)
        f0 = np.abs(pf_ref.mismatch(Y1, np.ones(net.n), np.zeros(net.n), net.P, net.Q, net.c)).max()
        Vm, Va, err, it = pf_ref.pf(Y1, net.P, net.Q, net.c)
        d = np.abs(np.asarray(err, dtype=float) - np.asarray(err_o)).max() if it else 0.0
        print("\nPFREF %-12s n_iter %d (oracle %d)  |err_f - oracle| %.2e  (|f0| %.2e)  |dV| %.2e"
              % (name, it, it_o, d, f0, max(np.abs(np.asarray(Vm, dtype=float) - Vm_o[:net.n]).max(), np.abs(np.asarray(Va, dtype=float) - Va_o[:net.n]).max())))
        assert it == it_o and it > 0
        assert d <= 1e-12 * max(1.0, float(f0))
        assert np.abs(np.asarray(Vm, dtype=float) - Vm_o[:net.n]).max() <= 1e-13
        assert np.abs(np.asarray(Va, dtype=float) - Va_o[:net.n]).max() <= 1e-13


def test_pf_ref_jacobian_is_the_derivative_of_its_mismatch(tmp_path):
    """J d against the central difference (f(x + h d) - f(x - h d)) / 2h of the long-double mismatch, |d|_inf = 1, h = 1e-6.  f is a sum of
    |Y_ik| V_i conj(V_k) terms, each the product of two factors V_m e^(j V_a): its third derivative along d is at most 8 (1 + V_m)^2 <= 36
    times the row sums of |Y1| (V_m <= 1.1), so the truncation error h^2 / 6 |f'''| stays below 6e-12 |Y1|_inf; the rounding of the two
    evaluations, about 10 eps |Y1|_inf V_m^2 with eps = 1.1e-19, divided by h adds 1.3e-12 |Y1|_inf.  Bound: 1e-11 |Y1|_inf, eleven orders
    below what a wrong sign or a dropped term of J would show."""
    rng = np.random.default_rng(5)
    h = np.longdouble(1e-6)
    for name, fb, fl in _cases(tmp_path):
        o, net, rowptr, col, Yval = _oracle_net(fb, fl)
        n, c = net.n, net.c
        Y1 = pf_ref.dense_Y1(rowptr, col, Yval[0], n)
        ynorm = float(np.abs(Y1).sum(axis=1).max())
        Vm = np.ones(n, dtype=np.longdouble)
        Va = np.zeros(n, dtype=np.longdouble)
        Vm[1:] = rng.uniform(0.9, 1.1, n - 1)
        Va[1:] = rng.uniform(-0.3, 0.3, n - 1)
        J = pf_ref.jacobian(Y1, Vm, Va, c)
        assert J.shape == (2 * n - 1 - c, 2 * n - 1 - c) and J.dtype == np.longdouble
        worst = 0.0
        for _ in range(4):
            d = rng.choice([-1.0, 1.0], size=2 * n - 1 - c).astype(np.longdouble) * rng.uniform(0.2, 1.0, 2 * n - 1 - c)
            d[0] = 1.0

            def at(t):
                vm, va = Vm.copy(), Va.copy()
                va[1:] += t * d[:n - 1]
                vm[c:] += t * d[n - 1:]
                return pf_ref.mismatch(Y1, vm, va, net.P, net.Q, c)
            fd = (at(h) - at(-h)) / (2 * h)
            worst = max(worst, float(np.abs(J @ d - fd).max()))
        print("\nPFREF %-12s |J d - central difference| %.2e  (bound %.2e)" % (name, worst, 1e-11 * ynorm))
        assert worst <= 1e-11 * ynorm
        # and a wrong sign is seen: flipping one entry of J misses the bound by orders
        k = int(np.argmax(np.abs(J[0])))
        Jw = J.copy()
        Jw[0, k] = -Jw[0, k]
        dk = np.zeros(2 * n - 1 - c, dtype=np.longdouble)
        dk[k] = 1.0
        assert float(np.abs((Jw - J) @ dk).max()) > 1e6 * 1e-11 * ynorm
