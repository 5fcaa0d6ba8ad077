"""Per-scenario source currents on the host (csrc/hpf_sources.hpp and the source pointer of csrc/hpf_assembly.hpp through tests/cpu_emul/
sources_emul.cpp; no GPU): the scale-and-shift expansion against sweep.source_currents, and the mismatch row with a source pointer against a
model that gives every nonlinear bus a device type of its own.

Bounds.  Bit for bit where both sides run the same operations on the same operands (the expansion from given cos / sin values; the mismatch).
Through each side's own sin / cos: 6 * 2^-52 * |a| * |I_N[q]| per component against the exact value -- derived, not measured: sin and cos
within 1 ulp (2 x 2^-52 relative to a factor of at most 1), one rounding each for a*c and a*s, two products and one sum (2^-53 each, together
below 4 x 2^-52 with the products' operands bounded by |a| |I_N|).  The exact value is formed in long double (64-bit mantissa) from the SAME rounded
angle (double)h * phi: the rounding of the angle belongs to the definition (hpf_sources.hpp)."""
import os

import numpy as np
import pytest

from conftest import INPUTS

import sources_emul as se

ORDERS = np.array([1, 3, 5, 7, 9, 11, 49, 99], dtype=np.int32)


def _cases(count=4000, seed=5):
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.0, 3.0, count)
    phi = rng.uniform(-np.pi, np.pi, count)
    order = rng.choice(ORDERS, count)
    i_n = (rng.normal(size=count) + 1j * rng.normal(size=count)) * 10.0 ** rng.uniform(-6, 1, count)
    a[:4], phi[:4] = [1.0, 0.0, 1.0, 2.5], [0.0, 0.3, np.pi, -0.0]
    return a, phi, order, i_n


def test_expansion_from_given_cos_and_sin_is_the_numpy_restatement_bit_for_bit():
    from harmonic_power_flow_amd import sweep
    a, phi, order, i_n = _cases()
    ang = order.astype(np.float64) * phi
    c, s = np.cos(ang), np.sin(ang)
    got = se.expand(a, phi, order, i_n, cs=(c, s))
    # one "bus" per case: scale / shift [count], I_N_bus [count][1], cs [count][1]
    ref = sweep.source_currents(i_n[:, None], a, phi, [0], cs=(c[:, None], s[:, None]))[:, 0]
    assert got.tobytes() == ref.tobytes()
    assert se.expand([1.0], [0.0], [7], [0.25 - 2j], cs=([1.0], [0.0]))[0] == 0.25 - 2j      # a = 1, phi = 0: the model's I_N itself


def test_expansion_end_to_end_is_within_the_derived_bound_of_the_exact_product():
    from harmonic_power_flow_amd import sweep
    a, phi, order, i_n = _cases()
    ang = (order.astype(np.float64) * phi).astype(np.longdouble)
    w = a.astype(np.longdouble) * (np.cos(ang) + 1j * np.sin(ang))
    exact = w * i_n.astype(np.clongdouble)
    bound = 6.0 * 2.0 ** -52 * np.abs(a) * np.abs(i_n)
    by_numpy = np.empty(len(a), dtype=np.complex128)         # (sweep.source_currents takes one order per harmonic position: group the cases by order)
    for h in np.unique(order):
        k = order == h
        by_numpy[k] = sweep.source_currents(i_n[k][:, None], a[k], phi[k], [h])[:, 0]
    worst = {}
    for name, got in (("emulation", se.expand(a, phi, order, i_n)), ("numpy", by_numpy)):
        d = got.astype(np.clongdouble) - exact
        err = np.maximum(np.abs(d.real), np.abs(d.imag)).astype(np.float64)
        worst[name] = float((err[bound > 0] / bound[bound > 0]).max())
        assert (err <= bound).all(), name
    print("\nSOURCES expansion: worst error / bound  emulation %.3f  numpy %.3f (bound = 6 * 2^-52 |a| |I_N|)" % (worst["emulation"], worst["numpy"]))


@pytest.mark.parametrize("coupled", [True, False])
def test_mismatch_with_a_source_pointer_is_the_mismatch_of_a_per_bus_device_model_bit_for_bit(tmp_path, coupled):
    """syn100 x harmonics to 11 (Hn = 6: rows q < 4 take the 4-group body of the Norton product, q = 4, 5 the tail) at the flat start and at a
    perturbed state: model A = the feeder's device types + I_src through the pointer; model B = one device type per nonlinear bus with
    I_N[type] = I_src[bus] and the Y_N of the bus's device, no pointer."""
    import hpf_oracle as o
    from harmonic_power_flow_amd import synth, sweep
    fb, fl = synth.gen(100, seed=0, outdir=str(tmp_path))
    H = o.harmonics_upto(11)
    case = se.oracle_network(fb, fl, H, coupled, INPUTS)
    net, (rowptr, col, Yval), NE = case["net"], case["mats"], case["NE"]
    n, m, c, Hn = net.n, net.m, net.c, len(H)
    names = list(NE)
    dev = np.full(n, -1, dtype=np.int32)
    dev[m:] = [names.index(net.component[i]) for i in range(m, n)]
    I_N = np.array([NE[k][0] for k in names])
    Y_N = np.array([NE[k][1] for k in names])
    a, phi = se.scale_shift(n - m, n_scen=2)
    I_src = sweep.source_currents(case["I_N_bus"], a, phi, H)
    rng = np.random.default_rng(3)
    Vm, Va = o.init_voltages(n, Hn)
    states = [(Vm, Va), (Vm * rng.uniform(0.8, 1.2, n * Hn), rng.uniform(-0.5, 0.5, n * Hn))]
    dev_b = np.full(n, -1, dtype=np.int32)
    dev_b[m:] = np.arange(n - m)
    for s in range(2):
        for vm, va in states:
            U = vm * np.exp(1j * va)
            fa = se.mismatch(n, m, c, Hn, rowptr, col, Yval, dev, Y_N, I_N, coupled, U, net.P, net.Q, src=I_src[s])
            fb_ = se.mismatch(n, m, c, Hn, rowptr, col, Yval, dev_b, Y_N[dev[m:]], I_src[s], coupled, U, net.P, net.Q)
            f0 = se.mismatch(n, m, c, Hn, rowptr, col, Yval, dev, Y_N, I_N, coupled, U, net.P, net.Q)
            assert fa.tobytes() == fb_.tobytes()
            assert np.abs(fa - f0).max() > 1e-6                       # (the sources do enter)
    # the pointer with the model's own currents = no pointer
    f1 = se.mismatch(n, m, c, Hn, rowptr, col, Yval, dev, Y_N, I_N, coupled, U, net.P, net.Q, src=case["I_N_bus"])
    assert f1.tobytes() == f0.tobytes()
