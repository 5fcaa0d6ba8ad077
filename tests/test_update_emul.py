"""csrc/hpf_update.hpp, compiled for the host (tests/update_emul.py), against the NumPy restatement (tests/update_ref.py).

10 000 random entries with c = 3: stacked indices 0..2 (the polar update: k = 0 has no dtheta either) among them, a fifth of the magnitudes
negative, angles up to +-7 (raw states are un-wrapped), dtheta up to +-20, dV up to +-2; and entries whose step takes them to U' = 0 exactly.
U'.re, U'.im and vm' are products, sums and one square root, each rounded on its own in both: bit-exact.  va' comes from two atan2
implementations, each within a few ulp of the exact angle, which lies in [-pi, pi]: 4 ulp of pi.  Entries with k < c are bit-identical to the
polar formula, the state as well as the stored U."""
import numpy as np

import update_emul as emul
import update_ref as ref

C_PV = 3
ULP_PI = 2.0 ** -51                                           # spacing of doubles in [2, 4)


def _entries(count=10000, seed=5):
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 2000, count)
    k[:300] = rng.integers(0, C_PV, 300)
    vm = rng.uniform(0.02, 1.2, count) * np.where(rng.random(count) < 0.2, -1.0, 1.0)
    va = rng.uniform(-7.0, 7.0, count)
    dth = rng.uniform(-20.0, 20.0, count)
    dth[::7] *= 1e-3
    dv = rng.uniform(-2.0, 2.0, count)
    u = vm * np.cos(va) + 1j * (vm * np.sin(va))
    e = u * (1.0 / vm)
    # U' = 0 exactly: at angle 0 and pi E = (+-1, 0), U = (+-vm, 0); dtheta = 0 and dV = vm remove U without rounding
    z = np.arange(400, 440)
    k[z] = rng.integers(C_PV, 2000, len(z))
    va[z] = 0.0
    dth[z] = 0.0
    dv[z] = vm[z]
    u[z] = vm[z] + 0j
    e[z] = 1.0 + 0j
    return k, vm, va, u, e, dth, dv


def test_the_emulation_equals_the_restatement():
    k, vm, va, u, e, dth, dv = _entries()
    got = emul.update(k, C_PV, vm, va, u, e, dth, dv)
    vm_r, va_r, tre, tim = ref.rect_update(vm, va, u, e, k, C_PV, dth, dv)
    rect = k >= C_PV
    assert rect.sum() > 9000 and (~rect).sum() >= 300 and (k == 0).any()
    assert got["target"].real[rect].tobytes() == tre[rect].tobytes()
    assert got["target"].imag[rect].tobytes() == tim[rect].tobytes()
    assert got["vm"].tobytes() == vm_r.tobytes()
    assert (got["vm"][rect] >= 0).all() and (vm[rect] < 0).any()
    d = np.abs(got["va"] - va_r)
    print("\nUPDATE emulation: largest |va' - restatement| %.3e (%.2f ulp of pi)" % (d.max(), d.max() / ULP_PI))
    assert d.max() <= 4 * ULP_PI
    assert np.abs(got["va"][rect]).max() <= np.pi
    # U' = 0
    z = rect & (tre == 0.0) & (tim == 0.0)
    assert z.sum() >= 40
    assert (got["vm"][z] == 0).all() and (got["va"][z] == 0).all() and (got["U"][z] == 0).all() and np.isfinite(got["E"][z].view(float)).all()
    # the stored U, E are polar<false> of the new state (checked against the same products formed by NumPy from the emulation's own vm', va',
    # within the libm's sin / cos: 4 ulp)
    nz = rect & ~z
    U_np = got["vm"][nz] * np.exp(1j * got["va"][nz])
    assert np.abs(got["U"][nz] - U_np).max() <= 4 * 2.0 ** -52 * np.abs(U_np).max()
    # ... and sit where the update aimed: |U - U'| within the rounding of sqrt, atan2, sin / cos and two products (16 ulp of |U'| is generous
    # for five roundings of relative size 2^-53 and three library calls of a few ulp)
    t = got["target"][nz]
    assert (np.abs(got["U"][nz] - t) <= 16 * 2.0 ** -52 * np.abs(t)).all()


def test_entries_below_c_take_the_polar_update_bit_for_bit():
    k, vm, va, u, e, dth, dv = _entries()
    low = k < C_PV
    got = emul.update(k, C_PV, vm, va, u, e, dth, dv)
    pol = emul.update(k, C_PV, vm, va, u, e, dth, dv, rectangular=False)
    vm_p, va_p = ref.polar_update(vm, va, k, C_PV, dth, dv)
    for name in ("vm", "va", "U", "E"):
        assert got[name][low].tobytes() == pol[name][low].tobytes(), name
    assert got["vm"][low].tobytes() == vm_p[low].tobytes() == vm[low].tobytes()
    assert got["va"][low].tobytes() == va_p[low].tobytes()
    assert (got["va"][k == 0] == va[k == 0]).all()            # (the slack fundamental has no unknown at all)
    assert pol["vm"].tobytes() == vm_p.tobytes() and pol["va"].tobytes() == va_p.tobytes()
    assert np.isnan(got["target"][low].real).all()
