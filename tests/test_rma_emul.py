"""Resonance mode analysis without a GPU: the host emulation (tests/rma_emul.py: the functions of csrc/hpf_resonance.hpp in the kernels' order)
against numpy.linalg.eig of zscan_ref.dense_Y, bit-identity of every output across chunk lengths, and the stand-alone sanitizer program.

The grid is 130 points on 0.5 .. 50.5, iters = 64.  A point is compared only where the reference's two smallest eigenvalues satisfy
|lam1 / lam2| <= 0.5 (inverse iteration converges by that ratio per step); all 130 points of each of the seven shapes must qualify.  Bounds,
derived and not tuned (eps = 2^-52, V the reference's eigenvector matrix with unit columns):
  eigenvalue      |lam - lam1| / |lam1| <= 4 eps kappa_2(Y) kappa_2(V)        first order: the tree solve perturbs Y^-1 by eps kappa_2(Y) relative, an
                                                                            eigenvalue moves by at most kappa_2(V) times that (Bauer-Fike); two
                                                                            computations of the same quantity each get twice the first-order bound
  participation   max_i |pf_i - pf_ref,i| <= 4 eps ||Y||_2 kappa_2(V) / min_{j != 1} |lam_j - lam1|     the eigenvector's first-order bound
  residual        res <= 1e-12        (0.5^64 = 5e-20: only rounding is left at 64 steps)
  normalisation   |sum_i pf_i - 1| <= n 2^-50
Shares of the two bounds used by the emulation (printed by the test): see the table there."""
import os

import numpy as np
import pytest

import rma_emul as rm
import zscan_emul as ze

SHAPES = ["n2", "chain9", "chain33", "chain65", "syn12", "syn40", "net1"]
ITERS = 64

_RUNS = {}


def _case(name, iters=ITERS):
    """-> model, y_extra, (code, outputs) of the emulation with the automatic chunk; computed once and shared (left unchanged)"""
    if (name, iters) not in _RUNS:
        model, banks = rm.shape(name)
        yx = rm.y_extra(model, rm.GRID, banks)
        _RUNS[name, iters] = (model, yx, rm.modes(model, rm.GRID, yx, iters))
    return _RUNS[name, iters]


@pytest.mark.parametrize("name", SHAPES)
def test_emulation_matches_the_dense_eigenpair(name):
    model, yx, (rc, out) = _case(name)
    n = int(model["n"])
    assert rc == 0
    if name == "net1":
        assert len(ze.plan(model)[3]) == 4
    d = rm.dense(name)
    print(name, "worst |lam1 / lam2| %.3f" % d["gap"].max())
    assert np.all(d["gap"] <= 0.5), d["gap"].max()          # every point qualifies
    s_lam, s_pf = rm.bound_shares(out, d)
    print(name, "share of the eigenvalue bound used %.3g, of the participation bound %.3g; max |pf - pf_ref| %.3g; max res %.3g"
          % (s_lam.max(), s_pf.max(), np.abs(out["pf"] - d["pf"]).max(), out["res"].max()))
    assert np.all(s_lam <= 1.0), s_lam.max()
    assert np.all(s_pf <= 1.0), s_pf.max()
    assert np.all(out["res"] <= 1e-12), out["res"].max()
    assert np.all(np.abs(out["pf"].sum(axis=1) - 1.0) <= n * 2.0 ** -50)
    assert np.allclose(out["zm"], 1.0 / np.abs(out["lam"]), rtol=1e-14, atol=0.0)
    assert np.array_equal(out["top"], np.abs(out["pf"]).argmax(axis=1))


@pytest.mark.parametrize("name", SHAPES)
def test_thirty_two_steps_resolve_every_point_of_these_shapes(name):
    """The basis of the Python default iters = 32 and of converged(tol = 1e-8): the error falls by |lam1 / lam2| <= 0.5 per step, 0.5^32 = 2.3e-10,
    which leaves a factor of 43 for the start vector's share of the other modes"""
    rc, out = _case(name, 32)[2]
    print(name, "max res at 32 steps %.3g" % out["res"].max())
    assert rc == 0 and np.all(out["res"] <= 1e-8)


@pytest.mark.parametrize("name", SHAPES + ["n1", "star9"])
def test_every_output_is_bit_identical_for_every_chunk_length(name):
    model, banks = rm.shape(name)
    yx = rm.y_extra(model, rm.GRID, banks)
    for iters in (1, 5):
        rc, base = rm.modes(model, rm.GRID, yx, iters)
        for chunk in (1, 17, 64, 129):
            rc2, got = rm.modes(model, rm.GRID, yx, iters, chunk)
            assert rc2 == rc
            for key in rm.OUTPUTS:
                assert rm.same(got[key], base[key]), (name, iters, chunk, key)
        rc3, peaks_only = rm.modes(model, rm.GRID, yx, iters, 17, full=False)
        assert rc3 == rc and peaks_only["pf"] is None and all(rm.same(peaks_only[k], base[k]) for k in rm.OUTPUTS[:4])


def test_one_step_is_the_solve_of_the_start_vector():
    """iters = 1: y = Y^-1 x0, x0_i = 1 + i / n; lam = (x0 . x0) / (x0 . y), top = argmax |y|"""
    import zscan_ref as ref
    model, _ = rm.shape("chain33")
    n = 33
    rc, out = rm.modes(model, rm.GRID[:5], None, 1)
    x0 = 1.0 + np.arange(n) / n
    for f, h in enumerate(rm.GRID[:5]):
        y = np.linalg.solve(ref.dense_Y(model, h), x0)
        assert abs(out["lam"][f] - (x0 @ x0) / (x0 @ y)) <= 1e-10 * abs(out["lam"][f])
        assert out["top"][f] == np.abs(y).argmax()
        assert np.abs(out["pf"][f] - y * y / (y @ y)).max() <= 1e-10


def test_a_singular_admittance_is_reported_with_the_outputs_written():
    model = ze.raw_model(1, [], xsh0=0.005)                   # xsh only: Y = 0 at h = 1
    rc, out = rm.modes(model, np.array([0.5, 1.0, 2.0]), None, 3)
    assert rc == 3 and out["top"].tolist() == [0, 0, 0]
    assert np.isfinite(out["lam"][[0, 2]]).all() and not np.isfinite(out["zm"][1])
    assert np.allclose(out["lam"][[0, 2]], [-1j / (0.005 * 0.5), -1j / (0.005 * 2.0)]) and np.allclose(out["pf"][[0, 2], 0], 1.0)


def test_emulation_under_asan_ubsan(tmp_path):
    """tests/cpu_emul/rma_main.cpp: a stand-alone program, exactly sized buffers, on the CPU"""
    import subprocess
    exe = str(tmp_path / "rma.bin")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", ze.CSRC, os.path.join(ze.HERE, "cpu_emul", "rma_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "rma clean" in r.stdout
