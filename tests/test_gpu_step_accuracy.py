"""Every Newton-step path of the library judged against the yardstick of tests/stepcheck.py -- SuperLU + long-double iterative refinement on
the SAME J (hpf_jacobian_csr, pinned to the reference's J0) and f -- instead of against another GPU path: the fused block-tree step at every
block width 2 ... 112 (coupled) and at the widths around the padding classes 12 / 28 / 52 / 100 / 112 (uncoupled), each build switch of hpf_create,
meshed feeders in each bordered form, the dense rocSOLVER path, and hpf_sparse_solve (up to its own limit, b = 128).  Fixed-point tests
cannot see a wrong step (Newton absorbs it); these gates do: eta <= ETA_MAX (normwise backward error) and |dx - dx_ref| <= STEP_MAX
max(1, |dx_ref|), per scenario, at the pf seed (large first steps) and after 3 Newton iterations (small f).  Every case prints its worst eta
and step error."""
import ctypes as C

import numpy as np
import pytest

import stepcheck as sc

from conftest import INPUTS

pytestmark = pytest.mark.gpu

ETA_MAX = sc.ETA_MAX
STEP_MAX = sc.STEP_MAX
N_BUS = 90
SEED = 0
S = 3


def _hp():
    import harmonic_power_flow_amd as hp
    return hp


def _net(tmp_path, n, hmax, seed=SEED, coupled=True, frac_nl=0.35, n_pv=0, ties=0, pv_p="-120", ne_dir=INPUTS, files=None):
    """A synthetic feeder (synth.gen; files=(buses.csv, lines.csv): that radial feeder instead), optionally with PV buses (IDs 2.., the dialect
    of tools/fuzz_parity.py) and k loop-closing lines; Norton tables from ne_dir (the 64-harmonic one of tests/wide_ne.py for b > 100)."""
    hp = _hp()
    from harmonic_power_flow_amd import synth
    fb, fl = files or synth.gen(n, seed=seed, frac_nl=frac_nl, outdir=str(tmp_path))
    if ties:
        synth.add_ties(fl, n, ties, seed=seed)
    if n_pv:
        rows = open(fb).read().splitlines()
        for bid in range(2, 2 + n_pv):
            cols = rows[bid].split(";")
            cols[1], cols[2], cols[4], cols[5] = "PV", "gen_%d" % bid, pv_p, "0"
            rows[bid] = ";".join(cols)
        open(fb, "w").write("\n".join(rows) + "\n")
    st = hp.Settings(H_MAX=hmax)
    buses, lines, m, nn, c = hp.init_network(fb, fl, settings=st)
    Y = hp.build_admittance_matrices(buses, lines, st.HARMONICS)
    NE = hp.import_Norton_Equivalents(buses, coupled, st, ne_dir)
    return dict(st=st, buses=buses, Y=Y, NE=NE, c=c, n=nn, coupled=coupled, fb=fb, fl=fl)


def _scales(n, S_):
    from harmonic_power_flow_amd import synth
    return np.stack([synth.scenario_scale(n, s) for s in range(S_)])


def _run(net, S_=S, cap=None, solver="block_tree", options=None, set_opts=(), converge=True, states=("seed", "iter3")):
    """One handle (capacity `cap`, batch of S_ scenarios with synth.scenario_scale loads): converge under dm.solve, then from the pf seed the
    Newton steps of every scenario at the seed and after 3 iterations -> {state: [(J, f, dx, Vm, Va, err)]}, census."""
    from harmonic_power_flow_amd import api
    st, buses, c = net["st"], net["buses"], net["c"]
    n = len(buses)
    dm = api._device_model(buses, net["Y"], net["NE"], net["coupled"], st.HARMONICS, solver=solver, max_scenarios=cap or S_, options=options)
    out = {}
    try:
        for k, v in set_opts:
            dm.set_option(k, v)
        sc_ = _scales(n, S_)
        dm.set_loads(buses["P"].to_numpy(float) * sc_, buses["Q"].to_numpy(float) * sc_)
        dm.set_state(None, None, n_scen=S_)
        dm.fund_pf(1e-6, 30)
        seed = dm.get_state()
        if converge:
            n_iter, err, _ = dm.solve(1e-4, 50)
            assert (err <= 1e-4).all() and (n_iter < 50).all(), ("feeder does not converge", n_iter, err)
            dm.set_state(*seed)
        done = 0
        for state in states:
            want = 0 if state == "seed" else 3
            if want > done:
                dm.mismatch(want_f=False)
                dm.iterate(want - done)
            Vm, Va = dm.get_state()
            _, err = dm.mismatch()
            steps = sc.newton_steps(dm, c)
            done = want + 1
            out[state] = [(J, f, dx, Vm[s].copy(), Va[s].copy(), float(err[s])) for s, (J, f, dx) in enumerate(steps)]
        out["census"] = dm.tree_census() if dm.solver == "block_tree" else None
        out["solver"] = dm.solver
    finally:
        dm.close()
    return out


def _sparse_solve(J, f, n, c, Hn):
    """hpf_sparse_solve itself (no residual check, no dense fallback) -> (rc, dx)."""
    from harmonic_power_flow_amd import _lib
    lib = _lib.load()
    Jc = J.tocsr()
    indptr = np.ascontiguousarray(Jc.indptr, dtype=np.int32)
    indices = np.ascontiguousarray(Jc.indices, dtype=np.int32)
    data = np.ascontiguousarray(Jc.data, dtype=np.float64)
    fv = np.ascontiguousarray(f, dtype=np.float64)
    dx = np.full(fv.size, np.nan)
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    rc = lib.hpf_sparse_solve(0, int(n), int(c), int(Hn), indptr.ctypes.data_as(ip), indices.ctypes.data_as(ip), data.ctypes.data_as(dp),
                              fv.ctypes.data_as(dp), dx.ctypes.data_as(dp))
    return rc, dx


class StepGateExceeded(AssertionError):
    """A step that meets the eta gate (and every other check of its case) but misses STEP_MAX: raised last, so that a strict xfail of a
    recorded exceedance cannot be satisfied by any other failure."""


def _step_gate(lost):
    if lost:
        raise StepGateExceeded("; ".join(lost))


def _judge(tag, out, net, sparse=False):
    """eta and step error of every scenario at every state (and of hpf_sparse_solve on the same J, f); prints the worst; asserts the eta gate
    and the sparse solve's gates at once, and returns the fused steps that miss STEP_MAX (with eta and kappa_inf) for _step_gate."""
    Hn = len(net["st"].HARMONICS)
    worst = {"step": (0.0, 0.0), "sparse": (0.0, 0.0)}
    lost = []
    f_drop = []
    for state in ("seed", "iter3"):
        for J, f, dx, Vm, Va, err in out.get(state, []):
            import scipy.sparse.linalg as spl
            lu = spl.splu(J.tocsc())
            ref = sc.refined_solve(J, f, lu=lu)
            eta, se = sc.backward_error(J, dx, f), sc.step_error(dx, ref)
            worst["step"] = (max(worst["step"][0], eta), max(worst["step"][1], se))
            f_drop.append((state, float(np.abs(f).max())))
            assert eta <= ETA_MAX, (tag, state, eta, se)
            if se > STEP_MAX:
                lost.append("%s %s: step error %.2e at eta %.2e, kappa_inf %.2e" % (tag, state, se, eta, sc.cond_inf(J, lu)))
                print("\nSTEPCHECK " + lost[-1])
            if sparse:
                rc, dxs = _sparse_solve(J, f, net["n"], net["c"], Hn)
                if Hn == 1 and rc == -3:
                    continue                                # (one harmonic: bus 0 has no equation -> the topology the sparse route refuses)
                assert rc == 0, (tag, state, rc)
                eta_s, se_s = sc.backward_error(J, dxs, f), sc.step_error(dxs, ref)
                worst["sparse"] = (max(worst["sparse"][0], eta_s), max(worst["sparse"][1], se_s))
                assert eta_s <= ETA_MAX and se_s <= STEP_MAX, (tag, "hpf_sparse_solve", state, eta_s, se_s)
    fs = {k: max(v for s_, v in f_drop if s_ == k) for k in ("seed", "iter3") if any(s_ == k for s_, _ in f_drop)}
    print("\nSTEPCHECK %-44s step eta %.2e err %.2e | sparse eta %.2e err %.2e | |f| seed %.1e iter3 %.1e"
          % (tag, worst["step"][0], worst["step"][1], worst["sparse"][0], worst["sparse"][1], fs.get("seed", np.nan), fs.get("iter3", np.nan)))
    return lost


# ---- a. width sweep -------------------------------------------------------------------------------------------------------------------
def _vs_oracle(net, out, ne_dir=INPUTS):
    """f, err and J of the block-tree handle per scenario against the oracle (harmonic_mismatch, build_harmonic_jacobian) at 1e-12."""
    import hpf_oracle as o
    st = net["st"]
    onet = o.init_network(net["fb"], net["fl"])
    rowptr, col, Yval = o.build_admittance_matrices(onet, st.HARMONICS)
    NE = o.import_Norton_Equivalents(onet, st.HARMONICS, net["coupled"], ne_dir)
    sc_ = _scales(onet.n, S)
    P0, Q0 = onet.P.copy(), onet.Q.copy()
    for state in ("seed", "iter3"):
        for s, (J, f, dx, Vm, Va, err) in enumerate(out[state]):
            onet.P, onet.Q = P0 * sc_[s], Q0 * sc_[s]
            mdl = o.Model(onet, st.HARMONICS, rowptr, col, Yval, NE, net["coupled"])
            f_o, e_o = o.harmonic_mismatch(mdl, Vm.copy(), Va.copy())
            J_o = o.build_harmonic_jacobian(mdl, Vm.copy(), Va.copy())
            fsc = max(1.0, np.abs(f_o).max())
            assert np.abs(f - f_o).max() <= 1e-12 * fsc, (state, s, np.abs(f - f_o).max())
            assert abs(err - e_o) <= 1e-12 * fsc
            d = (J - J_o).tocoo()
            assert (np.abs(d.data).max() if d.nnz else 0.0) <= 1e-12 * np.abs(J_o.data).max(), (state, s)


# generator seeds of the widths whose seed-0 feeder does not converge in every scenario (the oracle's NR diverges there too)
WIDTH_SEED = {3: 4, 5: 1, 21: 1, 28: 1, 29: 1, 38: 1,
              # b > 100, the 64-harmonic table of tests/wide_ne.py (chosen with the oracle, three scenarios each): Hn = 51 .. 55 converge at seed 0
              # (20 - 38 iterations); Hn = 56 at seed 1 only (25 / 24 / 23 iterations; seeds 0 and 2 diverge).  Uncoupled, b = 102 and 112:
              # seed 0 converges (18 iterations), seeds 1 and 2 do not.  tests/test_wide_ne_host.py re-checks Hn = 56.
              56: 1}


# Fused steps that meet the eta gate but miss STEP_MAX (measured on the MI355X; every other check of these cases holds).  All sit on the
# 100-wide block path (b > 52: k_factor_q<100>, static pivot order, 4 x 4 pivot blocks) at states with kappa_inf 7e7 - 3e10, where the step's
# backward error, 2e-16 - 5e-14, is up to 1e4 times that of a partially pivoted LU.  On the same systems hpf_sparse_solve (1.9e-11 - 1.3e-10),
# the dense rocSOLVER path (b = 54: 3.2e-11) and the library's pivoted variant (HPF_GJ_MODE=0, 5.3e-12 - 1.9e-10,
# test_width_sweep_pivoted_variant) meet the gate, which places the loss in the static-pivot factorisation.  Open item, like case g below.
STEP_LOSS = {27: "b=54 after 3 iterations: step error 2.3e-9 at eta 2.4e-16, kappa_inf 2.1e10",
             28: "b=56 after 3 iterations: step error 3.2e-8 at eta 3.4e-15, kappa_inf 2.0e10",
             29: "b=58 after 3 iterations: step error 1.3e-9 at eta 9.5e-16, kappa_inf 1.5e10",
             35: "b=70 at the pf seed: step error 9.4e-9 at eta 4.8e-14, kappa_inf 7.7e7",
             40: "b=80 after 3 iterations: step error 1.1e-8 at eta 3.6e-15, kappa_inf 3.7e9 (pf seed: 5.1e-9 at eta 4.3e-14)",
             47: "b=94 after 3 iterations: step error 1.7e-9 at eta 3.9e-16, kappa_inf 3.1e10"}


def _width_params():
    return [pytest.param(Hn, marks=pytest.mark.xfail(strict=True, raises=StepGateExceeded,
                                                     reason="static-pivot step of the 100-wide block path: " + STEP_LOSS[Hn]))
            if Hn in STEP_LOSS else Hn for Hn in range(1, 51)]


@pytest.mark.parametrize("Hn", _width_params())
def test_width_sweep_coupled(Hn, tmp_path):
    """Coupled, H_MAX = 2 Hn - 1: every even block width b = 2 ... 100, so the first padded width above each class (14, 30, 54) and the
    ones no other test reaches (4, 8, 10, 18, 32, 34, 48, 50) run; fused step and hpf_sparse_solve against the yardstick, f / err / J against the oracle."""
    net = _net(tmp_path, N_BUS, 2 * Hn - 1, seed=WIDTH_SEED.get(Hn, SEED), coupled=True)
    out = _run(net)
    lost = _judge("a coupled b=%d" % (2 * Hn), out, net, sparse=True)
    _vs_oracle(net, out)
    _step_gate(lost)


@pytest.mark.parametrize("Hn", sorted(STEP_LOSS))
def test_width_sweep_pivoted_variant(Hn, tmp_path):
    """The systems of the recorded exceedances through the library's pivoted variant (HPF_GJ_MODE=0: partial pivoting over the whole bus
    block): the step gate holds there, which places the loss in the static-pivot factorisation of the default path."""
    net = _net(tmp_path, N_BUS, 2 * Hn - 1, seed=WIDTH_SEED.get(Hn, SEED), coupled=True)
    out = _run(net, options="HPF_GJ_MODE=0")
    _step_gate(_judge("a pivoted b=%d" % (2 * Hn), out, net))


@pytest.mark.parametrize("b", [2, 12, 14, 28, 30, 52, 54, 100])
def test_width_sweep_uncoupled(b, tmp_path):
    net = _net(tmp_path, N_BUS, b - 1, coupled=False)
    out = _run(net)
    lost = _judge("a uncoupled b=%d" % b, out, net, sparse=True)
    _vs_oracle(net, out)
    _step_gate(lost)


# ---- a'. blocks wider than 100 ----------------------------------------------------------------------------------------------------
# 100 < b <= 112 (wave_block_size 0): no contracted tree, no 2x2 algebra even in uncoupled models -- every bus is a dense bus of the generic
# 256-thread kernels (k_tree_factor<7>, more than 64 KB of dynamic LDS; k_tree_back), partial pivoting over the whole bus block.  The golden
# Norton table has 50 harmonics; tests/wide_ne.py derives one of 64 from it.
@pytest.fixture(scope="module")
def wide_dir(tmp_path_factory):
    import wide_ne
    return wide_ne.write(str(tmp_path_factory.mktemp("wide_ne")), INPUTS)


def _assert_generic_path(out, net):
    """the census of a handle whose steps ran on the generic kernels alone: a later change of dispatch cannot let a wide case pass elsewhere"""
    cs = out["census"]
    assert out["solver"] == "block_tree", out["solver"]
    assert cs["dense_buses"] == net["n"] and cs["gauss_jordan"] == net["n"], cs                  # every bus dense, none on the 2x2 path
    for k in ("const_leaves", "lazy_leaves", "bordered", "nested_bordered", "fused_levels", "compress_steps", "back_walks", "back_tails", "ties"):
        assert cs[k] == 0, (k, cs)


# Fused steps of a width above 100 that meet the eta gate but miss STEP_MAX, recorded like STEP_LOSS: none.  Measured on the MI355X (worst of
# three scenarios, pf seed and after 3 iterations), b = 102 / 104 / 106 / 108 / 110 / 112: eta 1.3e-15 / 3.3e-15 / 1.8e-15 / 1.9e-15 / 6.3e-16 /
# 1.1e-15, step error 5.4e-11 / 5.3e-11 / 1.4e-11 / 1.6e-11 / 1.7e-11 / 5.1e-11; uncoupled 102 and 112: 1.1e-17, 2.4e-15.  hpf_sparse_solve returns
# the same figures on the same systems: both run gj_dense_invert with partial pivoting over the whole bus block.
WIDE_STEP_LOSS = {}


def _wide_params():
    return [pytest.param(Hn, marks=pytest.mark.xfail(strict=True, raises=StepGateExceeded, reason="generic block path: " + WIDE_STEP_LOSS[Hn]))
            if Hn in WIDE_STEP_LOSS else Hn for Hn in range(51, 57)]


@pytest.mark.parametrize("Hn", _wide_params())
def test_width_sweep_coupled_wide(Hn, tmp_path, wide_dir):
    """Coupled, b = 102 ... 112: the whole window between the widest multi-wave block and the planner's limit, at the gates of the sweep above."""
    net = _net(tmp_path, N_BUS, 2 * Hn - 1, seed=WIDTH_SEED.get(Hn, SEED), coupled=True, ne_dir=wide_dir)
    out = _run(net)
    _assert_generic_path(out, net)
    lost = _judge("a coupled b=%d" % (2 * Hn), out, net, sparse=True)
    _vs_oracle(net, out, ne_dir=wide_dir)
    _step_gate(lost)


@pytest.mark.parametrize("b", [102, 112])
def test_width_sweep_uncoupled_wide(b, tmp_path, wide_dir):
    """Uncoupled above 100: use_lin is off, so the harmonic-diagonal buses run as dense blocks too."""
    net = _net(tmp_path, N_BUS, b - 1, coupled=False, ne_dir=wide_dir)
    out = _run(net)
    _assert_generic_path(out, net)
    lost = _judge("a uncoupled b=%d" % b, out, net, sparse=True)
    _vs_oracle(net, out, ne_dir=wide_dir)
    _step_gate(lost)


@pytest.fixture(scope="module")
def wide_seed_system(tmp_path_factory, wide_dir):
    """J and f of a 40-bus feeder at its pf seed from the oracle on the host, per Hn (no block-tree handle exists above b = 112)."""
    import hpf_oracle as o
    from harmonic_power_flow_amd import synth
    fb, fl = synth.gen(40, seed=0, outdir=str(tmp_path_factory.mktemp("wide40")))
    net = o.init_network(fb, fl)
    cache = {}

    def system(Hn):
        if Hn not in cache:
            H = o.harmonics_upto(2 * Hn - 1)
            rowptr, col, Yval = o.build_admittance_matrices(net, H)
            Vm, Va, _, _ = o.pf(net, rowptr, col, Yval)
            mdl = o.Model(net, H, rowptr, col, Yval, o.import_Norton_Equivalents(net, H, True, wide_dir), True)
            f, _ = o.harmonic_mismatch(mdl, Vm.copy(), Va.copy())
            cache[Hn] = (o.build_harmonic_jacobian(mdl, Vm.copy(), Va.copy()).tocsr(), f, net.n, net.c)
        return cache[Hn]
    return system


@pytest.mark.parametrize("Hn", [57, 60, 64])
def test_sparse_solve_beyond_the_block_tree(Hn, wide_seed_system):
    """hpf_sparse_solve at b = 114, 120, 128 (R = 8 register tiles, up to 135 KB of LDS per workgroup) at the gates of the fused step."""
    J, f, n, c = wide_seed_system(Hn)
    rc, dx = _sparse_solve(J, f, n, c, Hn)
    assert rc == 0, rc
    eta, se, _ = sc.judge(J, f, dx)
    print("\nSTEPCHECK %-44s sparse eta %.2e err %.2e | |f| seed %.1e" % ("a sparse b=%d n=%d" % (2 * Hn, n), eta, se, np.abs(f).max()))
    assert eta <= ETA_MAX and se <= STEP_MAX, (Hn, eta, se)


def test_sparse_solve_refuses_65_harmonics(wide_seed_system):
    """b = 130: HPF_E_ARG from the argument checks, before anything is launched -- dx stays as it was handed in."""
    J, f, n, c = wide_seed_system(57)
    N65 = 2 * (n * 65 - 1) - (c - 1)
    import scipy.sparse as sp
    rc, dx = _sparse_solve(sp.identity(N65, format="csr"), np.ones(N65), n, c, 65)
    assert rc == -1 and np.isnan(dx).all()


# ---- b. path matrix ---------------------------------------------------------------------------------------------------------------
PATH_WIDTHS = [12, 14, 28, 30, 52, 54, 100]
# n = 300, seed 2: at b <= 52 the default tree has lazy leaves, bordered and nested bordered buses, compress steps and fused levels (asserted
# below); fusion and lazy leaves exist only up to b = 52
PATH_N, PATH_SEED = 300, 2
VARIANTS = [("default", None, (), 3), ("HPF_LAZY=0", "HPF_LAZY=0", (), 3), ("HPF_LAZY=1", "HPF_LAZY=1", (), 3), ("HPF_SLEAF=0", "HPF_SLEAF=0", (), 3),
            ("HPF_LEAFBATCH=0", "HPF_LEAFBATCH=0", (), 3), ("HPF_SLBACK=0", "HPF_SLBACK=0", (), 3), ("HPF_SLLAZY=0", "HPF_SLLAZY=0", (), 3),
            ("HPF_SLNEST=0", "HPF_SLNEST=0", (), 3), ("HPF_FUSELEVEL=0", "HPF_FUSELEVEL=0", (), 3), ("HPF_LINBUNDLE=0", "HPF_LINBUNDLE=0", (), 3),
            ("HPF_LINTREE=0", "HPF_LINTREE=0", (), 3), ("HPF_CHAINBUNDLE=0", "HPF_CHAINBUNDLE=0", (), 3), ("HPF_COMPRESS=0", "HPF_COMPRESS=0", (), 3),
            ("HPF_FUSEBACK=0", "HPF_FUSEBACK=0", (), 3), ("HPF_GJ_MODE=0", "HPF_GJ_MODE=0", (), 3),
            ("block_pivoting=1", None, (("block_pivoting", 1),), 3), ("S=1", None, (), 1), ("S=17", None, (), 17), ("S=33", None, (), 33)]


@pytest.mark.parametrize("variant", [v[0] for v in VARIANTS])
@pytest.mark.parametrize("b", PATH_WIDTHS)
def test_path_matrix(b, variant, tmp_path):
    name, opts, set_opts, cap = next(v for v in VARIANTS if v[0] == variant)
    net = _net(tmp_path, PATH_N, b - 1, seed=PATH_SEED)
    out = _run(net, S_=min(S, cap), cap=cap, options=opts, set_opts=set_opts)
    cs = out["census"]
    lost = _judge("b b=%d %s" % (b, name), out, net)
    print("census", cs)
    if name == "default":
        if b <= 52:
            # (fused_levels: every level one k_level launch -- at 3 scenarios only with blocks of 52, b = 30 and 52)
            for k in ("lazy_leaves", "bordered", "nested_bordered", "compress_steps") + (("fused_levels",) if b > 28 else ()):
                assert cs[k] > 0, (b, k, cs)
        else:
            assert cs["lazy_leaves"] == 0 and cs["fused_levels"] == 0 and cs["compress_steps"] > 0, cs
        _step_gate(lost)
        return
    # each switch runs the path it names (and takes away what it switches off)
    if b <= 52:
        want = {"HPF_LAZY=0": lambda: cs["lazy_leaves"] == 0, "HPF_LAZY=1": lambda: cs["lazy_leaves"] > 0,
                "HPF_SLEAF=0": lambda: cs["bordered"] == 0, "HPF_SLLAZY=0": lambda: cs["nested_bordered"] == 0,
                "HPF_SLNEST=0": lambda: cs["nested_bordered"] == 0 and cs["bordered"] > 0, "HPF_FUSELEVEL=0": lambda: cs["fused_levels"] == 0,
                "HPF_COMPRESS=0": lambda: cs["compress_steps"] == 0, "HPF_GJ_MODE=0": lambda: cs["lazy_leaves"] == 0 and cs["fused_levels"] == 0,
                "block_pivoting=1": lambda: True}
        for k in ("HPF_LEAFBATCH=0", "HPF_SLBACK=0", "HPF_LINBUNDLE=0", "HPF_LINTREE=0", "HPF_CHAINBUNDLE=0", "HPF_FUSEBACK=0", "S=1", "S=17", "S=33"):
            want[k] = lambda: cs["lazy_leaves"] > 0 and cs["bordered"] > 0 and cs["compress_steps"] > 0
        assert want[name](), (b, name, cs)
    elif name == "HPF_COMPRESS=0":
        assert cs["compress_steps"] == 0, cs
    _step_gate(lost)


# ---- c. meshed feeders ------------------------------------------------------------------------------------------------------------
MESH_FORMS = [("factor-once", None, ()), ("HPF_BORDER_GJ_MFMA=0", "HPF_BORDER_GJ_MFMA=0", ()), ("border_pivoting=1", None, (("border_pivoting", 1),)),
              ("HPF_MESH_SEL=0", "HPF_MESH_SEL=0", ()), ("HPF_MESH_SEL=0 slots=16", "HPF_MESH_SEL=0 HPF_BORDER_SLOTS=16", ())]


@pytest.mark.parametrize("form", [f[0] for f in MESH_FORMS])
@pytest.mark.parametrize("b", [14, 30, 54, 100])
@pytest.mark.parametrize("k", [1, 3, 12])
def test_meshed(k, b, form, tmp_path):
    name, opts, set_opts = next(f for f in MESH_FORMS if f[0] == form)
    net = _net(tmp_path, N_BUS, b - 1, ties=k)
    out = _run(net, options=opts, set_opts=set_opts)
    cs = out["census"]
    assert out["solver"] == "block_tree" and cs["ties"] == k, cs
    assert cs["bordered_form"] == (0 if "MESH_SEL" in name else cs["bordered_form"]) and (cs["bordered_form"] > 0) == ("MESH_SEL" not in name), cs
    if name == "HPF_MESH_SEL=0 slots=16" and k == 12:
        # border_slots (hpf_block.hip): the m + 1 right-hand sides run in chunks of 16 once m + 1 >= 256 -- the chunked path ran
        assert cs["border_unknowns"] + 1 >= 256, cs
    _step_gate(_judge("c k=%d b=%d %s" % (k, b, name), out, net, sparse=(name == "factor-once")))


def test_meshed_uncoupled(tmp_path):
    net = _net(tmp_path, N_BUS, 29, coupled=False, ties=3)
    out = _run(net)
    assert out["census"]["ties"] == 3
    _step_gate(_judge("c uncoupled k=3 b=30", out, net, sparse=True))


# ---- d. the dense rocSOLVER path --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [2, 14, 54, 100])
def test_dense_path(b, tmp_path):
    net = _net(tmp_path, N_BUS, b - 1)
    out = _run(net, solver="dense")
    assert out["solver"] == "dense"
    _step_gate(_judge("d dense b=%d" % b, out, net))


# ---- f. positive control ----------------------------------------------------------------------------------------------------------
def test_positive_control_ablated_norton_coupling(tmp_path):
    """HPF_DEBUG_ABLATE=4 drops the whole assembled diagonal block of a bus -- the Norton terms with it -- in assemble_row.  That body runs in
    k_factor_w, i.e. on the pivoted variant (HPF_GJ_MODE=0; fused levels and the constant-inverse / lazy leaves never call it), so the control
    runs there.  The Gauss-Jordan then meets zero pivots and the step is NaN: this control shows only that the gate rejects a non-finite step
    (the finite wrong step is the next control's).  J comes from hpf_jacobian_csr, which the switch does not touch."""
    net = _net(tmp_path, N_BUS, 27)
    out = _run(net, options="HPF_DEBUG_ABLATE=4 HPF_GJ_MODE=0", converge=False, states=("seed",))
    J, f, dx = out["seed"][0][:3]
    eta = sc.backward_error(J, dx, f)
    print("\nSTEPCHECK f positive control (ABLATE=4) b=28 eta %.2e" % eta)
    assert not np.isfinite(eta)
    assert not eta <= ETA_MAX


def test_positive_control_skipped_child_updates(tmp_path):
    """HPF_DEBUG_ABLATE=2 skips the Schur complements a bus pulls from its dense children in k_factor_w (pivoted variant, every bus dense):
    the factorisation stays finite and the step is wrong.  It must miss the gate by 1000x."""
    net = _net(tmp_path, N_BUS, 27)
    out = _run(net, options="HPF_DEBUG_ABLATE=2 HPF_GJ_MODE=0", converge=False, states=("seed",))
    J, f, dx = out["seed"][0][:3]
    eta = sc.backward_error(J, dx, f)
    print("\nSTEPCHECK f positive control (ABLATE=2) b=28 eta %.2e (%.0fx ETA_MAX)" % (eta, eta / ETA_MAX))
    assert np.isfinite(dx).all()
    assert eta >= 1000 * ETA_MAX


# ---- g. the known blind spot ------------------------------------------------------------------------------------------------------
@pytest.mark.xfail(strict=True, raises=AssertionError, reason="open item: the fused step of a nested bordered core is not monitored -- fuzz case 38 loses ~2e-6 of the "
                                       "step there and hpf_solve does not flag it (flags bit 3)")
def test_unmonitored_nested_bordered_core_is_accurate_or_flagged(tmp_path):
    """Case 38 of the 400-case fuzz run (n = 286, H_MAX = 15, 85 % nonlinear, 2 PV buses, generator seed 441135, radial), built like
    tools/fuzz_parity.py builds it.  Contract: the first step meets the gate, or hpf_solve(max_iter=1) flags the scenario (flags bit 3)."""
    net = _net(tmp_path, 286, 15, seed=441135, frac_nl=0.85, n_pv=2)
    out = _run(net, S_=1, converge=False, states=("seed",))
    J, f, dx = out["seed"][0][:3]
    eta = sc.backward_error(J, dx, f)
    from harmonic_power_flow_amd import api
    dm = api._device_model(net["buses"], net["Y"], net["NE"], True, net["st"].HARMONICS, solver="block_tree")
    try:
        sc_ = _scales(net["n"], 1)
        dm.set_loads(net["buses"]["P"].to_numpy(float) * sc_, net["buses"]["Q"].to_numpy(float) * sc_)
        dm.set_state(None, None, n_scen=1)
        dm.fund_pf(1e-6, 30)
        dm.solve(1e-4, 1)
        flags = int(dm.stats()["flags"][0])
    finally:
        dm.close()
    print("\nSTEPCHECK g fuzz case 38 eta %.2e flags %d" % (eta, flags))
    assert eta <= ETA_MAX or (flags & 8)
