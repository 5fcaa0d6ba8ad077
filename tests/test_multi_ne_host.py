"""The four-type Norton tables and multi-type feeders of tests/multi_ne.py without a GPU: the files read back as specified, ingest numbers the
types as the GPU tests assume, the oracle converges on the small cases (and on the combinations the GPU tests add to the list of the helper's
header), the CSR pattern of the device walk equals the oracle's entry for entry with rows of two lengths at one harmonic, and the planner's
dump of the three-type 300-bus feeder still has every kind of bus test_gpu_step_accuracy.test_path_matrix asserts -- with parents and children
of different types."""
import os
import sys

import numpy as np
import pytest

import multi_ne
from conftest import INPUTS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.fixture(scope="module")
def ne_dir(tmp_path_factory):
    return multi_ne.write(str(tmp_path_factory.mktemp("multi_ne")), INPUTS)


def test_tables_read_back_as_specified(ne_dir):
    from harmonic_power_flow_amd import ingest
    K = multi_ne.K
    f0, Y0, I0, Yu0, Iu0 = ingest.read_Norton_file(os.path.join(INPUTS, "smps_NE.csv"))
    got = {name: ingest.read_Norton_file(os.path.join(ne_dir, name + "_NE.csv")) for name in multi_ne.TYPES4}
    assert sorted(os.listdir(ne_dir)) == sorted(name + "_NE.csv" for name in multi_ne.TYPES4)
    for name, (f1, Y1, I1, Yu1, Iu1) in got.items():
        assert f1 == f0 and Y1.shape == (K, K) and I1.shape == Yu1.shape == Iu1.shape == (K,), name
    # smps: the committed file, bit for bit
    for a, b in zip(got["smps"][1:], (Y0, I0, Yu0, Iu0)):
        assert np.array_equal(_bits(a), _bits(b))
    # led: one complex factor on every array (the product as numpy forms it, written and read back exactly)
    g = 0.6 * np.exp(0.3j)
    for a, b in zip(got["led"][1:], (Y0, I0, Yu0, Iu0)):
        assert np.array_equal(_bits(a), _bits(b * g))
    # vfd: row q times a(q).  The file holds the product as numpy's array multiply rounds it (round trip bit for bit); the formula evaluated
    # entry by entry in Python scalars agrees within the rounding of one complex product, 2^-50 relative
    q = np.arange(K)
    a_q = np.array([(0.5 + 0.4 * np.cos(0.9 * k) ** 2) * np.exp(0.3j * np.sin(0.5 * k)) for k in range(K)])
    _, Yv, Iv, Yuv, Iuv = got["vfd"]
    for i, j in ((0, 0), (0, 49), (49, 0), (7, 31), (31, 7), (49, 49)):
        assert abs(Yv[i, j] - complex(Y0[i, j]) * complex(a_q[i])) <= 2.0 ** -50 * abs(Yv[i, j])
    assert np.array_equal(Yv, Y0 * a_q[:, None]) and np.array_equal(Iv, I0 * a_q) and np.array_equal(Yuv, Yu0 * a_q) and np.array_equal(Iuv, Iu0 * a_q)
    assert 0.5 <= np.abs(a_q).min() and np.abs(a_q).max() <= 0.9 and a_q[0] == 0.9
    # ... which is no scalar multiple of smps, and differs from its own transposed scaling
    ratio = Yv / Y0
    assert np.abs(ratio - ratio[0, 0]).max() > 0.3 and np.abs(Yv - Y0 * a_q[None, :]).max() > 0.1 * np.abs(Yv).max()
    # band: smps inside |q - p| <= 3 bit for bit, exact zeros outside; the other three arrays unchanged
    _, Yb, Ib, Yub, Iub = got["band"]
    far = np.abs(q[:, None] - q[None, :]) > multi_ne.BAND
    assert far.sum() == K * K - (7 * K - 12) and (Y0[far] != 0).all()
    assert np.array_equal(_bits(Yb[~far]), _bits(Y0[~far]))
    assert (_bits(Yb[far]) == 0).all()                                  # +0.0 + 0.0j, not merely == 0
    for a, b in ((Ib, I0), (Yub, Yu0), (Iub, Iu0)):
        assert np.array_equal(_bits(a), _bits(b))
    # the oracle's own reader selects the same numbers
    import hpf_oracle as o
    h = o.harmonics_upto(99)
    for name in multi_ne.TYPES4:
        I_o, Y_o = o.import_norton(os.path.join(ne_dir, name + "_NE.csv"), h, True)
        assert np.array_equal(Y_o, got[name][1] / o.base_admittance) and np.array_equal(I_o, got[name][2] / o.base_current), name


@pytest.mark.parametrize("arrangement", multi_ne.ARRANGEMENTS)
@pytest.mark.parametrize("types", [multi_ne.TYPES3, multi_ne.TYPES4], ids=["three", "four"])
def test_norton_arrays_number_the_types_in_the_helper_s_order(types, arrangement, ne_dir, tmp_path):
    import harmonic_power_flow_amd as hp
    from harmonic_power_flow_amd import ingest
    (fb, fl), ti = multi_ne.feeder(tmp_path, 24, 0, types, arrangement)
    st = hp.Settings(H_MAX=11)
    buses, lines, m, n, c = hp.init_network(fb, fl, settings=st)
    T, n_nl = len(types), n - m
    assert n_nl == 8 and len(ti) == n_nl
    want = [j % T for j in range(n_nl)] if arrangement == "interleaved" else [(T * j) // n_nl for j in range(n_nl)]
    assert ti.tolist() == want and list(buses["component"][m:]) == [types[t] for t in want]
    assert types[want[0]] == "vfd" and set(want) == set(range(T))       # the first nonlinear bus is not smps; every type occurs
    for coupled in (True, False):
        NE = hp.import_Norton_Equivalents(buses, coupled, st, ne_dir)
        dev, Y_N, I_N, n_dev = ingest.norton_arrays(buses, NE, coupled, len(st.HARMONICS))
        assert n_dev == T and list(NE) == list(types)
        assert dev[:m].tolist() == [-1] * m and dev[m:].tolist() == want
        # every table is its own type's: the rows of Y_N / I_N against the files
        Hn = len(st.HARMONICS)
        for d, name in enumerate(types):
            _, Ycc, Ic, Yuc, Iuc = ingest.read_Norton_file(os.path.join(ne_dir, name + "_NE.csv"))
            if coupled:
                assert np.array_equal(Y_N[d], Ycc[:Hn, :Hn] / st.base_admittance) and np.array_equal(I_N[d], Ic[:Hn] / st.base_current)
            else:
                assert np.array_equal(Y_N[d], Yuc[:Hn] / st.base_admittance) and np.array_equal(I_N[d], Iuc[:Hn] / st.base_current)
        assert len({Y_N[d].tobytes() for d in range(T)}) == (T if coupled or "band" not in types else T - 1)   # (band's uncoupled table is smps's)


# (buses, generator seed, types, H_MAX, coupled, ties): the small cases of the helper's header, and the combinations the GPU tests add to it --
# each must converge in the oracle before a step test may use it (iterations measured here: see the helper's header and test_gpu_device_types.py)
BOTH = multi_ne.ARRANGEMENTS
ORACLE_CASES = [(24, 0, "four", 11, True, 0, BOTH), (24, 0, "four", 51, True, 0, BOTH), (90, 0, "three", 11, True, 0, BOTH),
                (24, 0, "four", 99, True, 0, BOTH), (24, 0, "four", 11, False, 0, BOTH), (24, 0, "four", 51, False, 0, BOTH),
                (24, 0, "four", 99, False, 0, BOTH), (90, 0, "three", 13, True, 0, BOTH[:1]), (90, 0, "three", 29, True, 3, BOTH[:1])]


@pytest.mark.parametrize("n,seed,types,hmax,coupled,ties,arrangement", [c[:6] + (a,) for c in ORACLE_CASES for a in c[6]])
def test_the_oracle_converges(n, seed, types, hmax, coupled, ties, arrangement, ne_dir, tmp_path):
    import hpf_oracle as o
    from harmonic_power_flow_amd import synth
    tt = multi_ne.TYPES3 if types == "three" else multi_ne.TYPES4
    (fb, fl), _ = multi_ne.feeder(tmp_path, n, seed, tt, arrangement, ties=ties)
    h = o.harmonics_upto(hmax)
    net = o.init_network(fb, fl)
    rowptr, col, Yval = o.build_admittance_matrices(net, h)
    NE = o.import_Norton_Equivalents(net, h, coupled, ne_dir)
    assert list(NE) == list(tt)
    P0, Q0 = net.P.copy(), net.Q.copy()
    its = []
    for s in range(3):
        sc_ = synth.scenario_scale(net.n, s)
        net.P, net.Q = P0 * sc_, Q0 * sc_
        Vm, Va, _, _ = o.pf(net, rowptr, col, Yval)
        r = o.hpf_from_model(o.Model(net, h, rowptr, col, Yval, NE, coupled), Vm, Va)
        assert r["err_h"] <= 1e-4 and r["n_iter_h"] < 50, (s, r["n_iter_h"], r["err_h"])
        its.append(r["n_iter_h"])
    print("\nMULTI_NE oracle gen(%d, %d) %s %s H_MAX %d %s ties %d: iterations %s" % (n, seed, types, arrangement, hmax, "c" if coupled else "uc", ties, its))


@pytest.mark.parametrize("arrangement", multi_ne.ARRANGEMENTS)
@pytest.mark.parametrize("hmax", [11, 51])
def test_csr_pattern_equals_the_oracle_s_and_band_rows_are_shorter(hmax, arrangement, tmp_path):
    """jcsr_count / jcsr_fill on the host (Emul.jacobian_csr): the stored entries are the oracle's, entry for entry, and a row of a band bus is
    shorter than the row of an smps bus at the same harmonic -- the case has rows of more than one length and cannot lose that unnoticed."""
    import hpf_oracle as o
    case = multi_ne.host_case(tmp_path, INPUTS, arrangement=arrangement, hmax=hmax)
    em, mdl, n, m, c, Hn = case["em"], case["mdl"], case["n"], case["m"], case["c"], len(case["st"].HARMONICS)
    Vm, Va = multi_ne.oracle_states(case, iters=(0, 1))[1]
    J = em.jacobian_csr(Vm, Va)
    Jo = o.build_harmonic_jacobian(mdl, Vm.copy(), Va.copy()).tocsr()
    Jo.sort_indices()
    assert (Jo.data != 0).all()                                         # (no stored zero on the oracle's side hides a pattern difference)
    assert J.nnz == Jo.nnz and np.array_equal(J.indptr, Jo.indptr) and np.array_equal(J.indices, Jo.indices)
    assert np.abs(J.data - Jo.data).max() <= 1e-13 * np.abs(Jo.data).max()
    # row lengths per (bus, harmonic): the real row of the current balance of bus i at harmonic q is row (m - 1) + q n + i - m of J (HG:469-472)
    length = np.diff(J.indptr)
    types = multi_ne.TYPES4
    by_type = {t: [m + j for j, ti in enumerate(case["ti"]) if types[ti] == t] for t in types}
    deg = np.diff(case["Y"].rowptr)
    cross = {"band": lambda q: min(Hn - 1, q + multi_ne.BAND) - max(0, q - multi_ne.BAND), "smps": lambda q: Hn - 1}
    shorter = 0
    for q in range(Hn):
        for t in ("band", "smps"):
            for i in by_type[t]:
                row = (m - 1) + q * n + (i - m)
                # theta and V columns of every admittance entry of the bus (the slack's fundamental has neither; c = 1: no PV bus)
                own = 2 * int(deg[i]) - (2 if q == 0 and 0 in case["Y"].col[case["Y"].rowptr[i]:case["Y"].rowptr[i + 1]] else 0)
                assert length[row] == own + 2 * cross[t](q), (t, i, q, length[row])         # (cross terms: the bus's own columns, never the slack's)
        nb, ns = cross["band"](q), cross["smps"](q)
        if nb < ns:
            shorter += 1
    assert shorter == (Hn if Hn > 2 * multi_ne.BAND + 1 else 2 * (Hn - 1 - multi_ne.BAND)) > 0
    assert len(set(length[(m - 1):(m - 1) + Hn * n])) > 2


def _plan(arrangement, outdir):
    import tree_plan
    ne = multi_ne.write(outdir, INPUTS, multi_ne.TYPES3)
    (fb, fl), ti = multi_ne.feeder(outdir, 300, 2, multi_ne.TYPES3, arrangement)
    rows = tree_plan.plan(300, 51, files=(fb, fl), ne_dir=ne)
    m = 300 - len(ti)
    dev = {m + j: int(t) for j, t in enumerate(ti)}
    return rows, dev


@pytest.mark.parametrize("arrangement", multi_ne.ARRANGEMENTS)
def test_plan_of_the_three_type_feeder_keeps_every_kind_of_bus_and_mixes_types(arrangement, tmp_path, monkeypatch):
    """hpf_tree_plan's dump of gen(300, 2) at H_MAX 51 (columns as tests/test_shapes_plan_host.py reads them: bus, dense parent, level, depth,
    kind, vector_only, hbm_children, via_chain, compress_role).  The per-bus images -- a bordered bus's low-rank inverse from its own Y_N and the
    images of its lazy leaves, a Gauss-Jordan bus's constant-inverse leaves -- meet parents and children of different types."""
    for k in [k for k in os.environ if k.startswith("HPF_") and k != "HPF_ENV_SWITCHES"]:
        monkeypatch.delenv(k)
    rows, dev = _plan(arrangement, str(tmp_path))
    kids = {}
    for r in rows:
        kids.setdefault(r[1], []).append(r)
    lazy = [r for r in rows if r[5] != 0]
    bordered = [r for r in rows if r[4] == 2]
    nested = [r for r in bordered if any(c[4] == 2 and c[5] != 0 for c in kids.get(r[0], []))]
    compress = [r for r in rows if r[8] != 0]
    print("\nMULTI_NE plan %s: dense %d, lazy %d, bordered %d, nested bordered %d, compress roles %d" % (arrangement, len(rows), len(lazy), len(bordered),
                                                                                                         len(nested), len(compress)))
    assert lazy and bordered and nested and compress
    # the plan does not depend on the types' values (bordered buses and leaves are chosen by topology): the smps-only plan, row for row
    import tree_plan
    assert rows == tree_plan.plan(300, 51, seed=2)
    if arrangement == "interleaved":
        other = [(r[0], dev[r[0]], [dev.get(c[0]) for c in kids.get(r[0], []) if c[5] != 0]) for r in bordered if r[0] in dev]
        other = [x for x in other if any(t is not None and t != x[1] for t in x[2])]
        assert other, "no nonlinear bordered bus with a lazy child of another type"
        two = [(r[0], sorted({dev[c[0]] for c in kids.get(r[0], []) if c[4] == 1 and c[0] in dev})) for r in rows if r[4] == 0]
        two = [x for x in two if len(x[1]) >= 2]
        assert two, "no Gauss-Jordan bus with constant-inverse leaves of two types"
        print("MULTI_NE plan: bordered (bus, type, lazy children's types) %s; Gauss-Jordan (bus, leaf types) %s" % (other[:3], two[:3]))
