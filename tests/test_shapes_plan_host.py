"""The block-tree plan of the feeders of tests/shapes.py without a GPU: deep paths, caterpillars, brooms, stars, a full binary tree and feeders of
one bus class -- the shapes at which the planner's capacities bind (WALK_SLOTS, WALK_LISTS, LZ_MAX, the lin_np thresholds, TAIL_SLOTS), none of
which synth.gen's random trees reach.  For every case, with and without compress steps: the dependency invariants of
test_tree_plan_host.py, the walk invariants of test_back_walk_plan_host.py and the family invariants of test_back_tail_plan_host.py (their
parsers, imported), the facts of shapes.CASES, and the facts that make a case what it is for: a walk list longer than the LDS ring, lazy and
constant-inverse leaves mixed under one hub, no 2x2 algebra on an all-nonlinear feeder, no dense bus on an all-linear one.  The oracle solves
every case inside the iteration limits of the GPU tests."""
import os
import re
import sys

import numpy as np
import pytest

import shapes
import test_back_tail_plan_host as tail_host
import test_back_walk_plan_host as walk_host
import test_tree_plan_host as plan_host
from conftest import INPUTS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

LZ_MAX = 4              # hpf_tree_plan.hpp (plan_leaf_images)
ALL = shapes.CASES + shapes.EXTRA
IDS = [c.id for c in ALL]


def _constant(name):
    """a constexpr int of hpf_internal.hpp (of WALK_SLOTS the default: -DHPF_WALK_SLOTS in HPF_CFLAGS overrides it, see _ring)"""
    src = open(os.path.join(REPO, "harmonic-power-flow_amd", "csrc", "hpf_internal.hpp")).read()
    m = re.search(r"#define HPF_%s (\d+)" % name, src) or re.search(r"\b%s = (\d+)" % name, src)
    return int(m.group(1))


def _ring(f):
    """the ring size the library was built with, from the dump's `# caps:` line; the header's default unless a build flag overrides it"""
    if "HPF_WALK_SLOTS" not in os.environ.get("HPF_CFLAGS", ""):
        assert f["walk_slots"] == _constant("WALK_SLOTS")
    return f["walk_slots"]


def _far(block, ring):
    """same-list dependencies (parent, compress child) of the walk that lie at least `ring` records back: (bus, dependency, distance)"""
    rows = [tuple(map(int, ln.split())) for ln in block if not ln.startswith("#")]
    par = {r[0]: r[1] for r in rows}
    comp = dict(tuple(map(int, ln.split()[2:4])) for ln in block if ln.startswith("# walk_comp "))
    out = []
    for ln in block:
        if ln.startswith("# walk_list "):
            li = list(map(int, ln.split()[3:]))
            pos = {k: i for i, k in enumerate(li)}
            out += [(k, d, pos[k] - pos[d]) for k in li for d in (par[k], comp.get(k, -1)) if d in pos and pos[k] - pos[d] >= ring]
    return out


@pytest.fixture
def files(tmp_path, monkeypatch):
    """Writes a case's CSV pair and points tools/tree_plan.plan -- what the three imported parsers call -- at it.  The parsers were written
    for synth.gen feeders and pass a bus count, a seed or a golden net's name; the patched plan() ignores all of these (and `ties`: the shapes
    are radial) and plans the shape's files instead, so whatever the callers below hand the parsers as `net` / `n` / `seed` is a placeholder."""
    import tree_plan
    real = tree_plan.plan

    def use(case):
        fb, fl = shapes.write(case.name, case.n, str(tmp_path))
        monkeypatch.setattr(tree_plan, "plan", lambda nb, hmax, seed=0, max_scenarios=1, ties=0, lines_out=False, files=None:
                            real(0, hmax, max_scenarios=max_scenarios, lines_out=lines_out, files=(fb, fl)))
        return fb, fl
    return use


def _dump(case, monkeypatch, compress):
    """the contracted tree's block of the dump, as lines"""
    import tree_plan
    if compress is None:
        monkeypatch.delenv("HPF_COMPRESS", raising=False)
    else:
        monkeypatch.setenv("HPF_COMPRESS", compress)
    lines = tree_plan.plan(case.n, case.hmax, lines_out=True)
    heads = [i for i, ln in enumerate(lines) if re.match(r"# (contracted|plain) tree:", ln)]
    assert lines[heads[0]].startswith("# contracted tree:")
    return lines[heads[0]:heads[1] if len(heads) > 1 else len(lines)]


def _facts(block):
    """the `# caps:`, `# lin:` and `# chains:` lines of the dump -> dict"""
    out = {}
    for tag in ("caps", "lin"):
        ln = [x for x in block if x.startswith("# %s:" % tag)]
        assert len(ln) == 1, (tag, block[:6])
        w = ln[0].split()[2:]
        out.update({k: int(v) for k, v in zip(w[::2], w[1::2])})
    ln = [x for x in block if x.startswith("# chains:")]
    assert len(ln) == 1
    out["chains"], out["max_chain"], out["chain_launches"], out["chains_bundled"] = map(
        int, re.match(r"# chains: (\d+) chains, longest (\d+), own launches (\d+), bundled (\d+)", ln[0]).groups())
    return out


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_dependencies_with_and_without_compress_steps(case, files, monkeypatch):
    """the invariants of test_compress_plan_dependencies, on the shape's own trees"""
    files(case)
    flat = plan_host._plan(case.n, case.hmax, monkeypatch, "0")
    comp = plan_host._plan(case.n, case.hmax, monkeypatch, None)
    assert set(flat) == set(comp) and len(comp) == case.dense
    assert all(v["role"] == 0 for v in flat.values())
    for k, v in flat.items():                       # leaf-first order: a bus one level above its tallest dense child, one depth below its parent
        kids = [c for c, w in flat.items() if w["par"] == k]
        assert v["level"] == (max(flat[c]["level"] for c in kids) + 1 if kids else 0) or (not kids and v["kind"] == 0)
        assert v["depth"] == (flat[v["par"]]["depth"] + 1 if v["par"] >= 0 else 0)
    lv_f = max((v["level"] for v in flat.values()), default=-1) + 1
    lv_c = max((v["level"] for v in comp.values()), default=-1) + 1
    vs = [k for k, v in comp.items() if v["role"] == 1]
    cs = [k for k, v in comp.items() if v["role"] == 2]
    assert len(vs) == len(cs) and len(vs) + len(cs) == case.roles
    assert lv_c == case.levels and (lv_c < lv_f if cs else lv_c == lv_f)
    for c in cs:                                    # a pending child: Gauss-Jordan bus, re-linked to its grandparent, never compressed itself
        v = flat[c]["par"]
        assert comp[v]["role"] == 1 and comp[c]["par"] == flat[v]["par"] == comp[v]["par"]
        assert comp[c]["kind"] == 0 and comp[v]["kind"] == 0 and comp[comp[v]["par"]]["kind"] == 0
        assert comp[v]["level"] < comp[c]["level"] < comp[comp[c]["par"]]["level"]          # v -> c -> p in the factor sweep
        assert comp[comp[c]["par"]]["depth"] < comp[c]["depth"] < comp[v]["depth"]          # p -> c -> v in the back sweep
    for k, v in comp.items():                       # everybody else: after its dense children, below its parent
        for c, w in comp.items():
            if w["par"] == k:
                assert w["level"] < v["level"] and w["depth"] > v["depth"]
    assert all(flat[k]["kind"] == comp[k]["kind"] and flat[k]["vector_only"] == comp[k]["vector_only"] for k in flat)
    # the deep shapes are what the compress steps are for: they halve the chain of levels
    if case.name in ("allnl_path", "path", "caterpillar"):
        assert cs and lv_c <= lv_f // 2 + 3, (lv_f, lv_c)


@pytest.mark.parametrize("compress", [None, "0"])
@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_walk_covers_every_gauss_jordan_bus_once_in_dependency_order(case, compress, files, monkeypatch):
    """the invariants of the test of that name in test_back_walk_plan_host.py; at most WALK_LISTS branch lists everywhere"""
    files(case)
    if case.walk is None:                           # no dense bus: no walk at all
        block = _dump(case, monkeypatch, compress)
        assert not [ln for ln in block if not ln.startswith("#")] and not [ln for ln in block if ln.startswith("# walk")]
        return
    info, depth, nl, lists, comp = walk_host._walk(case.n, case.hmax, 0, compress, monkeypatch)
    assert walk_host.WALK_LISTS == _constant("WALK_LISTS")
    assert len(lists) == nl + 1 and 0 <= nl <= walk_host.WALK_LISTS and depth >= 1
    walked = [k for li in lists for k in li]
    assert len(walked) == len(set(walked)), "a bus walked twice"
    gj = {k for k, v in info.items() if v["kind"] == 0}
    assert set(walked) == gj, (sorted(gj - set(walked))[:5], sorted(set(walked) - gj)[:5])
    trunk = set(lists[0])
    assert all(info[k]["depth"] < depth for k in trunk) and all(info[k]["depth"] >= depth for li in lists[1:] for k in li)
    assert bool(comp) == (compress is None and case.roles > 0)
    for li in lists:
        pos = {k: i for i, k in enumerate(li)}
        for k in li:
            for dep in (info[k]["par"], comp.get(k, -1)):
                if dep < 0:
                    continue
                assert (li is not lists[0] and dep in trunk) or (dep in pos and pos[dep] < pos[k]), (k, dep)
    for v, c in comp.items():
        assert info[v]["role"] == 1 and info[c]["role"] == 2
    if compress is None:
        assert [len(li) for li in lists] == case.walk


@pytest.mark.parametrize("compress", [None, "0"])
@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_families_cover_every_batch_record_once_in_dependency_order(case, compress, files, monkeypatch):
    """the invariants of the test of that name in test_back_tail_plan_host.py (minus what only its own feeders promise: three generations)"""
    files(case)
    if case.leaves + case.bordered == 0:
        block = _dump(case, monkeypatch, compress)
        assert not [ln for ln in block if ln.startswith("# tail")]
        return
    if compress is None:
        monkeypatch.delenv("HPF_COMPRESS", raising=False)
    else:
        monkeypatch.setenv("HPF_COMPRESS", compress)
    info, bsleaf, bleaf, fams = tail_host._tail(case.n, case.hmax, 0, monkeypatch)
    TAIL_SLOTS = tail_host.TAIL_SLOTS
    assert TAIL_SLOTS == _constant("TAIL_SLOTS")
    batched = bsleaf + bleaf
    assert len(set(batched)) == len(batched) and (len(bsleaf), len(bleaf)) == (case.bordered, case.leaves)
    assert all(info[k]["kind"] == 2 for k in bsleaf) and all(info[k]["kind"] == 1 for k in bleaf)
    members = [k for fam in fams for k, _, _ in fam]
    assert sorted(members) == sorted(batched), "a record in no family, or in more than one place"
    assert [len(f) for f in fams] == sorted((len(f) for f in fams), reverse=True), "families are not longest first"
    assert len(fams) == case.families
    bset = set(batched)
    for fam in fams:
        pos = {k: i for i, (k, _, _) in enumerate(fam)}
        owner = {}                                       # LDS slot -> the bus whose x it holds
        assert info[fam[0][0]]["par"] not in bset        # the root hangs under a bus of the walk / the depth launches
        for i, (k, pslot, oslot) in enumerate(fam):
            par = info[k]["par"]
            if par in bset:
                assert i > 0 and par in pos and pos[par] < i, (k, par)
                assert info[par]["kind"] == 2
                assert pslot == -2 or (0 <= pslot < TAIL_SLOTS and owner.get(pslot) == par), (k, par, pslot, owner)
            else:
                assert i == 0 and pslot == -1, (k, par, pslot)
            assert -1 <= oslot < TAIL_SLOTS
            if oslot >= 0:
                assert info[k]["kind"] == 2              # (only a bordered bus has batched children)
                owner[oslot] = k
        if len(fam) == 1:
            assert fam[0][2] == -1
    # no shape exhausts the two LDS slots of a family: no member reads a parent of its own family back from HBM (families are chains
    # of nested bordered buses with their leaves, at most five members)
    assert all(pslot != -2 for fam in fams for _, pslot, _ in fam) and max(len(f) for f in fams) <= 5
    # hundreds of families of one leaf each (stars), against a handful of deep ones
    if case.name in ("star", "star_allnl", "star_nlhub", "broom"):
        assert all(len(f) == 1 for f in fams) and len(fams) >= 30


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_plan_facts(case, files, monkeypatch):
    """shapes.CASES, asserted against the planner's dump (default plan), and what each shape is in the suite for"""
    files(case)
    block = _dump(case, monkeypatch, None)
    rows = [tuple(map(int, ln.split())) for ln in block if not ln.startswith("#")]
    f = _facts(block)
    kinds = [sum(r[4] == k for r in rows) for k in range(3)]
    assert len(rows) == case.dense and kinds == [case.gj, case.leaves, case.bordered]
    assert max((r[2] for r in rows), default=-1) + 1 == case.levels
    assert sum(r[5] != 0 for r in rows) == case.lazy and sum(r[8] != 0 for r in rows) == case.roles
    for k in ("chains", "max_chain", "chain_launches", "max_unit"):
        assert f[k] == getattr(case, k), (k, f)
    assert (f["form"], f["lin_np"], f["roots"]) == (case.lin_form, case.lin_np, case.lin_roots), f
    ring = _ring(f)
    assert (f["walk_lists"], f["tail_slots"]) == (_constant("WALK_LISTS"), _constant("TAIL_SLOTS"))
    Hn = (case.hmax + 1) // 2
    walk = [len(ln.split()) - 3 for ln in block if ln.startswith("# walk_list ")]
    if case.name in ("allnl_path", "caterpillar"):
        # the LDS ring of k_back_walk wraps: a list longer than WALK_SLOTS, and (allnl_path) a second wrap.  Every dependency is at most
        # 3 records back, so at the default ring the wrap only overwrites slots nobody reads any more; a ring of 2 or 3 slots
        # (-DHPF_WALK_SLOTS) turns these lists into re-reads from HBM
        assert max(walk) > ring
        assert case.name != "allnl_path" or max(walk) > 2 * ring
        assert bool(_far(block, ring)) == (ring <= 3)
    if case.name == "comb_allnl":
        # the re-read from HBM after a wrap, at the default ring: parents 33 records back, compress children 66
        far = _far(block, ring)
        assert max(walk) > ring and len(far) >= 33 and max(d for _, _, d in far) >= 2 * ring, far[:4]
        comp = dict(tuple(map(int, ln.split()[2:4])) for ln in block if ln.startswith("# walk_comp "))
        assert any(comp.get(k) == d for k, d, _ in far) and any(comp.get(k) != d for k, d, _ in far)
    if case.name == "binary_allnl":
        assert len(walk) - 1 == f["walk_lists"]
    if case.name == "no_nl":
        assert not rows and f["roots"] == 1 and f["max_unit"] == case.n
    if case.name in shapes.ALL_NL:
        # no 2x2 algebra at all: no linear root, no contracted chain
        assert f["roots"] == 0 and f["chains"] == 0 and f["heights"] == 0 and len(rows) == case.n
    if case.name in ("star_nlhub", "star_allnl"):
        # LZ_MAX lazy leaves under the hub, every other leaf constant-inverse with a Schur complement of its own, under the same Gauss-Jordan bus
        hub = case.n - 1
        kids = [r for r in rows if r[1] == hub]
        assert {r[0]: r for r in rows}[hub][4] == 0 and all(r[4] == 1 for r in kids) and len(kids) == case.leaves
        assert sum(r[5] != 0 for r in kids) == LZ_MAX and sum(r[5] == 0 for r in kids) == case.leaves - LZ_MAX > 0
    if case.name == "broom":
        hub = case.n // 2 - 1
        kids = [r for r in rows if r[1] == hub]
        assert len(kids) == case.leaves and sum(r[5] != 0 for r in kids) == LZ_MAX and all(r[7] == 0 for r in kids)
    if case.name in ("path", "one_nl_deep", "broom"):
        # a chain the one-round-trip bundles would not hold (Hn items per chain bus): it runs in the chain launches
        assert f["chains"] == 1 and f["chain_launches"] == 1 and f["chains_bundled"] == 0
        assert case.hmax < 51 or f["max_chain"] * Hn > 1024
    if case.name == "linstar_under_nl":
        # one unit of 101 buses, 100 of them at one height: above every lin_np class at 26 harmonics (tree bundles, 9 buses per height
        # and pass of the workgroup), in the largest class at 6
        assert f["max_unit"] * Hn > 1024 if case.hmax == 51 else 512 < f["max_unit"] * Hn <= 1024
        assert (f["form"], f["lin_np"]) == ((shapes.LIN_TREE, 0) if case.hmax == 51 else (shapes.LIN_BUNDLE, 4))
        assert f["max_unit"] - 1 > 256 // Hn
    if case.name == "star":
        assert f["roots"] == case.n - 1 - case.leaves and f["heights"] == 1 and f["form"] == shapes.LIN_LEVELS


LIN_CASES = [("path", 51), ("one_nl_deep", 51), ("linstar_under_nl", 51), ("linstar_under_nl", 11)]


@pytest.mark.parametrize("switch", ["HPF_LINBUNDLE=0", "HPF_LINTREE=0", "HPF_CHAINBUNDLE=0"])
@pytest.mark.parametrize("name,hmax", LIN_CASES)
def test_which_switch_changes_the_form_of_the_2x2_algebra(name, hmax, switch, files, monkeypatch):
    """shapes.LIN_SWITCHED: the three combinations in which a switch of test_gpu_shapes.py's form test moves the plan to another form; the
    others leave the default plan as it is"""
    case = shapes.case(name, hmax=hmax)
    files(case)
    base = _facts(_dump(case, monkeypatch, None))
    monkeypatch.setenv(*switch.split("="))
    f = _facts(_dump(case, monkeypatch, None))
    want = shapes.LIN_SWITCHED.get((name, hmax, switch))
    if want is None:
        assert f == base
    else:
        assert (f["form"], f["lin_np"]) == want != (base["form"], base["lin_np"])


def test_a_converged_step_cannot_be_judged_as_a_state_difference(tmp_path):
    """Why test_gpu_shapes.py judges the star at one harmonic at the pf seed only.  stepcheck.newton_steps measures a step as the difference
    of two states.  The oracle's iteration on this feeder has converged after 3 iterations (steps below 1e-9 on states of magnitude 1), and the
    refined reference solution ITSELF, rounded through x1 = x0 - dx, dx' = x0 - x1, misses the eta gate there by orders of magnitude."""
    import hpf_oracle as o
    import stepcheck as sc
    import harmonic_power_flow_amd as hp
    from harmonic_power_flow_amd import synth
    for n in (90, 300):
        fb, fl = shapes.write("star", n, str(tmp_path))
        net = o.init_network(fb, fl)
        s0 = synth.scenario_scale(net.n, 0)
        net.P, net.Q = net.P * s0, net.Q * s0
        r = o.hpf(net, hp.Settings(H_MAX=1).HARMONICS, True, INPUTS, thresh_h=0.0, max_iter_h=3)
        Vm, Va = r["Vm_raw"].copy(), r["Va_raw"].copy()
        f, err = o.harmonic_mismatch(r["model"], Vm, Va)
        J = o.build_harmonic_jacobian(r["model"], Vm, Va)
        ref = sc.refined_solve(J, f)
        x0 = o.harmonic_state_vector(r["model"], Vm, Va)
        through_state = x0 - (x0 - ref)
        eta_ref, eta_state = sc.backward_error(J, ref, f), sc.backward_error(J, through_state, f)
        print("\nSHAPES star-%d-H1 after 3 iterations: err %.1e |dx| %.1e eta of the reference %.1e, through the state difference %.1e"
              % (n, err, np.abs(ref).max(), eta_ref, eta_state))
        assert err <= 1e-4 and np.abs(ref).max() < 1e-9
        assert eta_ref <= sc.ETA_MAX < 1e4 * sc.ETA_MAX < eta_state


def test_shapes_files_are_in_the_generator_dialect(tmp_path):
    """bus order slack | PQ | nonlinear, one line per bus but the slack, a tree; write() is deterministic and leaves synth.gen's draws alone"""
    import harmonic_power_flow_amd as hp
    from harmonic_power_flow_amd import synth
    for case in ALL:
        fb, fl = shapes.write(case.name, case.n, str(tmp_path))
        st = hp.Settings(H_MAX=case.hmax)
        buses, lines, m, n, c = hp.init_network(fb, fl, settings=st)
        assert n == case.n and len(lines) == n - 1
        par, n_nl = shapes._tree(case.name, case.n)
        assert m == n - n_nl
        for k in par:                               # every bus reaches the slack
            seen = 0
            while k != 1:
                k = par[k]
                seen += 1
                assert seen < n
        a = open(fb).read(), open(fl).read()
        (tmp_path / "again").mkdir(exist_ok=True)
        fb2, fl2 = shapes.write(case.name, case.n, str(tmp_path / "again"))
        assert a == (open(fb2).read(), open(fl2).read())
    first = open(synth.gen(50, outdir=str(tmp_path))[0]).read()
    shapes.write("star", 90, str(tmp_path))
    gb = synth.gen(50, outdir=str(tmp_path))
    assert open(gb[0]).read() == first


@pytest.mark.parametrize("case", shapes.CASES, ids=[c.id for c in shapes.CASES])
def test_the_oracle_solves_every_case(case, tmp_path):
    """the reference's algorithm converges on every case inside the iteration limits the GPU tests use"""
    import hpf_oracle as o
    import harmonic_power_flow_amd as hp
    fb, fl = shapes.write(case.name, case.n, str(tmp_path))
    st = hp.Settings(H_MAX=case.hmax)
    r = o.hpf(o.init_network(fb, fl), st.HARMONICS, True, INPUTS)
    print("\nSHAPES oracle %-24s n_iter_f %d n_iter_h %d err_h %.2e" % (case.id, r["n_iter_f"], r["n_iter_h"], r["err_h"]))
    assert r["err_h"] <= 1e-4 and r["n_iter_h"] < 50 and r["n_iter_f"] < 30
