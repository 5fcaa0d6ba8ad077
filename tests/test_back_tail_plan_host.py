"""Host logic of the back-sweep tail (k_back_tail) without a GPU: the planner's dump lists the batch records of the back sweep (d_bsleaf: bordered
buses, d_bleaf: constant-inverse leaves) and the families it groups them into -- a batched bus whose dense parent is not batched, its nested
bordered buses and the leaves below any of them.  Checked here for feeders of blocks of 12, 28 and 52 rows: every record is in exactly one
family, once; a member's parent comes earlier in its family or is no batched bus; an LDS parent slot holds that parent's x when the member
reads it; families come longest first; each feeder has a family of three generations, and none with HPF_SLNEST=0."""
import os
import re
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

TAIL_SLOTS = 2          # hpf_internal.hpp

FEEDERS = [(600, 11, 0), (400, 27, 0), (300, 51, 2)]      # buses, H_MAX, seed


def _tail(n, hmax, seed, monkeypatch, slnest=None):
    """the contracted tree's block of the dump: its bus rows, the bus ids of d_bsleaf and d_bleaf, the families as lists of (bus, parent's slot, own slot)"""
    import tree_plan
    if slnest is None:
        monkeypatch.delenv("HPF_SLNEST", raising=False)
    else:
        monkeypatch.setenv("HPF_SLNEST", slnest)
    lines = tree_plan.plan(n, hmax, seed=seed, lines_out=True)
    heads = [i for i, ln in enumerate(lines) if re.match(r"# (contracted|plain) tree:", ln)]
    assert lines[heads[0]].startswith("# contracted tree:"), lines[:2]
    block = lines[heads[0]:heads[1] if len(heads) > 1 else len(lines)]
    rows = [tuple(map(int, ln.split())) for ln in block if not ln.startswith("#")]
    info = {r[0]: dict(par=r[1], kind=r[4]) for r in rows}
    head = [ln for ln in block if ln.startswith("# tail:")]
    assert len(head) == 1, block[:3]
    nf, slots = map(int, re.match(r"# tail: (\d+) families, (\d+) slots", head[0]).groups())
    assert slots == TAIL_SLOTS
    bsleaf = [list(map(int, ln.split()[2:])) for ln in block if ln.startswith("# tail_bsleaf")]
    bleaf = [list(map(int, ln.split()[2:])) for ln in block if ln.startswith("# tail_bleaf")]
    assert len(bsleaf) == 1 and len(bleaf) == 1
    fams = [[tuple(map(int, m.split(":"))) for m in ln.split()[3:]] for ln in block if ln.startswith("# tail_family ")]
    assert len(fams) == nf
    return info, bsleaf[0], bleaf[0], fams


def _generations(info, fam):
    """does the family hold a bordered bus, a bordered bus nested in it and a leaf of the nested one"""
    members = {k for k, _, _ in fam}
    for k, _, _ in fam:
        p = info[k]["par"]
        if info[k]["kind"] == 1 and p in members and info[p]["kind"] == 2 and info[p]["par"] in members and info[info[p]["par"]]["kind"] == 2:
            return True
    return False


@pytest.mark.parametrize("n,hmax,seed", FEEDERS)
def test_families_cover_every_batch_record_once_in_dependency_order(n, hmax, seed, monkeypatch):
    info, bsleaf, bleaf, fams = _tail(n, hmax, seed, monkeypatch)
    batched = bsleaf + bleaf
    assert len(bsleaf) > 0 and len(bleaf) > 0 and len(set(batched)) == len(batched)
    assert all(info[k]["kind"] == 2 for k in bsleaf) and all(info[k]["kind"] == 1 for k in bleaf)
    members = [k for fam in fams for k, _, _ in fam]
    assert sorted(members) == sorted(batched), "a record in no family, or in more than one place"
    assert [len(f) for f in fams] == sorted((len(f) for f in fams), reverse=True), "families are not longest first"
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
    assert any(_generations(info, fam) for fam in fams), "no family of three generations: bordered, nested bordered, leaf"
    # two slots are enough on these feeders: no member reads a parent of its own family back from HBM
    assert all(pslot != -2 for fam in fams for _, pslot, _ in fam)


@pytest.mark.parametrize("n,hmax,seed", FEEDERS)
def test_no_nested_member_without_nested_bordered_buses(n, hmax, seed, monkeypatch):
    info, bsleaf, bleaf, fams = _tail(n, hmax, seed, monkeypatch, slnest="0")
    bs = set(bsleaf)
    assert bs and all(info[k]["par"] not in bs for k in bsleaf)
    for fam in fams:
        assert sum(1 for k, _, _ in fam if k in bs) <= 1
        assert not _generations(info, fam)


def test_backtail_switch_parses(tmp_path):
    """HPF_BACKTAIL (default on) in csrc/hpf_switches.hpp, parsed like the other switches"""
    import subprocess
    src = tmp_path / "bt.cpp"
    src.write_text('#include <stdio.h>\n#include "hpf_switches.hpp"\nint main() {\n'
                   '    const hpf::Switches d = hpf::parse_switches(nullptr, false), a = hpf::parse_switches("HPF_BACKWALK=1,HPF_BACKTAIL=0", false),\n'
                   '                        b = hpf::parse_switches("HPF_BACKTAIL=1 HPF_LAZY=0", false);\n'
                   '    printf("%d %d %d %d\\n", (int)d.back_tail, (int)a.back_tail, (int)b.back_tail, (int)a.back_walk);\n    return 0;\n}\n')
    exe = str(tmp_path / "bt.bin")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(REPO, "harmonic-power-flow_amd", "csrc"), str(src), "-o", exe])
    env = {k: v for k, v in os.environ.items() if not k.startswith("HPF_")}
    assert subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env).stdout.split() == ["1", "0", "1", "1"]
