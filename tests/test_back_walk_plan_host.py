"""Host logic of the back-sweep tree walk (k_back_walk) without a GPU: the planner's dump lists the walk's trunk (list 0) and branch
lists.  Checked here, for the golden networks, synthetic feeders of 50 - 1 000 buses, meshed ones and both HPF_COMPRESS settings: every
Gauss-Jordan bus of the back sweep is walked exactly once; a bus comes after its dense parent and, in compress role 1, after its pending
child c -- earlier in its own list, or in the trunk; constant-inverse leaves and bordered buses (back_batched, after the walk) enter no list."""
import os
import re
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
INPUTS = os.path.join(REPO, "tests", "golden", "inputs")

WALK_LISTS = 8          # hpf_internal.hpp


def _walk(net, hmax, ties, compress, monkeypatch):
    """the contracted tree's block of the dump (from its header line to the plain tree's): its bus rows, trunk depths, lists, compress pairs"""
    import tree_plan
    if compress is None:
        monkeypatch.delenv("HPF_COMPRESS", raising=False)
    else:
        monkeypatch.setenv("HPF_COMPRESS", compress)
    if isinstance(net, str):
        lines = tree_plan.plan(0, hmax, lines_out=True,
                               files=(os.path.join(INPUTS, net + "_buses.csv"), os.path.join(INPUTS, net + "_lines.csv")))
    else:
        lines = tree_plan.plan(net, hmax, ties=ties, lines_out=True)
    heads = [i for i, ln in enumerate(lines) if re.match(r"# (contracted|plain) tree:", ln)]
    assert lines[heads[0]].startswith("# contracted tree:"), lines[:2]
    block = lines[heads[0]:heads[1] if len(heads) > 1 else len(lines)]
    rows = [tuple(map(int, ln.split())) for ln in block if not ln.startswith("#")]
    info = {r[0]: dict(par=r[1], depth=r[3], kind=r[4], role=r[8]) for r in rows}
    assert len(info) == len(rows)
    head = [ln for ln in block if ln.startswith("# walk:")]
    assert len(head) == 1, block[:3]
    depth, nl = map(int, re.match(r"# walk: (\d+) trunk depths, (\d+) branch lists", head[0]).groups())
    lists = [list(map(int, ln.split()[3:])) for ln in block if ln.startswith("# walk_list ")]
    comp = dict(tuple(map(int, ln.split()[2:4])) for ln in block if ln.startswith("# walk_comp "))
    return info, depth, nl, lists, comp


GOLDEN = [("net1", 51, 0), ("net2", 51, 0), ("net3", 51, 0), ("lin4", 51, 0), ("fuchs4", 51, 0), ("quirk5", 51, 0)]
SYNTH = [(50, 51, 0), (100, 51, 0), (200, 51, 0), (300, 51, 0), (400, 51, 0), (500, 51, 0), (700, 51, 0), (1000, 51, 0),
         (120, 51, 1), (300, 51, 4), (260, 51, 12), (1000, 51, 5)]


@pytest.mark.parametrize("compress", [None, "0"])
@pytest.mark.parametrize("net,hmax,ties", GOLDEN + SYNTH)
def test_walk_covers_every_gauss_jordan_bus_once_in_dependency_order(net, hmax, ties, compress, monkeypatch):
    info, depth, nl, lists, comp = _walk(net, hmax, ties, compress, monkeypatch)
    assert len(lists) == nl + 1 and 0 <= nl <= WALK_LISTS and depth >= 1
    walked = [k for li in lists for k in li]
    assert len(walked) == len(set(walked)), "a bus walked twice"
    gj = {k for k, v in info.items() if v["kind"] == 0}
    assert set(walked) == gj, (sorted(gj - set(walked))[:5], sorted(set(walked) - gj)[:5])
    trunk = set(lists[0])
    assert all(info[k]["depth"] < depth for k in trunk) and all(info[k]["depth"] >= depth for li in lists[1:] for k in li)
    if compress == "0" or not isinstance(net, int) or net < 300:
        assert compress != "0" or not comp
    else:
        assert comp                                  # (feeders of this size have compress steps)
    for li in lists:
        pos = {k: i for i, k in enumerate(li)}
        for k in li:
            for dep in (info[k]["par"], comp.get(k, -1)):
                if dep < 0:
                    continue
                assert (li is not lists[0] and dep in trunk) or (dep in pos and pos[dep] < pos[k]), (k, dep)
    for v, c in comp.items():
        assert info[v]["role"] == 1 and info[c]["role"] == 2


def test_walk_shape_of_the_headline_feeder(monkeypatch):
    """syn1000, K = 25 (blocks of 52): three trunk depths, eight branch lists that share the 73 buses below the trunk"""
    info, depth, nl, lists, comp = _walk(1000, 51, 0, None, monkeypatch)
    assert (depth, nl) == (3, WALK_LISTS)
    assert len(lists[0]) == 10 and sum(map(len, lists[1:])) == 73 and max(map(len, lists[1:])) <= 12


def test_backwalk_switches_parse(tmp_path):
    """HPF_BACKWALK (default on), HPF_BACKWALK_MIN (default 16) and HPF_BACKWALK_MAX (default 256) in csrc/hpf_switches.hpp, parsed like the other switches"""
    import subprocess
    src = tmp_path / "bw.cpp"
    src.write_text('#include <stdio.h>\n#include "hpf_switches.hpp"\nint main() {\n'
                   '    const hpf::Switches d = hpf::parse_switches(nullptr, false), a = hpf::parse_switches("HPF_BACKWALK=0,HPF_BACKWALK_MIN=2,HPF_BACKWALK_MAX=7", false);\n'
                   '    printf("%d %d %d %d %d %d\\n", (int)d.back_walk, d.back_walk_min, d.back_walk_max, (int)a.back_walk, a.back_walk_min, a.back_walk_max);\n    return 0;\n}\n')
    exe = str(tmp_path / "bw.bin")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(REPO, "harmonic-power-flow_amd", "csrc"), str(src), "-o", exe])
    env = {k: v for k, v in os.environ.items() if not k.startswith("HPF_")}
    assert subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env).stdout.split() == ["1", "16", "256", "0", "2", "7"]
