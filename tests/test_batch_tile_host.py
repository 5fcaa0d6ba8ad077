"""The role mapping of the scenario-batched factor bodies (csrc/hpf_batch_tile.hpp: which thread serves which row and harmonic of a tile of 16
or 8 scenarios) compiled on its own with g++ under ASan + UBSan; tests/cpu_emul/batch_tile_main.cpp is the driver.  And the switch that
pick the tile (HPF_BATCH_TILE8_MAX, HPF_LEAF_TILE8_MAX, csrc/hpf_switches.hpp) parse like their neighbours."""
import os
import subprocess

from conftest import REPO

SRC = os.path.join(REPO, "tests", "cpu_emul", "batch_tile_main.cpp")
CSRC = os.path.join(REPO, "harmonic-power-flow_amd", "csrc")


def _run(tmp_path, name, src):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", CSRC, src, "-o", exe])
    env = {k: v for k, v in os.environ.items() if not k.startswith("HPF_")}
    return subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)


def test_every_row_and_harmonic_has_one_owner(tmp_path):
    r = _run(tmp_path, "batch_tile.bin", SRC)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "batch tile clean" in r.stdout


def test_tile_switch_parses(tmp_path):
    src = tmp_path / "tile_switch.cpp"
    src.write_text('#include <stdio.h>\n#include "hpf_switches.hpp"\n#include "hpf_batch_tile.hpp"\nusing namespace hpf;\n'
                   'int main() {\n'
                   '    const int d = parse_switches(nullptr, false).batch_tile8_max;\n'
                   '    const Switches s = parse_switches("HPF_FUSEBACK_MAX=8 HPF_BATCH_TILE8_MAX=64,HPF_LEAF_TILE8_MAX=16", false);\n'
                   '    printf("%d %d %d %d %d %d %d\\n", d, s.batch_tile8_max, s.fuse_back_max, batch_tile_of(64, s.batch_tile8_max),\n'
                   '           batch_tile_of(65, s.batch_tile8_max), parse_switches(nullptr, false).leaf_tile8_max, s.leaf_tile8_max);\n'
                   '    return 0;\n}\n')
    r = _run(tmp_path, "tile_switch.bin", str(src))
    assert r.returncode == 0, r.stdout + r.stderr
    d, t8, fb, a, b, dl, l8 = (int(x) for x in r.stdout.split())
    assert d >= 0 and dl >= 0 and (t8, fb, a, b, l8) == (64, 8, 8, 16, 16)
