"""The split of a batch over the scenario groups (csrc/hpf_groups.hpp: group count and tile-aligned bounds, the one copy every enqueue uses)
compiled on its own with g++ under ASan + UBSan; tests/cpu_emul/groups_main.cpp is the driver."""
import os
import subprocess

from conftest import REPO

SRC = os.path.join(REPO, "tests", "cpu_emul", "groups_main.cpp")
CSRC = os.path.join(REPO, "harmonic-power-flow_amd", "csrc")


def test_scenario_group_split(tmp_path):
    exe = str(tmp_path / "groups.bin")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", CSRC, SRC, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "groups clean" in r.stdout
