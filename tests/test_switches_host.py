"""The build-switch parser (csrc/hpf_switches.hpp: parse_switches, the one list of libhpf's HPF_* switches) compiled on its own with g++ under
ASan + UBSan; tests/cpu_emul/switches_main.cpp is the driver."""
import os
import subprocess

from conftest import REPO

SRC = os.path.join(REPO, "tests", "cpu_emul", "switches_main.cpp")
CSRC = os.path.join(REPO, "harmonic-power-flow_amd", "csrc")


def test_switch_parser(tmp_path):
    exe = str(tmp_path / "switches.bin")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", CSRC, SRC, "-o", exe])
    env = {k: v for k, v in os.environ.items() if not k.startswith("HPF_")}     # (the driver sets the environment it needs)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "switches clean" in r.stdout
