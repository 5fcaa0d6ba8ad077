"""The shared part of the sweep accumulators (csrc/hpf_accum.hpp: list entry, counters walk, owner walk, statistic slot) compiled on its own
with g++ under ASan + UBSan over exactly sized buffers; tests/cpu_emul/accum_main.cpp is the driver."""
import os
import subprocess

from conftest import REPO

SRC = os.path.join(REPO, "tests", "cpu_emul", "accum_main.cpp")
CSRC = os.path.join(REPO, "harmonic-power-flow_amd", "csrc")


def test_list_walks_and_slot_layout(tmp_path):
    exe = str(tmp_path / "accum.bin")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", CSRC, SRC, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "accum clean" in r.stdout
