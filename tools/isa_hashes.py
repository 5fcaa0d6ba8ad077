#!/usr/bin/env python3
"""sha256 of the gfx950 assembly text of every device function of the library's translation units, by symbol name: the check that a host-side
change left the device code alone.  Compiles the device side only, with build.py's flags (cross-compiles without a GPU).
python tools/isa_hashes.py [repository root] > hashes.txt       # two trees have the same device code when the two files are equal
A function's text is everything from its label to its .size line plus its .amdhsa_kernel block.  The numbers the compiler gives a function's
local labels (.LBB<i>_<j>, .Lfunc_end<i>) count the functions of the file before it, so <i> is blanked: the comparison is by name, not by
position in the file."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPO = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else HERE
CSRC = os.path.join(REPO, "harmonic-power-flow_amd", "csrc")
sys.path.insert(0, os.path.join(HERE, "harmonic-power-flow_amd"))
import build                                                # noqa: E402  (this tree's list of translation units and flags, for either root)
SOURCES = build.SOURCES
FLAGS = build.FLAGS + os.environ.get("HPF_CFLAGS", "").split()


def functions(asm):
    """-> {symbol: text} of every symbol typed @function"""
    lines = asm.split("\n")
    names = [m.group(1) for m in (re.match(r"\s*\.type\s+(\S+),@function", ln) for ln in lines) if m]
    out = {}
    for name in names:
        beg = next(i for i, ln in enumerate(lines) if ln.startswith(name + ":"))
        end = next(i for i in range(beg, len(lines)) if re.match(r"\s*\.size\s+%s," % re.escape(name), lines[i]))
        text = lines[beg:end + 1]
        head = "\t.amdhsa_kernel " + name
        if head in lines:
            k = lines.index(head)
            text += lines[k:lines.index("\t.end_amdhsa_kernel", k) + 1]
        out[name] = re.sub(r"\.L(BB|func_end|func_begin)\d+", r".L\1", "\n".join(text))
    return out


with tempfile.TemporaryDirectory() as tmp:
    for src in SOURCES:
        s_file = os.path.join(tmp, src + ".s")
        subprocess.check_call([os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")] + FLAGS +
                              ["--cuda-device-only", "-S", os.path.join(CSRC, src), "-o", s_file], stderr=subprocess.DEVNULL)
        fn = functions(open(s_file).read())
        for name in sorted(fn):
            print("%s %s %s" % (src, name, hashlib.sha256(fn[name].encode()).hexdigest()))
