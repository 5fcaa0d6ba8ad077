#!/usr/bin/env python3
"""Device-memory leak check of meshed handles: 90 create / solve / destroy cycles in the three forms of the bordered step.   python tools/mesh_leak_check.py   (GPU)"""
import os, sys, tempfile
sys.path.insert(0, os.getcwd())
import numpy as np
import harmonic_power_flow_amd as hp
from harmonic_power_flow_amd import api, synth
from harmonic_power_flow_amd.device import device_memory        # the library's own count of live blocks / bytes: other processes on the device do not show
INP = "tests/golden/inputs"
fb, fl = synth.gen(300, seed=2, outdir=tempfile.mkdtemp()); synth.add_ties(fl, 300, 5)
st = hp.Settings(H_MAX=27); buses, lines, m, n, c = hp.init_network(fb, fl, settings=st)
Y = hp.build_admittance_matrices(buses, lines, st.HARMONICS); NE = hp.import_Norton_Equivalents(buses, True, st, INP)
def once(opt=None):
    dm = api._device_model(buses, Y, NE, True, st.HARMONICS, solver="block_tree", max_scenarios=4, options=opt)
    dm.set_loads(np.tile(buses["P"].to_numpy(float), (4, 1)), np.tile(buses["Q"].to_numpy(float), (4, 1))); dm.set_state(None, None, n_scen=4); dm.fund_pf(1e-6, 30); dm.solve(1e-4, 5); dm.close()
once(); once("HPF_BORDER_GJ=0"); once("HPF_MESH_SEL=0")
f0 = device_memory()
for i in range(30):
    once(); once("HPF_BORDER_GJ=0"); once("HPF_MESH_SEL=0")
f1 = device_memory()
print("live device blocks / bytes before and after 90 create-solve-destroy cycles of meshed handles: %d / %d -> %d / %d" % (f0 + f1))
sys.exit(0 if f0 == f1 == (0, 0) else 1)
