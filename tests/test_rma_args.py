"""hpf_resonance_modes: the host checks through libhpf.so.  Every HPF_E_ARG / HPF_E_TOPOLOGY case of include/hpf.h is decided on the host before
any HIP call: the calls below return their code on a machine without a GPU, where a call that passes the checks ends at the first HIP call with
another code."""
import ctypes as C

import numpy as np

import zscan_emul as ze


def _call(model, h, y_extra=None, iters=8, chunk=0, nulls=(), F=None):
    from harmonic_power_flow_amd import _lib
    lib = _lib.load()
    ip, dp = _lib.c_int_p, _lib.c_dbl_p
    n = int(model["n"])
    a = {k: np.ascontiguousarray(model[k], dtype=np.int32 if k in ("fr", "to") else np.float64) for k in ("fr", "to", "R", "X", "gsh", "bsh", "xsh")}
    ptr = {k: (None if k in nulls else v.ctypes.data_as(ip if k in ("fr", "to") else dp)) for k, v in a.items()}
    net = _lib.hpf_zscan_net(n, int(model["nb"]), ptr["fr"], ptr["to"], ptr["R"], ptr["X"], ptr["gsh"], ptr["bsh"], ptr["xsh"])
    h = np.ascontiguousarray(h, dtype=np.float64)
    F = len(h) if F is None else F
    yx = None if y_extra is None else np.ascontiguousarray(y_extra, dtype=np.complex128)
    zm = np.empty(max(len(h), 1))
    return lib.hpf_resonance_modes(0, None if "net" in nulls else C.byref(net), F, None if "h" in nulls else h.ctypes.data_as(dp),
                                   None if yx is None else yx.ctypes.data_as(dp), iters, chunk, None, zm.ctypes.data_as(dp), None, None, None)


def test_resonance_modes_checks_its_arguments_on_the_host():
    ring = ze.raw_model(4, [(0, 1), (1, 2), (2, 3), (0, 3)])
    h = np.array([0.5, 2.0, 3.0])
    assert _call(ring, h) not in (-1, -3)                      # a valid call passes the analysis (no GPU here: the first HIP call ends it)
    assert _call(ring, h, iters=1, chunk=2) not in (-1, -3)
    assert _call(ring, h, iters=256) not in (-1, -3)
    # the iteration count
    assert _call(ring, h, iters=0) == -1
    assert _call(ring, h, iters=257) == -1
    assert _call(ring, h, iters=-1) == -1
    # what hpf_impedance_scan rejects for net, F, h, y_extra and chunk
    assert _call(ring, h, nulls=("net",)) == -1
    assert _call(ring, h, nulls=("h",)) == -1
    for key in ("fr", "to", "R", "X", "gsh", "bsh", "xsh"):
        assert _call(ring, h, nulls=(key,)) == -1
    assert _call(dict(ring, n=0), h) == -1
    assert _call(dict(ring, n=2 ** 22 + 1), h) == -1
    assert _call(dict(ring, nb=-1), h) == -1
    assert _call(ring, h, F=0) == -1
    assert _call(ring, h, F=2 ** 20 + 1) == -1

    def with_(**kw):
        m = {k: np.array(v, copy=True) if isinstance(v, np.ndarray) else v for k, v in ring.items()}
        for k, (pos, val) in kw.items():
            m[k][pos] = val
        return m
    assert _call(with_(fr=(1, 3)), h) == -1                    # from == to
    assert _call(with_(fr=(2, 3), to=(2, 2)), h) == -1         # from > to
    assert _call(with_(to=(3, 4)), h) == -1                    # end bus outside 0 .. n-1
    assert _call(with_(fr=(0, -1)), h) == -1
    assert _call(with_(fr=(3, 0), to=(3, 1)), h) == -1         # duplicate pair (0, 1)
    assert _call(with_(R=(1, 0.0), X=(1, 0.0)), h) == -1       # R = X = 0
    for key in ("R", "X", "gsh", "bsh", "xsh"):
        for bad in (np.nan, np.inf):
            assert _call(with_(**{key: (0, bad)}), h) == -1
    for bad in (np.nan, np.inf, 0.0, -1.0):
        assert _call(ring, np.array([0.5, bad, 3.0])) == -1    # non-finite h, h <= 0
    yx = np.zeros((3, 4), dtype=np.complex128)
    yx[1, 2] = complex(0.0, np.nan)
    assert _call(ring, h, y_extra=yx) == -1
    yx[1, 2] = complex(np.inf, 0.0)
    assert _call(ring, h, y_extra=yx) == -1
    assert _call(ring, h, chunk=-1) == -1
    # a forced chunk whose launches over n buses would not fit a one-dimensional grid: n ceil(chunk / 256) > 2^30
    big = ze.chain(2 ** 19)
    assert _call(big, np.linspace(0.5, 50.5, 2 ** 20), chunk=2 ** 20) == -1

def test_resonance_modes_classifies_the_topology_on_the_host():
    h = np.array([0.5, 2.0])
    assert _call(ze.raw_model(4, [(0, 1), (2, 3)]), h) == -3                              # not connected from bus 0
    assert _call(ze.raw_model(2, []), h) == -3
    ring10 = [(i, i + 1) for i in range(9)] + [(0, 9)]
    chords = [(0, 2), (1, 3), (2, 4), (3, 5), (4, 6), (5, 7), (6, 8), (7, 9)]
    assert _call(ze.raw_model(10, ring10 + chords[:7]), h) not in (-1, -3)                # 8 ties
    assert _call(ze.raw_model(10, ring10 + chords), h) == -3                              # 9 ties
