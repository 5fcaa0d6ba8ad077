"""The scratch-size formulas behind the automatic chunk lengths of hpf_impedance_scan and hpf_penetration (zscan_per_f of csrc/hpf_zscan.hpp,
pen_per_f and pen_per_j of csrc/hpf_penetration.hpp; exported by the emulation libraries) against the expressions they replaced, written out here,
and the chunk lengths that follow from them.  The bit-for-bit tests cannot see a chunk length -- no result depends on it -- so this pins them."""
import ctypes as C
import itertools

import pen_emul as pe
import zscan_emul as ze

NS, KS, SELS, FS, SS = (1, 2, 33, 1000), (0, 1, 4), (0, 3), (1, 65, 4096), (1, 70)


def _zscan_per_f(n, k, n_sel, has_x, want_Z):
    ncol = n_sel + 2 * k
    stage_rows = max(n if (want_Z or has_x) else 0, n_sel * n)
    return 3 * n + (n if has_x else 0) + ncol * n + k * k + stage_rows


def _pen_per_f(n, k, has_x):
    return 2 * n + (n if k else 0) + (2 * n if has_x else 0) + 2 * k * n + k * k


def _pen_per_j(n, k, n_inj, want_V):
    return n + max(n_inj, n if want_V else 0) + k


def _zscan_lib():
    lib = ze.load()
    lib.emul_zscan_per_f.restype = C.c_longlong
    return lib


def _pen_lib():
    lib = pe.load()
    lib.emul_pen_per_f.restype = lib.emul_pen_per_j.restype = C.c_longlong
    return lib


def test_the_scan_formula_and_its_chunk_lengths():
    lib = _zscan_lib()
    for n, k, n_sel, has_x, want_Z in itertools.product(NS, KS, SELS, (0, 1), (0, 1)):
        want = _zscan_per_f(n, k, n_sel, has_x, want_Z)
        assert lib.emul_zscan_per_f(n, k, n_sel, has_x, want_Z) == want, (n, k, n_sel, has_x, want_Z)
        for F in FS:
            got = lib.emul_zscan_chunk(F, 0, C.c_longlong(lib.emul_zscan_per_f(n, k, n_sel, has_x, want_Z)))
            assert got == lib.emul_zscan_chunk(F, 0, C.c_longlong(want)) and 1 <= got <= F, (n, k, n_sel, has_x, want_Z, F)


def test_the_penetration_formulas_and_their_chunk_lengths():
    lib = _pen_lib()
    for n, k, has_x, want_V in itertools.product(NS, KS, (0, 1), (0, 1)):
        for n_inj in sorted({1, (n + 1) // 2, n}):
            per_f, per_j = _pen_per_f(n, k, has_x), _pen_per_j(n, k, n_inj, want_V)
            assert lib.emul_pen_per_f(n, k, has_x) == per_f, (n, k, has_x)
            assert lib.emul_pen_per_j(n, k, n_inj, want_V) == per_j, (n, k, n_inj, want_V)
            for F, S in itertools.product(FS, SS):
                got = pe.chunks(F, S, 0, 0, lib.emul_pen_per_f(n, k, has_x), lib.emul_pen_per_j(n, k, n_inj, want_V))
                assert got == pe.chunks(F, S, 0, 0, per_f, per_j) and 1 <= got[0] <= F and 1 <= got[1] <= S, (n, k, has_x, n_inj, want_V, F, S)


def test_the_parent_formula_clips_a_large_scan_below_the_grid():
    """so that the table above does compare automatic lengths shorter than F, not F with F"""
    lib = _zscan_lib()
    assert lib.emul_zscan_chunk(4096, 0, C.c_longlong(_zscan_per_f(1000, 4, 3, 1, 1))) < 4096
    assert pe.chunks(4096, 70, 0, 0, _pen_per_f(1000, 4, 1), _pen_per_j(1000, 4, 1000, 1))[0] < 4096
