// Harmonic penetration (hpf_penetration): the bus voltages V(h) = Y(h)^-1 I(h) that S scenarios of injected harmonic currents produce over a grid of
// F real harmonic orders -- the linear "current injection" study.  The network, y_e(h), D_i, the BFS tree, w_i, t_i, the tie columns u_l and W^-1
// are exactly those of hpf_zscan.hpp (the factor: computed once per frequency point, shared by all scenarios); this header adds the right-hand-side
// path.  The k_pen_* kernels of hpf_zscan.hip run these functions on the device, one thread per (bus, j); the host emulation
// (tests/cpu_emul/pen_emul.cpp) runs the same functions serially.  Every product, sum and quotient is rounded on its own (-ffp-contract=off;
// cmul_unf, cadd, csub of hpf_assembly.hpp, crecip and zscan_abs of hpf_zscan.hpp), every sum has the one order written here, nothing is atomic:
// device == emulation bit for bit, for every chunking.
//
// A chunk is fc frequency points x sc scenarios; j = f sc + s (the scenario fastest inside a frequency point), J = fc sc.  The right-hand sides live
// in place as r [n][J]; the factor stays [bus][fc], read at f = j / sc.  b = the injected currents (zero at the buses not listed).
//   up    (deepest depth first):  r_i = ((b_i + t_c1 r_c1) + t_c2 r_c2) + ...      c1 < c2 < ...: the children of i; the parent gathers
//   down  (root first):           V_0 = w_0 r_0,   V_i = cadd(cmul_unf(w_i, r_i), cmul_unf(t_i, V_p(i)))                   (V overwrites r)
//   ties  (k > 0):                d_m = V[a_m] - V[b_m]
//                                 c_l = sum_m Winv_lm d_m            over ascending m from (0, 0)
//                                 V'_i = V_i - sum_l u_l[i] c_l      the sum over ascending l from (0, 0), then one csub
//   derived:  a = zscan_abs(V)
//             rss[s][i] = sqrt(sum_f (re re + im im))                sequentially over ascending f from 0.0, over ALL grid points
//             per (f, i) over the scenarios:  vmax, varg: the total order of wave_key / wave_peak_combine (a NaN is the maximum, ties to the
//                                             smallest s);  vsum = sum_s a,  vsumsq = sum_s a a   sequentially over ascending s from 0.0
//             rss_max, rss_arg, rss_sum, rss_sumsq: the same four of rss[s][i] over s
// The sums over s and over f are carried from chunk to chunk in ascending order (frequency chunks in the outer loop, scenario chunks in the inner
// one), so every output is bit-identical for every chunking.
#pragma once
#include "hpf_zscan.hpp"

namespace hpf {

constexpr int PEN_MAX_S = 1 << 16;
// S n (the carried rss sums), and n Fc Sc of a forced chunking (r of one chunk: every launch's one-dimensional grid and every int j stay in range)
constexpr long long PEN_MAX_SN = 1ll << 27, PEN_MAX_NJ = 1ll << 30;
// start value of a running maximum's argument: loses against every scenario
constexpr int PEN_NO_S = 0x7fffffff;

// scratch in complex values.  Per frequency point: w, t | Z (the column walks read it) | y_extra and its staging | the tie columns | W^-1;
// per (point, scenario): r | the staging buffer of I and V (stage_rows) | the tie coefficients
inline size_t pen_per_f(int n, int k, bool has_x) {
    return (size_t)2 * n + (k ? n : 0) + (has_x ? (size_t)2 * n : 0) + (size_t)2 * k * n + (size_t)k * k;
}
inline size_t pen_stage_rows(int n, int n_inj, bool want_V) {
    const size_t a = (size_t)n_inj, b = want_V ? n : 0;
    return a > b ? a : b;
}
inline size_t pen_per_j(int n, int k, int n_inj, bool want_V) { return (size_t)n + pen_stage_rows(n, n_inj, want_V) + k; }

// chunk lengths (Fc points, Sc scenarios): forced values as given (clipped to F, S); automatic ones (0) the largest that keep
// Fc (per_f + Sc per_j) complex values of scratch under ZSCAN_SCRATCH_BYTES -- all scenarios first, then as many points as fit; where one point with
// all scenarios does not fit, one point and as many scenarios as fit (a multiple of 64 from 64 on).  per_f: w, t, Z, y_extra, the tie columns, W^-1
// per frequency point; per_j: r, the staging buffer and the tie coefficients per (point, scenario).
inline void pen_chunks(int F, int S, int chunk_f, int chunk_s, size_t per_f, size_t per_j, int& Fc, int& Sc) {
    const size_t B = ZSCAN_SCRATCH_BYTES / sizeof(cplx);
    Fc = chunk_f > 0 ? (chunk_f < F ? chunk_f : F) : 0;
    Sc = chunk_s > 0 ? (chunk_s < S ? chunk_s : S) : 0;
    if (!Sc) {
        const size_t fc = Fc ? (size_t)Fc : 1, room = B / fc > per_f ? B / fc - per_f : 0;
        size_t c = room / per_j;
        if (c >= 64) c = c / 64 * 64;
        if (c < 1) c = 1;
        Sc = c < (size_t)S ? (int)c : S;
    }
    if (!Fc) {
        size_t c = B / (per_f + (size_t)Sc * per_j);
        if (c < 1) c = 1;
        Fc = c < (size_t)F ? (int)c : F;
    }
}

// upward step of bus i at j: r [n][J] holds b_i and the children's finished r; t [n][Fc]
HPF_DIST_HD cplx pen_up(const int* child_ptr, const int* child, int i, const cplx* t, const cplx* r, size_t Fc, size_t J, size_t f, size_t j) {
    cplx acc = r[(size_t)i * J + j];
    for (int p = child_ptr[i]; p < child_ptr[i + 1]; ++p) {
        const int c = child[p];
        const cplx tc = t[(size_t)c * Fc + f];
        acc = cadd(acc, cmul_unf(tc, r[(size_t)c * J + j]));
    }
    return acc;
}

// downward step: V_i from w_i, r_i, t_i and the parent's V; the root
HPF_DIST_HD cplx pen_down(cplx w_i, cplx r_i, cplx t_i, cplx v_p) { return cadd(cmul_unf(w_i, r_i), cmul_unf(t_i, v_p)); }
HPF_DIST_HD cplx pen_down_root(cplx w_0, cplx r_0) { return cmul_unf(w_0, r_0); }

// ties: c_l of j -> coef [k][J].  ta / tb [k] the ties' end buses; Winv [k k][Fc]; V [n][J]
HPF_DIST_HD void pen_tie_coef(int k, const int* ta, const int* tb, const cplx* Winv, const cplx* V, size_t Fc, size_t J, size_t f, size_t j, cplx* coef) {
    cplx d[ZSCAN_MAX_TIES];
    for (int m = 0; m < k; ++m) d[m] = csub(V[(size_t)ta[m] * J + j], V[(size_t)tb[m] * J + j]);
    for (int l = 0; l < k; ++l) {
        cplx c = {0.0, 0.0};
        for (int m = 0; m < k; ++m) c = cadd(c, cmul_unf(Winv[((size_t)l * k + m) * Fc + f], d[m]));
        coef[(size_t)l * J + j] = c;
    }
}

// ties: V'_i of j.  tc = the 2 k tie columns [n][Fc]
HPF_DIST_HD cplx pen_tie_fix(int k, const cplx* tc, const cplx* coef, size_t n, size_t Fc, size_t J, size_t f, size_t j, int i, cplx v) {
    cplx acc = {0.0, 0.0};
    for (int l = 0; l < k; ++l) acc = cadd(acc, cmul_unf(zscan_tie_u(tc, n, Fc, f, l, i), coef[(size_t)l * J + j]));
    return csub(v, acc);
}

// one term of rss's sum of squares
HPF_DIST_HD double pen_sq(cplx v) { return v.re * v.re + v.im * v.im; }

// the four running statistics of one quantity: value a of scenario s joins (key, arg, sum, sumsq)
struct PenStat {
    uint64_t key;
    int arg;
    double sum, sumsq;
};
HPF_DIST_HD PenStat pen_stat_start() { return {0ull, PEN_NO_S, 0.0, 0.0}; }
HPF_DIST_HD void pen_stat_add(PenStat& st, double a, int s) {
    wave_peak_combine(st.key, st.arg, wave_key(a), s);
    st.sum = st.sum + a;
    st.sumsq = st.sumsq + a * a;
}

}  // namespace hpf
