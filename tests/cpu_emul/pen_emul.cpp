// Host emulation of hpf_penetration: the functions of csrc/hpf_penetration.hpp (and, for the factor, of csrc/hpf_zscan.hpp) run serially in the
// kernels' order (hpf_zscan.hip) -- frequency chunks in the outer loop, scenario chunks in the inner one; per frequency chunk the factor (upward
// walk, and for ties the downward walk, the tie columns and W^-1), per scenario chunk the scatter, the two walks of the right-hand sides, the tie
// correction and the folds; arrays [bus][fc] and [bus][fc sc] like the device's.  Test infrastructure only.
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "hpf_penetration.hpp"

using namespace hpf;

extern "C" int emul_penetration(int n, int nb, const int32_t* from, const int32_t* to, const double* R, const double* X, const double* gsh,
                                const double* bsh, const double* xsh, int F, const double* h, const cplx* y_extra, int S, int n_inj,
                                const int32_t* inj, const cplx* I, int chunk_f, int chunk_s, cplx* V, double* rss, double* vmax, int32_t* varg,
                                double* vsum, double* vsumsq, double* rss_max, int32_t* rss_arg, double* rss_sum, double* rss_sumsq) {
    ZscanPlan P;
    const int rc = zscan_plan(n, nb, from, to, P);
    if (rc != HPF_OK) return rc;
    const int k = (int)P.tie.size(), ncol = 2 * k;
    std::vector<int> colbus, ta(k), tb(k);
    std::vector<double> tR(k), tX(k);
    for (int l = 0; l < k; ++l) {
        ta[l] = from[P.tie[l]], tb[l] = to[P.tie[l]];
        tR[l] = R[P.tie[l]], tX[l] = X[P.tie[l]];
        colbus.push_back(ta[l]);
        colbus.push_back(tb[l]);
    }
    std::vector<unsigned char> path((size_t)ncol * n, 0);
    for (int s = 0; s < ncol; ++s) zscan_mark_path(P, colbus[s], path.data() + (size_t)s * n);
    const size_t stage_rows = std::max<size_t>((size_t)n_inj, V ? n : 0);
    const size_t per_f = (size_t)2 * n + (k ? n : 0) + (y_extra ? (size_t)2 * n : 0) + (size_t)ncol * n + (size_t)k * k;
    const size_t per_j = (size_t)n + stage_rows + k;
    int Fc, Sc;
    pen_chunks(F, S, chunk_f, chunk_s, per_f, per_j, Fc, Sc);
    const ZscanView Vw{n, P.parent.data(), P.pbranch.data(), P.child_ptr.data(), P.child.data(), P.inc_ptr.data(), P.inc.data(), R, X, gsh, bsh, xsh};
    std::vector<cplx> w((size_t)n * Fc), t((size_t)n * Fc), Zd((size_t)n * Fc), cols((size_t)ncol * n * Fc), Winv((size_t)k * k * Fc);
    std::vector<cplx> r((size_t)n * Fc * Sc), coef((size_t)k * Fc * Sc);
    std::vector<PenStat> vst((size_t)F * n), rst((size_t)n);
    std::vector<double> sq((size_t)n * S);
    bool bad = false;
    for (int f0 = 0; f0 < F; f0 += Fc) {
        const int fc = std::min(Fc, F - f0);
        const size_t C = (size_t)fc;
        for (int d = P.n_depths - 1; d >= 0; --d)
            for (int q = P.dep_ptr[d]; q < P.dep_ptr[d + 1]; ++q) {
                const int i = P.dep_nodes[q];
                for (int f = 0; f < fc; ++f) {
                    const cplx yx = y_extra ? y_extra[(size_t)(f0 + f) * n + i] : cplx{0.0, 0.0};
                    zscan_up(Vw, i, h[f0 + f], y_extra != nullptr, yx, t.data(), C, (size_t)f, w[i * C + f], t[i * C + f]);
                }
            }
        if (k) {
            for (int d = 0; d < P.n_depths; ++d)
                for (int q = P.dep_ptr[d]; q < P.dep_ptr[d + 1]; ++q) {
                    const int i = P.dep_nodes[q], p = P.parent[i];
                    for (int f = 0; f < fc; ++f) Zd[i * C + f] = p < 0 ? w[i * C + f] : zscan_down(w[i * C + f], t[i * C + f], Zd[p * C + f]);
                }
            for (int s = 0; s < ncol; ++s) {
                cplx* col = cols.data() + (size_t)s * n * C;
                for (int f = 0; f < fc; ++f) zscan_col_walk(Vw.parent, colbus[s], t.data(), Zd.data(), col, C, (size_t)f);
                for (int d = 1; d < P.n_depths; ++d)
                    for (int q = P.dep_ptr[d]; q < P.dep_ptr[d + 1]; ++q) {
                        const int i = P.dep_nodes[q];
                        if (path[(size_t)s * n + i]) continue;
                        for (int f = 0; f < fc; ++f) col[i * C + f] = zscan_col_fill(t[i * C + f], col[P.parent[i] * C + f]);
                    }
            }
            for (int f = 0; f < fc; ++f)
                zscan_tie_winv(k, ta.data(), tb.data(), tR.data(), tX.data(), h[f0 + f], cols.data(), (size_t)n, C, (size_t)f, Winv.data());
        }
        for (int s0 = 0; s0 < S; s0 += Sc) {
            const int sc = std::min(Sc, S - s0);
            const size_t J = (size_t)fc * sc;
            std::fill(r.begin(), r.begin() + (size_t)n * J, cplx{0.0, 0.0});
            for (int q = 0; q < n_inj; ++q)
                for (int f = 0; f < fc; ++f)
                    for (int s = 0; s < sc; ++s) r[(size_t)inj[q] * J + (size_t)f * sc + s] = I[((size_t)(s0 + s) * F + (f0 + f)) * n_inj + q];
            for (int d = P.n_depths - 2; d >= 0; --d)
                for (int q = P.dep_ptr[d]; q < P.dep_ptr[d + 1]; ++q) {
                    const int i = P.dep_nodes[q];
                    if (P.child_ptr[i] == P.child_ptr[i + 1]) continue;
                    for (size_t j = 0; j < J; ++j) r[i * J + j] = pen_up(Vw.child_ptr, Vw.child, i, t.data(), r.data(), C, J, j / sc, j);
                }
            for (int d = 0; d < P.n_depths; ++d)
                for (int q = P.dep_ptr[d]; q < P.dep_ptr[d + 1]; ++q) {
                    const int i = P.dep_nodes[q], p = P.parent[i];
                    for (size_t j = 0; j < J; ++j) {
                        const size_t o = i * J + j, fo = i * C + j / sc;
                        r[o] = p < 0 ? pen_down_root(w[fo], r[o]) : pen_down(w[fo], r[o], t[fo], r[p * J + j]);
                    }
                }
            if (k) {
                for (size_t j = 0; j < J; ++j) pen_tie_coef(k, ta.data(), tb.data(), Winv.data(), r.data(), C, J, j / sc, j, coef.data());
                for (int i = 0; i < n; ++i)
                    for (size_t j = 0; j < J; ++j)
                        r[i * J + j] = pen_tie_fix(k, cols.data(), coef.data(), (size_t)n, C, J, j / sc, j, i, r[i * J + j]);
            }
            for (int i = 0; i < n; ++i)
                for (int f = 0; f < fc; ++f) {
                    PenStat& st = vst[(size_t)(f0 + f) * n + i];
                    if (s0 == 0) st = pen_stat_start();
                    for (int s = 0; s < sc; ++s) {
                        const cplx v = r[i * J + (size_t)f * sc + s];
                        if (!zscan_finite(v)) bad = true;
                        pen_stat_add(st, zscan_abs(v), s0 + s);
                    }
                }
            for (int i = 0; i < n; ++i)
                for (int s = 0; s < sc; ++s) {
                    double acc = f0 == 0 ? 0.0 : sq[(size_t)i * S + s0 + s];
                    for (int f = 0; f < fc; ++f) acc = acc + pen_sq(r[i * J + (size_t)f * sc + s]);
                    sq[(size_t)i * S + s0 + s] = acc;
                }
            if (V)
                for (int s = 0; s < sc; ++s)
                    for (int f = 0; f < fc; ++f)
                        for (int i = 0; i < n; ++i) V[((size_t)(s0 + s) * F + (f0 + f)) * n + i] = r[i * J + (size_t)f * sc + s];
        }
    }
    for (int i = 0; i < n; ++i) {
        rst[i] = pen_stat_start();
        for (int s = 0; s < S; ++s) {
            const double a = sqrt(sq[(size_t)i * S + s]);
            if (rss) rss[(size_t)s * n + i] = a;
            pen_stat_add(rst[i], a, s);
        }
        if (rss_max) rss_max[i] = wave_key_value(rst[i].key);
        if (rss_arg) rss_arg[i] = rst[i].arg;
        if (rss_sum) rss_sum[i] = rst[i].sum;
        if (rss_sumsq) rss_sumsq[i] = rst[i].sumsq;
    }
    for (size_t g = 0; g < (size_t)F * n; ++g) {
        if (vmax) vmax[g] = wave_key_value(vst[g].key);
        if (varg) varg[g] = vst[g].arg;
        if (vsum) vsum[g] = vst[g].sum;
        if (vsumsq) vsumsq[g] = vst[g].sumsq;
    }
    return bad ? HPF_E_SINGULAR : HPF_OK;
}

// the automatic / forced chunk lengths the call would use -> Fc, Sc
extern "C" void emul_pen_chunks(int F, int S, int chunk_f, int chunk_s, long long per_f, long long per_j, int32_t* Fc, int32_t* Sc) {
    int a, b;
    pen_chunks(F, S, chunk_f, chunk_s, (size_t)per_f, (size_t)per_j, a, b);
    *Fc = a, *Sc = b;
}
