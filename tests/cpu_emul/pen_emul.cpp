// Host emulation of hpf_penetration: the functions of csrc/hpf_penetration.hpp (and, for the factor, of csrc/hpf_zscan.hpp) run serially in the
// kernels' order (hpf_zscan.hip) -- frequency chunks in the outer loop, scenario chunks in the inner one; per frequency chunk the factor, per
// scenario chunk the scatter, the solve (both of zfactor_emul.hpp) and the folds; arrays [bus][fc] and [bus][fc sc] like the device's.  Test
// infrastructure only.
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "zfactor_emul.hpp"

using namespace hpf;

extern "C" int emul_penetration(int n, int nb, const int32_t* from, const int32_t* to, const double* R, const double* X, const double* gsh,
                                const double* bsh, const double* xsh, int F, const double* h, const cplx* y_extra, int S, int n_inj,
                                const int32_t* inj, const cplx* I, int chunk_f, int chunk_s, cplx* V, double* rss, double* vmax, int32_t* varg,
                                double* vsum, double* vsumsq, double* rss_max, int32_t* rss_arg, double* rss_sum, double* rss_sumsq) {
    EmulFactor E;
    const int rc = E.plan(n, nb, from, to, R, X, gsh, bsh, xsh);
    if (rc != HPF_OK) return rc;
    const int k = E.T.k;
    int Fc, Sc;
    pen_chunks(F, S, chunk_f, chunk_s, pen_per_f(n, k, y_extra != nullptr), pen_per_j(n, k, n_inj, V != nullptr), Fc, Sc);
    E.size(Fc, false);
    std::vector<cplx> r((size_t)n * Fc * Sc), coef((size_t)k * Fc * Sc);
    std::vector<PenStat> vst((size_t)F * n), rst((size_t)n);
    std::vector<double> sq((size_t)n * S);
    bool bad = false;
    for (int f0 = 0; f0 < F; f0 += Fc) {
        const int fc = std::min(Fc, F - f0);
        emul_factor(E, h, y_extra, f0, fc);
        for (int s0 = 0; s0 < S; s0 += Sc) {
            const int sc = std::min(Sc, S - s0);
            const size_t J = (size_t)fc * sc;
            std::fill(r.begin(), r.begin() + (size_t)n * J, cplx{0.0, 0.0});
            for (int q = 0; q < n_inj; ++q)
                for (int f = 0; f < fc; ++f)
                    for (int s = 0; s < sc; ++s) r[(size_t)inj[q] * J + (size_t)f * sc + s] = I[((size_t)(s0 + s) * F + (f0 + f)) * n_inj + q];
            emul_solve(E, fc, sc, r.data(), coef.data());
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

// the scratch-size formulas
extern "C" long long emul_pen_per_f(int n, int k, int has_x) { return (long long)pen_per_f(n, k, has_x); }
extern "C" long long emul_pen_per_j(int n, int k, int n_inj, int want_V) { return (long long)pen_per_j(n, k, n_inj, want_V); }

// the automatic / forced chunk lengths the call would use -> Fc, Sc
extern "C" void emul_pen_chunks(int F, int S, int chunk_f, int chunk_s, long long per_f, long long per_j, int32_t* Fc, int32_t* Sc) {
    int a, b;
    pen_chunks(F, S, chunk_f, chunk_s, (size_t)per_f, (size_t)per_j, a, b);
    *Fc = a, *Sc = b;
}
