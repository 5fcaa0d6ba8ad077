// Host emulation of hpf_impedance_scan: the functions of csrc/hpf_zscan.hpp run serially in the kernels' order (hpf_zscan.hip) -- per chunk of
// frequency points the upward walk by descending depth, the downward walk by ascending depth, the column walks and fills, the tie correction, the
// peak fold; arrays [bus][fc] like the device's.  Test infrastructure only.
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "hpf_zscan.hpp"

using namespace hpf;

extern "C" int emul_zscan(int n, int nb, const int32_t* from, const int32_t* to, const double* R, const double* X, const double* gsh,
                          const double* bsh, const double* xsh, int F, const double* h, const cplx* y_extra, int n_sel, const int32_t* sel,
                          int chunk, cplx* Z, cplx* Zt, double* zpeak, int32_t* fpeak) {
    ZscanPlan P;
    const int r = zscan_plan(n, nb, from, to, P);
    if (r != HPF_OK) return r;
    const int k = (int)P.tie.size(), ncol = n_sel + 2 * k;
    std::vector<int> colbus(sel, sel + n_sel), ta(k), tb(k);
    std::vector<double> tR(k), tX(k);
    for (int l = 0; l < k; ++l) {
        ta[l] = from[P.tie[l]], tb[l] = to[P.tie[l]];
        tR[l] = R[P.tie[l]], tX[l] = X[P.tie[l]];
        colbus.push_back(ta[l]);
        colbus.push_back(tb[l]);
    }
    std::vector<unsigned char> path((size_t)ncol * n, 0);
    for (int s = 0; s < ncol; ++s) zscan_mark_path(P, colbus[s], path.data() + (size_t)s * n);
    const size_t stage_rows = std::max<size_t>((Z || y_extra) ? n : 0, (size_t)n_sel * n);
    const int Fc = zscan_chunk(F, chunk, (size_t)3 * n + (y_extra ? n : 0) + (size_t)ncol * n + (size_t)k * k + stage_rows);
    const ZscanView V{n, P.parent.data(), P.pbranch.data(), P.child_ptr.data(), P.child.data(), P.inc_ptr.data(), P.inc.data(), R, X, gsh, bsh, xsh};
    std::vector<uint64_t> pkey(n, 0);
    std::vector<int> pf(n, ZSCAN_NO_F), bad(n, 0);
    std::vector<cplx> w((size_t)n * Fc), t((size_t)n * Fc), Zd((size_t)n * Fc), cols((size_t)ncol * n * Fc), Winv((size_t)k * k * Fc);
    for (int f0 = 0; f0 < F; f0 += Fc) {
        const int fc = std::min(Fc, F - f0);
        const size_t S = (size_t)fc;
        for (int d = P.n_depths - 1; d >= 0; --d)
            for (int q = P.dep_ptr[d]; q < P.dep_ptr[d + 1]; ++q) {
                const int i = P.dep_nodes[q];
                for (int f = 0; f < fc; ++f) {
                    const cplx yx = y_extra ? y_extra[(size_t)(f0 + f) * n + i] : cplx{0.0, 0.0};
                    zscan_up(V, i, h[f0 + f], y_extra != nullptr, yx, t.data(), S, (size_t)f, w[i * S + f], t[i * S + f]);
                }
            }
        for (int d = 0; d < P.n_depths; ++d)
            for (int q = P.dep_ptr[d]; q < P.dep_ptr[d + 1]; ++q) {
                const int i = P.dep_nodes[q], p = P.parent[i];
                for (int f = 0; f < fc; ++f) Zd[i * S + f] = p < 0 ? w[i * S + f] : zscan_down(w[i * S + f], t[i * S + f], Zd[p * S + f]);
            }
        for (int s = 0; s < ncol; ++s) {
            cplx* col = cols.data() + (size_t)s * n * S;
            for (int f = 0; f < fc; ++f) zscan_col_walk(V.parent, colbus[s], t.data(), Zd.data(), col, S, (size_t)f);
            for (int d = 1; d < P.n_depths; ++d)
                for (int q = P.dep_ptr[d]; q < P.dep_ptr[d + 1]; ++q) {
                    const int i = P.dep_nodes[q];
                    if (path[(size_t)s * n + i]) continue;
                    for (int f = 0; f < fc; ++f) col[i * S + f] = zscan_col_fill(t[i * S + f], col[P.parent[i] * S + f]);
                }
        }
        if (k) {
            const cplx* tc = cols.data() + (size_t)n_sel * n * S;
            for (int f = 0; f < fc; ++f) zscan_tie_winv(k, ta.data(), tb.data(), tR.data(), tX.data(), h[f0 + f], tc, (size_t)n, S, (size_t)f, Winv.data());
            for (int i = 0; i < n; ++i)
                for (int f = 0; f < fc; ++f) Zd[i * S + f] = csub(Zd[i * S + f], zscan_tie_form(k, tc, Winv.data(), (size_t)n, S, (size_t)f, i, i));
            for (int s = 0; s < n_sel; ++s)
                for (int i = 0; i < n; ++i)
                    for (int f = 0; f < fc; ++f) {
                        cplx& z = cols[((size_t)s * n + i) * S + f];
                        z = csub(z, zscan_tie_form(k, tc, Winv.data(), (size_t)n, S, (size_t)f, i, colbus[s]));
                    }
        }
        for (int i = 0; i < n; ++i) {
            uint64_t key = 0;
            int fbest = ZSCAN_NO_F;
            for (int f = 0; f < fc; ++f) {
                const cplx z = Zd[i * S + f];
                if (!zscan_finite(z)) bad[i] = 1;
                wave_peak_combine(key, fbest, wave_key(zscan_abs(z)), f0 + f);
            }
            wave_peak_combine(pkey[i], pf[i], key, fbest);
        }
        for (int f = 0; f < fc; ++f)
            for (int i = 0; i < n; ++i) {
                if (Z) Z[(size_t)(f0 + f) * n + i] = Zd[i * S + f];
                for (int s = 0; s < n_sel; ++s) Zt[((size_t)(f0 + f) * n_sel + s) * n + i] = cols[((size_t)s * n + i) * S + f];
            }
    }
    bool singular = false;
    for (int i = 0; i < n; ++i) {
        zpeak[i] = wave_key_value(pkey[i]);
        fpeak[i] = pf[i];
        singular |= bad[i] != 0;
    }
    return singular ? HPF_E_SINGULAR : HPF_OK;
}

// the planner alone: parent, parent branch, depth [n]; ties [HPF_ZSCAN_MAX_TIES] -> number of ties, or the planner's error code
extern "C" int emul_zscan_plan(int n, int nb, const int32_t* from, const int32_t* to, int32_t* parent, int32_t* pbranch, int32_t* depth,
                               int32_t* ties) {
    ZscanPlan P;
    const int r = zscan_plan(n, nb, from, to, P);
    if (r != HPF_OK) return r;
    for (int i = 0; i < n; ++i) parent[i] = P.parent[i], pbranch[i] = P.pbranch[i], depth[i] = P.depth[i];
    for (size_t l = 0; l < P.tie.size(); ++l) ties[l] = P.tie[l];
    return (int)P.tie.size();
}
