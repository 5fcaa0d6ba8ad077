// Host emulation of hpf_resonance_modes: the functions of csrc/hpf_resonance.hpp (for y = Y^-1 x those of csrc/hpf_penetration.hpp with one
// scenario, for the factor those of csrc/hpf_zscan.hpp) run serially in the kernels' order (hpf_zscan.hip) -- per chunk of frequency points the
// factor (upward walk, and for ties the downward walk, the tie columns and W^-1), the start vector, `iters` times the two walks of the right-hand
// side, the tie correction, the pivot per tile and over the tiles and the scaling, then the tile sums and their fold, the eigenpair, the
// participation factors and the residual; arrays [bus][fc] and [tile][fc] like the device's.  Test infrastructure only.
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "hpf_resonance.hpp"

using namespace hpf;

extern "C" int emul_resonance_modes(int n, int nb, const int32_t* from, const int32_t* to, const double* R, const double* X, const double* gsh,
                                    const double* bsh, const double* xsh, int F, const double* h, const cplx* y_extra, int iters, int chunk,
                                    cplx* lam, double* zm, double* res, int32_t* top, cplx* pf) {
    if (iters < 1 || iters > RMA_MAX_ITERS) return HPF_E_ARG;
    ZscanPlan P;
    const int rc = zscan_plan(n, nb, from, to, P);
    if (rc != HPF_OK) return rc;
    const int k = (int)P.tie.size(), ncol = 2 * k, tiles = rma_tiles(n);
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
    const int Fc = zscan_chunk(F, chunk, rma_per_f(n, k, y_extra != nullptr, pf != nullptr));
    const ZscanView Vw{n, P.parent.data(), P.pbranch.data(), P.child_ptr.data(), P.child.data(), P.inc_ptr.data(), P.inc.data(), R, X, gsh, bsh, xsh};
    std::vector<cplx> w((size_t)n * Fc), t((size_t)n * Fc), Zd((size_t)(k ? n : 0) * Fc), cols((size_t)ncol * n * Fc), Winv((size_t)k * k * Fc);
    std::vector<cplx> x((size_t)n * Fc), y((size_t)n * Fc), coef((size_t)k * Fc), part((size_t)3 * tiles * Fc), sums((size_t)3 * Fc), yp(Fc);
    std::vector<uint64_t> pkey((size_t)tiles * Fc);
    std::vector<int> parg((size_t)tiles * Fc), piv(Fc);
    bool bad = false;
    for (int f0 = 0; f0 < F; f0 += Fc) {
        const int fc = std::min(Fc, F - f0);
        const size_t C = (size_t)fc, q = (size_t)tiles * C;
        for (int d = P.n_depths - 1; d >= 0; --d)
            for (int s = P.dep_ptr[d]; s < P.dep_ptr[d + 1]; ++s) {
                const int i = P.dep_nodes[s];
                for (int f = 0; f < fc; ++f) {
                    const cplx yx = y_extra ? y_extra[(size_t)(f0 + f) * n + i] : cplx{0.0, 0.0};
                    zscan_up(Vw, i, h[f0 + f], y_extra != nullptr, yx, t.data(), C, (size_t)f, w[i * C + f], t[i * C + f]);
                }
            }
        if (k) {
            for (int d = 0; d < P.n_depths; ++d)
                for (int s = P.dep_ptr[d]; s < P.dep_ptr[d + 1]; ++s) {
                    const int i = P.dep_nodes[s], p = P.parent[i];
                    for (int f = 0; f < fc; ++f) Zd[i * C + f] = p < 0 ? w[i * C + f] : zscan_down(w[i * C + f], t[i * C + f], Zd[p * C + f]);
                }
            for (int s = 0; s < ncol; ++s) {
                cplx* col = cols.data() + (size_t)s * n * C;
                for (int f = 0; f < fc; ++f) zscan_col_walk(Vw.parent, colbus[s], t.data(), Zd.data(), col, C, (size_t)f);
                for (int d = 1; d < P.n_depths; ++d)
                    for (int u = P.dep_ptr[d]; u < P.dep_ptr[d + 1]; ++u) {
                        const int i = P.dep_nodes[u];
                        if (path[(size_t)s * n + i]) continue;
                        for (int f = 0; f < fc; ++f) col[i * C + f] = zscan_col_fill(t[i * C + f], col[P.parent[i] * C + f]);
                    }
            }
            for (int f = 0; f < fc; ++f)
                zscan_tie_winv(k, ta.data(), tb.data(), tR.data(), tX.data(), h[f0 + f], cols.data(), (size_t)n, C, (size_t)f, Winv.data());
        }
        for (int i = 0; i < n; ++i)
            for (int f = 0; f < fc; ++f) x[i * C + f] = y[i * C + f] = rma_start(i, n);
        for (int it = 1; it <= iters; ++it) {
            for (int d = P.n_depths - 2; d >= 0; --d)
                for (int s = P.dep_ptr[d]; s < P.dep_ptr[d + 1]; ++s) {
                    const int i = P.dep_nodes[s];
                    if (P.child_ptr[i] == P.child_ptr[i + 1]) continue;
                    for (size_t j = 0; j < C; ++j) y[i * C + j] = pen_up(Vw.child_ptr, Vw.child, i, t.data(), y.data(), C, C, j, j);
                }
            for (int d = 0; d < P.n_depths; ++d)
                for (int s = P.dep_ptr[d]; s < P.dep_ptr[d + 1]; ++s) {
                    const int i = P.dep_nodes[s], p = P.parent[i];
                    for (size_t j = 0; j < C; ++j) {
                        const size_t o = i * C + j;
                        y[o] = p < 0 ? pen_down_root(w[o], y[o]) : pen_down(w[o], y[o], t[o], y[p * C + j]);
                    }
                }
            if (k) {
                for (size_t j = 0; j < C; ++j) pen_tie_coef(k, ta.data(), tb.data(), Winv.data(), y.data(), C, C, j, j, coef.data());
                for (int i = 0; i < n; ++i)
                    for (size_t j = 0; j < C; ++j) y[i * C + j] = pen_tie_fix(k, cols.data(), coef.data(), (size_t)n, C, C, j, j, i, y[i * C + j]);
            }
            for (int T = 0; T < tiles; ++T)
                for (size_t f = 0; f < C; ++f) rma_tile_peak(y.data(), n, C, f, T, pkey[T * C + f], parg[T * C + f]);
            for (size_t f = 0; f < C; ++f) {
                uint64_t key;
                rma_peak_fold(pkey.data(), parg.data(), tiles, C, f, key, piv[f]);
                yp[f] = y[(size_t)piv[f] * C + f];
            }
            if (it < iters)
                for (int i = 0; i < n; ++i)
                    for (size_t f = 0; f < C; ++f) x[i * C + f] = y[i * C + f] = rma_scale(y[i * C + f], yp[f]);
        }
        for (int T = 0; T < tiles; ++T)
            for (size_t f = 0; f < C; ++f)
                rma_tile_sums(x.data(), y.data(), n, C, f, T, part[T * C + f], part[q + T * C + f], part[2 * q + T * C + f]);
        for (size_t f = 0; f < C; ++f)
            for (int s = 0; s < 3; ++s) sums[s * C + f] = rma_sum_fold(part.data() + s * q, tiles, C, f);
        for (size_t f = 0; f < C; ++f) {
            cplx l, ginv;
            double z;
            rma_eig(sums[f], sums[C + f], sums[2 * C + f], l, z, ginv);
            uint64_t key = 0;
            int arg = RMA_NO_BUS;
            for (int i = 0; i < n; ++i) {
                const cplx yi = y[i * C + f], p = rma_pf(yi, ginv);
                if (!zscan_finite(p)) bad = true;
                if (pf) pf[(size_t)(f0 + f) * n + i] = p;
                wave_peak_combine(key, arg, wave_key(rma_defect(x[i * C + f], l, yi)), i);
            }
            const double r = rma_res(key, l, yp[f]);
            if (!zscan_finite(l) || !rma_finite(z) || !rma_finite(r)) bad = true;
            if (lam) lam[f0 + f] = l;
            if (zm) zm[f0 + f] = z;
            if (res) res[f0 + f] = r;
            if (top) top[f0 + f] = piv[f];
        }
    }
    return bad ? HPF_E_SINGULAR : HPF_OK;
}
