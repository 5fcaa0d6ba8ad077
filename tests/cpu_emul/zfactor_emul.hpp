// Host equivalents of ZsFactor::factor and ZsFactor::solve (hpf_zscan.hip), shared by zscan_emul.cpp, pen_emul.cpp and rma_emul.cpp: the
// functions of csrc/hpf_zscan.hpp and csrc/hpf_penetration.hpp run serially in the kernels' order; arrays [bus][fc] and [bus][fc sc] like the
// device's.  Test infrastructure only.
#pragma once
#include <vector>

#include "hpf_penetration.hpp"

namespace hpf {

// the plan, the ties and the factor of one chunk of at most Fc points; Zd where the diagonal is wanted or the tie columns read it
struct EmulFactor {
    ZscanPlan P;
    ZscanTies T;
    ZscanView V{};
    bool diag = false;
    std::vector<cplx> w, t, Zd, cols, Winv;

    // the host part: HPF_OK or HPF_E_TOPOLOGY
    int plan(int n, int nb, const int32_t* from, const int32_t* to, const double* R, const double* X, const double* gsh, const double* bsh,
             const double* xsh, int n_sel = 0, const int32_t* sel = nullptr) {
        const int r = zscan_plan(n, nb, from, to, P);
        if (r != HPF_OK) return r;
        T = zscan_ties(P, from, to, R, X, n_sel, sel);
        V = ZscanView{n, P.parent.data(), P.pbranch.data(), P.child_ptr.data(), P.child.data(), P.inc_ptr.data(), P.inc.data(), R, X, gsh, bsh, xsh};
        return HPF_OK;
    }
    // the arrays of a chunk of Fc points
    void size(int Fc, bool want_diag) {
        const size_t nF = (size_t)P.n * Fc;
        diag = want_diag || T.k;
        w.resize(nF), t.resize(nF), Zd.resize(diag ? nF : 0), cols.resize(T.ncol * nF), Winv.resize((size_t)T.k * T.k * Fc);
    }
    const cplx* tie_cols(size_t fc) const { return cols.data() + (size_t)T.n_sel * P.n * fc; }
};

// the factor of the fc points from f0 on: the upward walk by descending depth, the downward walk by ascending depth, per column the walk and the
// fills, W^-1.  h [F] and y_extra [F][n] (or NULL) are the caller's whole grids
inline void emul_factor(EmulFactor& E, const double* h, const cplx* y_extra, int f0, int fc) {
    const ZscanPlan& P = E.P;
    const ZscanTies& T = E.T;
    const int n = P.n;
    const size_t C = (size_t)fc;
    std::vector<cplx>& w = E.w;
    std::vector<cplx>& t = E.t;
    std::vector<cplx>& Zd = E.Zd;
    for (int d = P.n_depths - 1; d >= 0; --d)
        for (int q = P.dep_ptr[d]; q < P.dep_ptr[d + 1]; ++q) {
            const int i = P.dep_nodes[q];
            for (int f = 0; f < fc; ++f) {
                const cplx yx = y_extra ? y_extra[(size_t)(f0 + f) * n + i] : cplx{0.0, 0.0};
                zscan_up(E.V, i, h[f0 + f], y_extra != nullptr, yx, t.data(), C, (size_t)f, w[i * C + f], t[i * C + f]);
            }
        }
    if (E.diag)
        for (int d = 0; d < P.n_depths; ++d)
            for (int q = P.dep_ptr[d]; q < P.dep_ptr[d + 1]; ++q) {
                const int i = P.dep_nodes[q], p = P.parent[i];
                for (int f = 0; f < fc; ++f) Zd[i * C + f] = p < 0 ? w[i * C + f] : zscan_down(w[i * C + f], t[i * C + f], Zd[p * C + f]);
            }
    for (int s = 0; s < T.ncol; ++s) {
        cplx* col = E.cols.data() + (size_t)s * n * C;
        for (int f = 0; f < fc; ++f) zscan_col_walk(E.V.parent, T.colbus[s], t.data(), Zd.data(), col, C, (size_t)f);
        for (int d = 1; d < P.n_depths; ++d)
            for (int q = P.dep_ptr[d]; q < P.dep_ptr[d + 1]; ++q) {
                const int i = P.dep_nodes[q];
                if (T.path[(size_t)s * n + i]) continue;
                for (int f = 0; f < fc; ++f) col[i * C + f] = zscan_col_fill(t[i * C + f], col[P.parent[i] * C + f]);
            }
    }
    for (int f = 0; T.k && f < fc; ++f)
        zscan_tie_winv(T.k, T.ta.data(), T.tb.data(), T.tR.data(), T.tX.data(), h[f0 + f], E.tie_cols(C), (size_t)n, C, (size_t)f, E.Winv.data());
}

// r [n][fc sc] <- Y^-1 r in place with the factor of the chunk: the two walks of the right-hand sides and the tie correction; coef [k][fc sc]
inline void emul_solve(const EmulFactor& E, int fc, int sc, cplx* r, cplx* coef) {
    const ZscanPlan& P = E.P;
    const int n = P.n, k = E.T.k;
    const size_t C = (size_t)fc, J = C * sc;
    for (int d = P.n_depths - 2; d >= 0; --d)
        for (int q = P.dep_ptr[d]; q < P.dep_ptr[d + 1]; ++q) {
            const int i = P.dep_nodes[q];
            if (P.child_ptr[i] == P.child_ptr[i + 1]) continue;
            for (size_t j = 0; j < J; ++j) r[i * J + j] = pen_up(E.V.child_ptr, E.V.child, i, E.t.data(), r, C, J, j / sc, j);
        }
    for (int d = 0; d < P.n_depths; ++d)
        for (int q = P.dep_ptr[d]; q < P.dep_ptr[d + 1]; ++q) {
            const int i = P.dep_nodes[q], p = P.parent[i];
            for (size_t j = 0; j < J; ++j) {
                const size_t o = i * J + j, fo = i * C + j / sc;
                r[o] = p < 0 ? pen_down_root(E.w[fo], r[o]) : pen_down(E.w[fo], r[o], E.t[fo], r[p * J + j]);
            }
        }
    if (k) {
        for (size_t j = 0; j < J; ++j) pen_tie_coef(k, E.T.ta.data(), E.T.tb.data(), E.Winv.data(), r, C, J, j / sc, j, coef);
        for (int i = 0; i < n; ++i)
            for (size_t j = 0; j < J; ++j) r[i * J + j] = pen_tie_fix(k, E.tie_cols(C), coef, (size_t)n, C, J, j / sc, j, i, r[i * J + j]);
    }
}

}  // namespace hpf
