// Impedance scan (hpf_impedance_scan): driving-point impedances Z_ii(h) and transfer columns Z_ij(h) of the network over a grid of real harmonic
// orders h > 0 -- the diagonal and selected columns of Y(h)^-1 without ever storing a matrix.  The kernels of hpf_zscan.hip run these functions on
// the device, one thread per (bus, frequency point); the host emulation (tests/cpu_emul/zscan_emul.cpp) runs the same functions serially.  Every
// product, sum and quotient is rounded on its own (-ffp-contract=off), every sum has one fixed order, nothing is atomic: device == emulation bit for
// bit, for every chunk length.
//
// Model (admittance.line_model): branch e = (from < to) with R_e, X_e; bus i with gsh_i, bsh_i, xsh_i; optional y_extra[f][i].
//   y_e(h)  = crecip((R_e, h X_e))                                  crecip(a) = (a.re / d, -a.im / d), d = a.re a.re + a.im a.im
//   Y_ij    = -y_e
//   Y_ii    = sum_{e at i} y_e + (gsh_i, h bsh_i) + [xsh_i != 0 and h != 1] (0, -1 / (xsh_i h)) + y_extra[f][i]
// The planner walks a BFS spanning tree from bus 0 (neighbours in ascending branch index): parent p(i), parent branch e(i), children in ascending
// bus index, the buses of each depth in BFS order; the branches off the tree are the ties (ascending branch index), at most HPF_ZSCAN_MAX_TIES.
//
// Per frequency point, in complex scalars (cmul_unf, cadd, csub of hpf_assembly.hpp):
//   D_i   = ((((0 + y_e1) + y_e2) + ...) + (gsh_i, h bsh_i)) [+ (0, -1 / (xsh_i h))] [+ y_extra]     e1 < e2 < ...: the TREE branches at i
//   up    (deepest depth first):  S_i = (((D_i - y_e(c1) t_c1) - y_e(c2) t_c2) - ...)   c1 < c2 < ...: the children of i
//                                 w_i = crecip(S_i),  t_i = y_e(i) w_i  (root: t = 0)
//   down  (root first):           Z_00 = w_0,  Z_cc = w_c + t_c (t_c Z_pp),  p = p(c)
//   column j:  col[j] = Z_jj;  prod = t_j;  for every ancestor a of j, nearest first:  col[a] = prod Z_aa,  prod = prod t_a;
//              every other bus i by ascending depth:  col[i] = t_i col[p(i)]
//   ties l < k, tie l = branch (a_l, b_l):  u_l[i] = col(a_l)[i] - col(b_l)[i]
//              W_lm = u_m[a_l] - u_m[b_l]  (l != m),   W_ll = (R_l, h X_l) + (u_l[a_l] - u_l[b_l])            ((R, h X) = 1 / y_l exactly)
//              Winv = W^-1: Gaussian elimination of [W | I] with partial pivoting (the largest re^2 + im^2 of the column, ties to the smallest
//                     row), multipliers m = A_rc crecip(A_cc), A_r. = A_r. - m A_c.; back substitution x_r = (b_r - sum_{c > r ascending} A_rc x_c) crecip(A_rr)
//              q(i, j) = sum_l u_l[i] v_l  over ascending l from 0,  v_l = sum_m Winv_lm u_m[j]  over ascending m from 0
//              Z'_ii = Z_ii - q(i, i);  selected column j:  Z'_ij = Z_ij - q(i, j)
//   peak:  |z| = sqrt(re re + im im);  zpeak[i] = max_f |Z_ii|, fpeak[i] the smallest such f; a NaN is the peak (wave_key / wave_peak_combine of
//          hpf_waveform.hpp: a total order, so lanes, wave reduction and chunks may combine in any grouping)
// All per-chunk arrays are [bus][Fc] (the frequency fastest): a wavefront reads and writes 64 consecutive 16-byte values.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/hpf.h"
#include "hpf_assembly.hpp"
#include "hpf_distortion.hpp"
#include "hpf_waveform.hpp"

namespace hpf {

constexpr int ZSCAN_MAX_TIES = HPF_ZSCAN_MAX_TIES, ZSCAN_MAX_SEL = HPF_ZSCAN_MAX_SEL, ZSCAN_MAX_F = 1 << 20, ZSCAN_MAX_N = 1 << 22;
// budget of the per-chunk device scratch (w, t, Z, y_extra, the columns, W^-1, the staging buffer of the transposed copies): the automatic chunk
// length is the largest multiple of 64 frequency points that fits (at least 64)
constexpr size_t ZSCAN_SCRATCH_BYTES = (size_t)256 << 20;

// ---- host planner ------------------------------------------------------------------------------------------------------------------------------
struct ZscanPlan {
    int n = 0, nb = 0, n_depths = 0;
    std::vector<int> parent, pbranch;        // [n] -1 for bus 0
    std::vector<int> child_ptr, child;       // [n + 1], [n - 1] ascending bus index inside a list
    std::vector<int> inc_ptr, inc;           // [n + 1], [2 (n - 1)] tree branches at a bus, ascending branch index
    std::vector<int> dep_ptr, dep_nodes;     // [n_depths + 1], [n] the buses of each depth, BFS order
    std::vector<int> depth;                  // [n]
    std::vector<int> tie;                    // loop-closing branches, ascending
};

// from / to [nb] valid (0 <= from < to < n, no duplicates: the caller checked).  HPF_OK or HPF_E_TOPOLOGY.
inline int zscan_plan(int n, int nb, const int32_t* from, const int32_t* to, ZscanPlan& P) {
    P = ZscanPlan();
    P.n = n;
    P.nb = nb;
    std::vector<int> adj_ptr((size_t)n + 1, 0), adj((size_t)2 * nb);
    for (int e = 0; e < nb; ++e) {
        adj_ptr[from[e] + 1]++;
        adj_ptr[to[e] + 1]++;
    }
    for (int i = 0; i < n; ++i) adj_ptr[i + 1] += adj_ptr[i];
    {
        std::vector<int> fill(adj_ptr.begin(), adj_ptr.end() - 1);
        for (int e = 0; e < nb; ++e) {                           // ascending branch index inside every list
            adj[fill[from[e]]++] = e;
            adj[fill[to[e]]++] = e;
        }
    }
    P.parent.assign(n, -2);
    P.pbranch.assign(n, -1);
    P.depth.assign(n, 0);
    std::vector<char> in_tree(nb > 0 ? nb : 1, 0);
    P.dep_nodes.reserve(n);
    P.parent[0] = -1;
    P.dep_nodes.push_back(0);
    for (size_t q = 0; q < P.dep_nodes.size(); ++q) {
        const int i = P.dep_nodes[q];
        for (int p = adj_ptr[i]; p < adj_ptr[i + 1]; ++p) {
            const int e = adj[p], j = from[e] == i ? to[e] : from[e];
            if (P.parent[j] == -2) {
                P.parent[j] = i;
                P.pbranch[j] = e;
                P.depth[j] = P.depth[i] + 1;
                in_tree[e] = 1;
                P.dep_nodes.push_back(j);
            }
        }
    }
    if ((int)P.dep_nodes.size() != n) return HPF_E_TOPOLOGY;   // not connected from bus 0
    for (int e = 0; e < nb; ++e)
        if (!in_tree[e]) P.tie.push_back(e);
    if ((int)P.tie.size() > ZSCAN_MAX_TIES) return HPF_E_TOPOLOGY;
    P.n_depths = P.depth[P.dep_nodes.back()] + 1;
    P.dep_ptr.assign((size_t)P.n_depths + 1, 0);
    for (int i = 0; i < n; ++i) P.dep_ptr[P.depth[i] + 1]++;
    for (int d = 0; d < P.n_depths; ++d) P.dep_ptr[d + 1] += P.dep_ptr[d];
    P.child_ptr.assign((size_t)n + 1, 0);
    P.child.assign(n > 1 ? n - 1 : 1, 0);
    for (int i = 1; i < n; ++i) P.child_ptr[P.parent[i] + 1]++;
    for (int i = 0; i < n; ++i) P.child_ptr[i + 1] += P.child_ptr[i];
    {
        std::vector<int> fill(P.child_ptr.begin(), P.child_ptr.end() - 1);
        for (int i = 1; i < n; ++i) P.child[fill[P.parent[i]]++] = i;
    }
    P.inc_ptr.assign((size_t)n + 1, 0);
    P.inc.assign(n > 1 ? (size_t)2 * (n - 1) : 1, 0);
    for (int i = 0; i < n; ++i) {
        int k = P.inc_ptr[i];
        for (int p = adj_ptr[i]; p < adj_ptr[i + 1]; ++p)
            if (in_tree[adj[p]]) P.inc[k++] = adj[p];
        P.inc_ptr[i + 1] = k;
    }
    return HPF_OK;
}

// ancestors-or-self of bus j: mark[i] = 1 (the buses a column walk writes; the fill leaves them alone)
inline void zscan_mark_path(const ZscanPlan& P, int j, unsigned char* mark) {
    for (int a = j; a >= 0; a = P.parent[a]) mark[a] = 1;
}

// the ties and the columns of one call, as the host hands them to the kernels and to the emulation: the columns of the n_sel selected buses first
// (the scan's: they leave as Zt), then col(a_l), col(b_l) of every tie l < k
struct ZscanTies {
    int k = 0, n_sel = 0, ncol = 0;          // ncol = n_sel + 2 k
    std::vector<int> colbus;                 // [ncol]
    std::vector<int> ta, tb;                 // [k] the ties' end buses
    std::vector<double> tR, tX;              // [k] ... and series impedance
    std::vector<unsigned char> path;         // [ncol][n] 1 on the column bus and its ancestors
};

inline ZscanTies zscan_ties(const ZscanPlan& P, const int32_t* from, const int32_t* to, const double* R, const double* X, int n_sel = 0,
                            const int32_t* sel = nullptr) {
    ZscanTies T;
    T.k = (int)P.tie.size(), T.n_sel = n_sel, T.ncol = n_sel + 2 * T.k;
    T.colbus.assign(sel, sel + n_sel);
    for (int e : P.tie) {
        T.ta.push_back(from[e]), T.tb.push_back(to[e]);
        T.tR.push_back(R[e]), T.tX.push_back(X[e]);
        T.colbus.push_back(from[e]);
        T.colbus.push_back(to[e]);
    }
    T.path.assign((size_t)T.ncol * P.n, 0);
    for (int s = 0; s < T.ncol; ++s) zscan_mark_path(P, T.colbus[s], T.path.data() + (size_t)s * P.n);
    return T;
}

// the scan's scratch per frequency point, in complex values: w, t, Zd | y_extra | the columns | W^-1 | the staging buffer of the transposed copies
// (stage_rows: y_extra in and Z out take n, the selected columns out n_sel n)
inline size_t zscan_stage_rows(int n, int n_sel, bool has_x, bool want_Z) {
    const size_t a = (want_Z || has_x) ? n : 0, b = (size_t)n_sel * n;
    return a > b ? a : b;
}
inline size_t zscan_per_f(int n, int k, int n_sel, bool has_x, bool want_Z) {
    return (size_t)3 * n + (has_x ? n : 0) + (size_t)(n_sel + 2 * k) * n + (size_t)k * k + zscan_stage_rows(n, n_sel, has_x, want_Z);
}

// chunk length for a grid of F points: the forced one, or the automatic one from the scratch budget.  cplx_per_f = complex values of scratch per
// frequency point
inline int zscan_chunk(int F, int chunk, size_t cplx_per_f) {
    if (chunk > 0) return chunk < F ? chunk : F;
    size_t c = ZSCAN_SCRATCH_BYTES / (sizeof(cplx) * (cplx_per_f ? cplx_per_f : 1));
    c = c / 64 * 64;
    if (c < 64) c = 64;
    return c < (size_t)F ? (int)c : F;
}

// ---- per-thread arithmetic ---------------------------------------------------------------------------------------------------------------------
// the tree and the model as the threads see them: device arrays in the kernels, host arrays in the emulation
struct ZscanView {
    int n;
    const int *parent, *pbranch, *child_ptr, *child, *inc_ptr, *inc;
    const double *R, *X, *gsh, *bsh, *xsh;
};

HPF_DIST_HD cplx crecip(cplx a) {
    const double d = a.re * a.re + a.im * a.im;
    return {a.re / d, -a.im / d};
}

HPF_DIST_HD cplx zscan_y(const ZscanView& V, int e, double h) { return crecip({V.R[e], h * V.X[e]}); }

// D_i; yx = y_extra of (f, i) when has_x
HPF_DIST_HD cplx zscan_diag(const ZscanView& V, int i, double h, bool has_x, cplx yx) {
    cplx d = {0.0, 0.0};
    for (int p = V.inc_ptr[i]; p < V.inc_ptr[i + 1]; ++p) d = cadd(d, zscan_y(V, V.inc[p], h));
    d = cadd(d, {V.gsh[i], h * V.bsh[i]});
    if (V.xsh[i] != 0.0 && h != 1.0) d = cadd(d, {0.0, -1.0 / (V.xsh[i] * h)});
    if (has_x) d = cadd(d, yx);
    return d;
}

// upward step of bus i at point f: t [n][Fc] holds the children's t
HPF_DIST_HD void zscan_up(const ZscanView& V, int i, double h, bool has_x, cplx yx, const cplx* t, size_t Fc, size_t f, cplx& w_i, cplx& t_i) {
    cplx S = zscan_diag(V, i, h, has_x, yx);
    for (int p = V.child_ptr[i]; p < V.child_ptr[i + 1]; ++p) {
        const int c = V.child[p];
        S = csub(S, cmul_unf(zscan_y(V, V.pbranch[c], h), t[(size_t)c * Fc + f]));
    }
    w_i = crecip(S);
    t_i = V.parent[i] >= 0 ? cmul_unf(zscan_y(V, V.pbranch[i], h), w_i) : cplx{0.0, 0.0};
}

// downward step: Z_cc from w_c, t_c and the parent's Z_pp
HPF_DIST_HD cplx zscan_down(cplx w_c, cplx t_c, cplx z_p) { return cadd(w_c, cmul_unf(t_c, cmul_unf(t_c, z_p))); }

// column j at point f, the walk up: col[j] and col[a] of every ancestor a
HPF_DIST_HD void zscan_col_walk(const int* parent, int j, const cplx* t, const cplx* Zd, cplx* col, size_t Fc, size_t f) {
    col[(size_t)j * Fc + f] = Zd[(size_t)j * Fc + f];
    cplx prod = t[(size_t)j * Fc + f];
    for (int a = parent[j]; a >= 0; a = parent[a]) {
        col[(size_t)a * Fc + f] = cmul_unf(prod, Zd[(size_t)a * Fc + f]);
        prod = cmul_unf(prod, t[(size_t)a * Fc + f]);
    }
}

// ... and every other bus from its parent
HPF_DIST_HD cplx zscan_col_fill(cplx t_i, cplx col_p) { return cmul_unf(t_i, col_p); }

// tie columns tc: [2 l] = col(a_l), [2 l + 1] = col(b_l), each [n][Fc]
HPF_DIST_HD cplx zscan_tie_u(const cplx* tc, size_t n, size_t Fc, size_t f, int l, int i) {
    return csub(tc[((size_t)(2 * l) * n + i) * Fc + f], tc[((size_t)(2 * l + 1) * n + i) * Fc + f]);
}

HPF_DIST_HD double zscan_abs2(cplx a) { return a.re * a.re + a.im * a.im; }

// W^-1 of point f -> Winv [k k][Fc] (row-major l k + m).  ta / tb / tR / tX [k]: the ties' end buses and series impedance
HPF_DIST_HD void zscan_tie_winv(int k, const int* ta, const int* tb, const double* tR, const double* tX, double h, const cplx* tc, size_t n,
                                size_t Fc, size_t f, cplx* Winv) {
    cplx A[ZSCAN_MAX_TIES][2 * ZSCAN_MAX_TIES], dinv[ZSCAN_MAX_TIES];
    for (int l = 0; l < k; ++l)
        for (int m = 0; m < k; ++m) {
            cplx v = csub(zscan_tie_u(tc, n, Fc, f, m, ta[l]), zscan_tie_u(tc, n, Fc, f, m, tb[l]));
            if (l == m) v = cadd({tR[l], h * tX[l]}, v);
            A[l][m] = v;
            A[l][k + m] = {l == m ? 1.0 : 0.0, 0.0};
        }
    for (int c = 0; c < k; ++c) {
        int piv = c;
        double best = zscan_abs2(A[c][c]);
        for (int r = c + 1; r < k; ++r) {
            const double v = zscan_abs2(A[r][c]);
            if (v > best) {
                best = v;
                piv = r;
            }
        }
        if (piv != c)
            for (int cc = 0; cc < 2 * k; ++cc) {
                const cplx s = A[c][cc];
                A[c][cc] = A[piv][cc];
                A[piv][cc] = s;
            }
        dinv[c] = crecip(A[c][c]);
        for (int r = c + 1; r < k; ++r) {
            const cplx m = cmul_unf(A[r][c], dinv[c]);
            for (int cc = c + 1; cc < 2 * k; ++cc) A[r][cc] = csub(A[r][cc], cmul_unf(m, A[c][cc]));
        }
    }
    for (int j = 0; j < k; ++j)
        for (int r = k - 1; r >= 0; --r) {
            cplx s = A[r][k + j];
            for (int c = r + 1; c < k; ++c) s = csub(s, cmul_unf(A[r][c], A[c][k + j]));
            A[r][k + j] = cmul_unf(s, dinv[r]);
        }
    for (int l = 0; l < k; ++l)
        for (int m = 0; m < k; ++m) Winv[((size_t)l * k + m) * Fc + f] = A[l][k + m];
}

// q(i, j) of point f
HPF_DIST_HD cplx zscan_tie_form(int k, const cplx* tc, const cplx* Winv, size_t n, size_t Fc, size_t f, int i, int j) {
    cplx uj[ZSCAN_MAX_TIES];
    for (int m = 0; m < k; ++m) uj[m] = zscan_tie_u(tc, n, Fc, f, m, j);
    cplx acc = {0.0, 0.0};
    for (int l = 0; l < k; ++l) {
        cplx v = {0.0, 0.0};
        for (int m = 0; m < k; ++m) v = cadd(v, cmul_unf(Winv[((size_t)l * k + m) * Fc + f], uj[m]));
        acc = cadd(acc, cmul_unf(zscan_tie_u(tc, n, Fc, f, l, i), v));
    }
    return acc;
}

HPF_DIST_HD double zscan_abs(cplx z) { return sqrt(z.re * z.re + z.im * z.im); }
HPF_DIST_HD bool zscan_finite(cplx z) { return fabs(z.re) <= 1.79769313486231570815e308 && fabs(z.im) <= 1.79769313486231570815e308; }

// start value of a bus's running peak: loses against every grid point
constexpr int ZSCAN_NO_F = 0x7fffffff;

}  // namespace hpf
