// Resonance mode analysis (hpf_resonance_modes): per point of a grid of F real harmonic orders, the eigenvalue of Y(h) of smallest modulus (the
// critical mode), its modal impedance 1 / |lambda| and the participation factors of the buses -- which resonance a peak of the impedance scan is,
// and which buses take part in it.  The network, y_e(h), D_i, the BFS tree, w_i, t_i, the tie columns u_l and W^-1 are exactly those of
// hpf_zscan.hpp (the factor, formed once per frequency point by the scan's kernels); y = Y^-1 x is the right-hand-side path of hpf_penetration.hpp
// with one scenario (sc = 1, J = Fc).  This header adds the inverse iteration around it.  The k_rma_* kernels of hpf_zscan.hip run these functions
// on the device; the host emulation (tests/cpu_emul/rma_emul.cpp) runs the same functions serially.  Every product, sum and quotient is rounded on
// its own (-ffp-contract=off; cmul_unf, cadd, csub of hpf_assembly.hpp, crecip and zscan_abs of hpf_zscan.hpp), every sum has the one order
// written here, every maximum is taken in a total order, nothing is atomic: device == emulation bit for bit, for every chunk length.
//
// Per frequency point, Y = Y(h) complex symmetric, x and y [n]:
//   start:      x_i = 1.0 + (double)i / (double)n          (not symmetric: an odd mode of a symmetric feeder is not orthogonal to it)
//   for k = 1 .. iters:
//               y = Y^-1 x                                  pen_up / pen_down / pen_tie_coef / pen_tie_fix
//               p = argmax_i zscan_abs(y_i)                 wave_key / wave_peak_combine: a NaN is the maximum, ties to the smallest bus; the order
//                                                           of the search is free (partial maxima per tile of RMA_TILE buses, then over the tiles)
//               if k < iters:  x_i = cmul_unf(y_i, crecip(y_p))
//   sums:       a = sum_i x_i y_i,  b = sum_i x_i x_i,  g = sum_i y_i y_i      of the last x and y, bilinear (no conjugate); each in tiles of
//                                                           RMA_TILE consecutive buses, ascending inside a tile from (0, 0), then the tile sums
//                                                           in ascending tile order from (0, 0): the order depends on n alone
//   eigenpair:  mu = cmul_unf(a, crecip(b)),  lambda = crecip(mu),  zm = zscan_abs(mu)
//   pf_i      = cmul_unf(cmul_unf(y_i, y_i), crecip(g))     sum_i pf_i = 1; L_i T_i of the mode for a symmetric Y
//   top       = p of the last iteration
//   res       = max_i zscan_abs(csub(x_i, cmul_unf(lambda, y_i))) / (zscan_abs(lambda) zscan_abs(y_p))      the maximum in the order of wave_key
//               = || Y y - lambda y ||_inf / (|lambda| || y ||_inf), because Y y = x.  Large where two modes cross or iters is too small:
//               nothing is retried or adapted.
#pragma once
#include "hpf_penetration.hpp"

namespace hpf {

constexpr int RMA_TILE = 32, RMA_MAX_ITERS = 256;
// start value of a running maximum's bus: loses against every bus
constexpr int RMA_NO_BUS = 0x7fffffff;

HPF_DIST_HD int rma_tiles(int n) { return (n + RMA_TILE - 1) / RMA_TILE; }

// complex values of scratch per frequency point: w, t | Z (the column walks read it) | y_extra | the tie columns | W^-1 and the tie coefficients |
// x, y | pf | the staging buffer of y_extra and pf | per tile: a partial key with its bus (one value) and three partial sums | per point: the three
// sums, y_p, lambda, 1 / g, (zm, res) and the pivot (eight values)
inline size_t rma_per_f(int n, int k, bool has_x, bool want_pf) {
    return (size_t)2 * n + (k ? n : 0) + (has_x ? n : 0) + (size_t)2 * k * n + (size_t)k * k + k + (size_t)2 * n + (want_pf ? n : 0) +
           (has_x || want_pf ? n : 0) + (size_t)4 * rma_tiles(n) + 8;
}

HPF_DIST_HD cplx rma_start(int i, int n) { return {1.0 + (double)i / (double)n, 0.0}; }

// the largest zscan_abs(v_i) of the buses of tile T at point f, and its bus; v [n][Fc]
HPF_DIST_HD void rma_tile_peak(const cplx* v, int n, size_t Fc, size_t f, int T, uint64_t& key, int& arg) {
    key = 0;
    arg = RMA_NO_BUS;
    const int i1 = (T + 1) * RMA_TILE < n ? (T + 1) * RMA_TILE : n;
    for (int i = T * RMA_TILE; i < i1; ++i) wave_peak_combine(key, arg, wave_key(zscan_abs(v[(size_t)i * Fc + f])), i);
}

// ... and over the tiles: pkey, parg [tiles][Fc]
HPF_DIST_HD void rma_peak_fold(const uint64_t* pkey, const int* parg, int tiles, size_t Fc, size_t f, uint64_t& key, int& arg) {
    key = 0;
    arg = RMA_NO_BUS;
    for (int T = 0; T < tiles; ++T) wave_peak_combine(key, arg, pkey[(size_t)T * Fc + f], parg[(size_t)T * Fc + f]);
}

HPF_DIST_HD cplx rma_scale(cplx y_i, cplx y_p) { return cmul_unf(y_i, crecip(y_p)); }

// the three sums of tile T at point f
HPF_DIST_HD void rma_tile_sums(const cplx* x, const cplx* y, int n, size_t Fc, size_t f, int T, cplx& a, cplx& b, cplx& g) {
    a = b = g = {0.0, 0.0};
    const int i1 = (T + 1) * RMA_TILE < n ? (T + 1) * RMA_TILE : n;
    for (int i = T * RMA_TILE; i < i1; ++i) {
        const cplx xi = x[(size_t)i * Fc + f], yi = y[(size_t)i * Fc + f];
        a = cadd(a, cmul_unf(xi, yi));
        b = cadd(b, cmul_unf(xi, xi));
        g = cadd(g, cmul_unf(yi, yi));
    }
}

// ... and one of them over the tiles: part [tiles][Fc]
HPF_DIST_HD cplx rma_sum_fold(const cplx* part, int tiles, size_t Fc, size_t f) {
    cplx s = {0.0, 0.0};
    for (int T = 0; T < tiles; ++T) s = cadd(s, part[(size_t)T * Fc + f]);
    return s;
}

// the eigenpair of a point from its sums: lambda, zm = |mu|, ginv = 1 / g
HPF_DIST_HD void rma_eig(cplx a, cplx b, cplx g, cplx& lam, double& zm, cplx& ginv) {
    const cplx mu = cmul_unf(a, crecip(b));
    lam = crecip(mu);
    zm = zscan_abs(mu);
    ginv = crecip(g);
}

HPF_DIST_HD cplx rma_pf(cplx y_i, cplx ginv) { return cmul_unf(cmul_unf(y_i, y_i), ginv); }

// one bus's term of the residual's maximum
HPF_DIST_HD double rma_defect(cplx x_i, cplx lam, cplx y_i) { return zscan_abs(csub(x_i, cmul_unf(lam, y_i))); }

// the residual from the key of the largest defect
HPF_DIST_HD double rma_res(uint64_t dkey, cplx lam, cplx y_p) { return wave_key_value(dkey) / (zscan_abs(lam) * zscan_abs(y_p)); }

HPF_DIST_HD bool rma_finite(double v) { return fabs(v) <= 1.79769313486231570815e308; }

}  // namespace hpf
