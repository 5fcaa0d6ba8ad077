// Host emulation of hpf_resonance_modes: the functions of csrc/hpf_resonance.hpp run serially in the kernels' order (hpf_zscan.hip) -- per chunk
// of frequency points the factor (zfactor_emul.hpp), the start vector, `iters` times the solve with one scenario (zfactor_emul.hpp), the pivot per
// tile and over the tiles and the scaling, then the tile sums and their fold, the eigenpair, the participation factors and the residual; arrays
// [bus][fc] and [tile][fc] like the device's.  Test infrastructure only.
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "hpf_resonance.hpp"
#include "zfactor_emul.hpp"

using namespace hpf;

extern "C" int emul_resonance_modes(int n, int nb, const int32_t* from, const int32_t* to, const double* R, const double* X, const double* gsh,
                                    const double* bsh, const double* xsh, int F, const double* h, const cplx* y_extra, int iters, int chunk,
                                    cplx* lam, double* zm, double* res, int32_t* top, cplx* pf) {
    if (iters < 1 || iters > RMA_MAX_ITERS) return HPF_E_ARG;
    EmulFactor E;
    const int rc = E.plan(n, nb, from, to, R, X, gsh, bsh, xsh);
    if (rc != HPF_OK) return rc;
    const int k = E.T.k, tiles = rma_tiles(n);
    const int Fc = zscan_chunk(F, chunk, rma_per_f(n, k, y_extra != nullptr, pf != nullptr));
    E.size(Fc, false);
    std::vector<cplx> x((size_t)n * Fc), y((size_t)n * Fc), coef((size_t)k * Fc), part((size_t)3 * tiles * Fc), sums((size_t)3 * Fc), yp(Fc);
    std::vector<uint64_t> pkey((size_t)tiles * Fc);
    std::vector<int> parg((size_t)tiles * Fc), piv(Fc);
    bool bad = false;
    for (int f0 = 0; f0 < F; f0 += Fc) {
        const int fc = std::min(Fc, F - f0);
        const size_t C = (size_t)fc, q = (size_t)tiles * C;
        emul_factor(E, h, y_extra, f0, fc);
        for (int i = 0; i < n; ++i)
            for (int f = 0; f < fc; ++f) x[i * C + f] = y[i * C + f] = rma_start(i, n);
        for (int it = 1; it <= iters; ++it) {
            emul_solve(E, fc, 1, y.data(), coef.data());
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
