// Host emulation of hpf_impedance_scan: the functions of csrc/hpf_zscan.hpp run serially in the kernels' order (hpf_zscan.hip) -- per chunk of
// frequency points the factor (zfactor_emul.hpp: the two walks, the column walks and fills, W^-1), the tie correction, the peak fold; arrays
// [bus][fc] like the device's.  Test infrastructure only.
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "zfactor_emul.hpp"

using namespace hpf;

extern "C" int emul_zscan(int n, int nb, const int32_t* from, const int32_t* to, const double* R, const double* X, const double* gsh,
                          const double* bsh, const double* xsh, int F, const double* h, const cplx* y_extra, int n_sel, const int32_t* sel,
                          int chunk, cplx* Z, cplx* Zt, double* zpeak, int32_t* fpeak) {
    EmulFactor E;
    const int r = E.plan(n, nb, from, to, R, X, gsh, bsh, xsh, n_sel, sel);
    if (r != HPF_OK) return r;
    const int k = E.T.k;
    const int Fc = zscan_chunk(F, chunk, zscan_per_f(n, k, n_sel, y_extra != nullptr, Z != nullptr));
    E.size(Fc, true);
    std::vector<cplx>& Zd = E.Zd;
    std::vector<cplx>& cols = E.cols;
    std::vector<uint64_t> pkey(n, 0);
    std::vector<int> pf(n, ZSCAN_NO_F), bad(n, 0);
    for (int f0 = 0; f0 < F; f0 += Fc) {
        const int fc = std::min(Fc, F - f0);
        const size_t S = (size_t)fc;
        emul_factor(E, h, y_extra, f0, fc);
        if (k) {
            const cplx* tc = E.tie_cols(S);
            for (int i = 0; i < n; ++i)
                for (int f = 0; f < fc; ++f) Zd[i * S + f] = csub(Zd[i * S + f], zscan_tie_form(k, tc, E.Winv.data(), (size_t)n, S, (size_t)f, i, i));
            for (int s = 0; s < n_sel; ++s)
                for (int i = 0; i < n; ++i)
                    for (int f = 0; f < fc; ++f) {
                        cplx& z = cols[((size_t)s * n + i) * S + f];
                        z = csub(z, zscan_tie_form(k, tc, E.Winv.data(), (size_t)n, S, (size_t)f, i, E.T.colbus[s]));
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

// the scratch-size formula and the chunk length the call would use
extern "C" long long emul_zscan_per_f(int n, int k, int n_sel, int has_x, int want_Z) { return (long long)zscan_per_f(n, k, n_sel, has_x, want_Z); }
extern "C" int emul_zscan_chunk(int F, int chunk, long long per_f) { return zscan_chunk(F, chunk, (size_t)per_f); }

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
