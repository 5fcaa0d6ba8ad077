// TEST INFRASTRUCTURE: executes the functions of csrc/hpf_waveform.hpp (what k_wave_peaks / k_wave_add run per lane and per thread) serially on the
// host, in the kernels' own order, so that `-m "not gpu"` tests can check them against the NumPy restatement (tests/waveform_ref.py) and the GPU
// tests can compare the device bit for bit.  It is NOT part of libhpf.so and never on the product path.
#include <vector>

#include "hpf_accum.hpp"
#include "hpf_waveform.hpp"
using namespace hpf;

extern "C" {

// (any power of two from 4 on: the header's functions do not need the ABI's 64 <= T <= 4096)
int emul_wave_table(int T, double* ct, double* st) {
    if (T < 4 || (T & (T - 1))) return -1;
    wave_table(T, ct, st);
    return 0;
}

// U [S][n][Hn] bus-major (the device layout), orders [Hn], sel [n_sel]; outputs: v [S][n_sel][T], peak / crest / slack [S][n], kpeak [S][n].
// The kernel's order: 64 lanes, lane l takes k = l, l + 64, ... ascending (strictly-greater-or-smaller-k rule), then the xor butterfly over the
// lanes -- wave_peak_combine is a total order, so any order gives the same pair; the butterfly is kept to show exactly that.
void emul_waveform(int n, int Hn, int S, int T, const int* orders, const cplx* U, const double* ct, const double* st, int n_sel, const int* sel,
                   double* v, double* peak, int* kpeak, double* crest, double* slack) {
    for (int s = 0; s < S; ++s)
        for (int bus = 0; bus < n; ++bus) {
            const cplx* Ub = U + ((size_t)s * n + bus) * Hn;
            uint64_t key[64];
            int kb[64];
            for (int lane = 0; lane < 64; ++lane) {
                key[lane] = 0;
                kb[lane] = lane;
                for (int k = lane; k < T; k += 64) wave_peak_combine(key[lane], kb[lane], wave_key(wave_sample(Ub, orders, Hn, T, ct, st, k)), k);
            }
            for (int off = 32; off > 0; off >>= 1) {
                uint64_t k2[64];
                int b2[64];
                for (int lane = 0; lane < 64; ++lane) k2[lane] = key[lane ^ off], b2[lane] = kb[lane ^ off];
                for (int lane = 0; lane < 64; ++lane) wave_peak_combine(key[lane], kb[lane], k2[lane], b2[lane]);
            }
            const size_t o = (size_t)s * n + bus;
            const double pk = wave_key_value(key[0]);
            peak[o] = pk;
            kpeak[o] = kb[0];
            crest[o] = wave_crest(pk, wave_sumsq(Ub, Hn));
            slack[o] = wave_slack(Ub, orders, Hn, T);
        }
    for (int s = 0; s < S; ++s)
        for (int b = 0; b < n_sel; ++b) {
            const cplx* Ub = U + ((size_t)s * n + sel[b]) * Hn;
            for (int k = 0; k < T; ++k) v[((size_t)s * n_sel + b) * T + k] = wave_sample(Ub, orders, Hn, T, ct, st, k);
        }
}

double emul_wave_rms(int Hn, const cplx* U_bus) { return wave_rms(U_bus, Hn); }

// the accumulator over a list as on the device (hpf_accum.hpp: L entries, slots / gids [L] or NULL, ids id_base + number; flags, thd_max [nrec]:
// the records by scenario number; peak, crest [storages][n]), bus by bus like k_wave_add; arrays accumulated INTO what the caller passes (zeroed,
// arg = -1, before the first call): f [6][n] (peak max | sum | sumsq, crest ...), arg, over [2][n]
void emul_wave_add(int n, int L, const int* slots, const int* gids, int id_base, int nrec, const double* peak, const double* crest, const int* flags,
                   const double* thd_max, int queue, const double* peak_limit, double crest_limit, long long* counts, double* f, int* arg,
                   uint32_t* over) {
    std::vector<hpf_stat> stats((size_t)nrec);
    for (int g = 0; g < nrec; ++g) stats[g].flags = flags[g], stats[g].thd_max = thd_max[g];
    const AccumList list{L, slots, gids, id_base, queue, stats.data()};
    accum_count(list, counts);
    for (int i = 0; i < n; ++i) {
        AccumSlot st[2];
        for (int k = 0; k < 2; ++k) st[k].load(f, arg, over, k, (size_t)n, (size_t)i);
        const bool any = accum_walk(list, [&](int s, int id) {
            const size_t o = (size_t)s * n + i;
            st[0].fold(peak[o], id, peak_limit[i]);
            st[1].fold(crest[o], id, crest_limit);
        });
        if (!any) continue;
        for (int k = 0; k < 2; ++k) st[k].store(f, arg, over, k, (size_t)n, (size_t)i);
    }
}
}
