// TEST INFRASTRUCTURE: executes the per-entry functions of csrc/hpf_distortion.hpp (what k_distortion_add runs per thread) serially on the
// host, entry by entry over the list of scenarios like the kernel, so that `-m "not gpu"` tests can check them against the NumPy restatement
// (tests/distortion_ref.py).  It is NOT part of libhpf.so and never on the product path.
#include <vector>

#include "hpf_accum.hpp"
using namespace hpf;

extern "C" {

// The list as on the device (hpf_accum.hpp): L entries, slots / gids [L] or NULL, ids id_base + number.  Vm [storages][Hn*n] raw signed magnitudes
// in the ABI's stacked order (k = q*n + i), flags [nrec] by scenario number (the records' thd_max is formed here, as k_stats does); outputs in the
// ABI's order (x_* [Hn][n], thd_* [n], hist [n][B + 1], counts [3]), accumulated INTO the arrays the caller passes (zeroed, arg = -1, by the caller
// before the first call).
void emul_distortion(int n, int Hn, int L, const int* slots, const int* gids, int id_base, int nrec, const double* Vm, const int* flags, int queue,
                     const double* limit, double thd_limit, double hist_max, int B, long long* counts, double* x_max, int* x_arg, double* x_sum,
                     double* x_sumsq, uint32_t* x_over, double* thd_max, int* thd_arg, double* thd_sum, double* thd_sumsq, uint32_t* thd_over,
                     uint32_t* hist) {
    const size_t E = (size_t)n * Hn;
    const double inv_w = (double)B / hist_max;
    std::vector<hpf_stat> stats((size_t)nrec);
    for (int g = 0; g < nrec; ++g) stats[g].flags = flags[g], stats[g].thd_max = 0.0;
    const AccumList bare{L, slots, gids, id_base, queue, nullptr}, list{L, slots, gids, id_base, queue, stats.data()};
    auto bus_major = [&](int s, int i, std::vector<double>& V) {       // the device's layout of one bus
        V.resize((size_t)Hn);
        for (int q = 0; q < Hn; ++q) V[q] = Vm[(size_t)s * E + (size_t)q * n + i];
    };
    std::vector<double> V;
    for (int l = 0; l < L; ++l) {
        const AccumEntry e = bare.entry(l);
        if (e.slot < 0) break;
        double best = 0.0;                              // hpf_stat.thd_max as k_stats forms it: NaN if any bus has one, else the maximum
        bool nan = false;
        for (int i = 0; i < n; ++i) {
            bus_major(e.slot, i, V);
            const double t = dist_thd(V.data(), Hn);
            if (t != t) nan = true;
            best = t > best ? t : best;
        }
        stats[e.number].thd_max = nan ? NAN : best;
    }
    accum_count(list, counts);
    for (int i = 0; i < n; ++i) {
        for (int q = 0; q < Hn; ++q) {
            const size_t k = (size_t)q * n + i;
            accum_walk(list, [&](int s, int id) {
                bus_major(s, i, V);
                dist_fold(dist_x(V.data(), q), id, limit[q], x_max[k], x_arg[k], x_sum[k], x_sumsq[k], x_over[k]);
            });
        }
        accum_walk(list, [&](int s, int id) {
            bus_major(s, i, V);
            const double t = dist_thd(V.data(), Hn);
            dist_fold(t, id, thd_limit, thd_max[i], thd_arg[i], thd_sum[i], thd_sumsq[i], thd_over[i]);
            hist[(size_t)i * (B + 1) + dist_bin(t, hist_max, inv_w, B)] += 1u;
        });
    }
}
}
