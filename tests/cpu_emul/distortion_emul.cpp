// TEST INFRASTRUCTURE: executes the per-entry functions of csrc/hpf_distortion.hpp (what k_distortion_add runs per thread) serially on the
// host, entry by entry over the list of scenarios like the kernel, so that `-m "not gpu"` tests can check them against the NumPy restatement
// (tests/distortion_ref.py).  It is NOT part of libhpf.so and never on the product path.
#include <vector>

#include "hpf_distortion.hpp"
using namespace hpf;

extern "C" {

// Vm [S][Hn*n] raw signed magnitudes in the ABI's stacked order (k = q*n + i), ids / flags [S]; outputs in the ABI's order (x_* [Hn][n],
// thd_* [n], hist [n][B + 1], counts [3]), accumulated INTO the arrays the caller passes (zeroed, arg = -1, by the caller before the first call).
void emul_distortion(int n, int Hn, int S, const double* Vm, const int* ids, const int* flags, int queue, const double* limit, double thd_limit,
                     double hist_max, int B, long long* counts, double* x_max, int* x_arg, double* x_sum, double* x_sumsq, uint32_t* x_over,
                     double* thd_max, int* thd_arg, double* thd_sum, double* thd_sumsq, uint32_t* thd_over, uint32_t* hist) {
    const size_t E = (size_t)n * Hn;
    const double inv_w = (double)B / hist_max;
    std::vector<double> V(S * E);                      // bus-major like the device state
    std::vector<int> cls(S);
    for (int s = 0; s < S; ++s) {
        for (int q = 0; q < Hn; ++q)
            for (int i = 0; i < n; ++i) V[s * E + (size_t)i * Hn + q] = Vm[s * E + (size_t)q * n + i];
        double best = 0.0;                              // hpf_stat.thd_max as k_stats forms it: NaN if any bus has one, else the maximum
        bool nan = false;
        for (int i = 0; i < n; ++i) {
            const double t = dist_thd(&V[s * E + (size_t)i * Hn], Hn);
            if (t != t) nan = true;
            best = t > best ? t : best;
        }
        cls[s] = dist_classify(flags[s], nan ? NAN : best, queue != 0);
        counts[cls[s]] += 1;
    }
    for (int i = 0; i < n; ++i) {
        for (int q = 0; q < Hn; ++q) {
            const size_t k = (size_t)q * n + i;
            for (int s = 0; s < S; ++s)
                if (cls[s] == DIST_ADD)
                    dist_fold(dist_x(&V[s * E + (size_t)i * Hn], q), ids[s], limit[q], x_max[k], x_arg[k], x_sum[k], x_sumsq[k], x_over[k]);
        }
        for (int s = 0; s < S; ++s) {
            if (cls[s] != DIST_ADD) continue;
            const double t = dist_thd(&V[s * E + (size_t)i * Hn], Hn);
            dist_fold(t, ids[s], thd_limit, thd_max[i], thd_arg[i], thd_sum[i], thd_sumsq[i], thd_over[i]);
            hist[(size_t)i * (B + 1) + dist_bin(t, hist_max, inv_w, B)] += 1u;
        }
    }
}
}
