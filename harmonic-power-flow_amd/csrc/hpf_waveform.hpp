// Bus voltage waveforms (hpf_waveform, hpf_waveform_stats_*): the per-sample arithmetic of v(t) at one bus over one fundamental period, its peak,
// RMS, crest factor and the bound of the sampling error.  k_wave_peaks / k_wave_add (hpf_lib.hip) run these functions on the device; the host
// emulation (tests/cpu_emul/waveform_emul.cpp) runs the same functions serially.  Every product, difference and sum is rounded on its own
// (-ffp-contract=off), every sum over the harmonics runs over ascending q in one thread, and nothing here is atomic.
//   T samples per fundamental period (a power of two, 64 .. 4096);  table ct[j] = cos(2 pi j / T), st[j] = sin(2 pi j / T), j < T (host libm)
//   sample k:  j = (orders[q] k) mod T  (integer phase: no argument reduction),  v[k] = sum_q (U[q].re ct[j] - U[q].im st[j])
//   peak = max_k |v[k]| at kpeak = the smallest such k;  rms = sqrt(0.5 sum_q |U[q]|^2);  crest = peak / rms  (sqrt 2 for a pure sine)
//   slack = 0.5 (pi / T)^2 sum_q orders[q]^2 |U[q]|:  the continuous peak lies in [peak, peak + slack]  (v' = 0 at it, |v''| <= sum h^2 |U|)
// Per unit of the nominal peak voltage: |U[0]| is the amplitude of the fundamental.
#pragma once
#include <math.h>
#include <stdint.h>

#include "hpf_assembly.hpp"
#include "hpf_distortion.hpp"

namespace hpf {

constexpr int WAVE_T_MIN = 64, WAVE_T_MAX = 4096, WAVE_ORDER_MAX = 32767;

inline bool wave_T_ok(int T) { return T >= WAVE_T_MIN && T <= WAVE_T_MAX && (T & (T - 1)) == 0; }
inline bool wave_order_ok(int h) { return h >= 1 && h <= WAVE_ORDER_MAX; }

// the twiddle table (host): libm's cos / sin of (double)j * (2 pi / T), the quadrant points exact
inline void wave_table(int T, double* ct, double* st) {
    const double w = 6.283185307179586 / (double)T;
    // (two loops: side by side a compiler may merge the pair into one sincos call, whose values differ from cos / sin in the last bit at a few j)
    for (int j = 0; j < T; ++j) ct[j] = cos((double)j * w);
    for (int j = 0; j < T; ++j) st[j] = sin((double)j * w);
    ct[0] = 1.0, st[0] = 0.0;
    ct[T / 4] = 0.0, st[T / 4] = 1.0;
    ct[T / 2] = -1.0, st[T / 2] = 0.0;
    ct[3 * T / 4] = 0.0, st[3 * T / 4] = -1.0;
}

// table position of harmonic order h at sample k (h <= 32767, k < 4096: the product stays below 2^27)
HPF_DIST_HD int wave_phase(int h, int k, int T) { return (h * k) & (T - 1); }

// one term of a sample, and the sample: sequential over ascending q from 0.0
HPF_DIST_HD double wave_term(cplx u, double c, double s) { return u.re * c - u.im * s; }

HPF_DIST_HD double wave_sample(const cplx* U_bus, const int* orders, int Hn, int T, const double* ct, const double* st, int k) {
    double v = 0.0;
    for (int q = 0; q < Hn; ++q) {
        const int j = wave_phase(orders[q], k, T);
        v = v + wave_term(U_bus[q], ct[j], st[j]);
    }
    return v;
}

// |v| as a key whose unsigned order is the order of the maximum: the IEEE bit pattern of a non-negative double is monotone, +inf sits above
// every finite value and every NaN (one pattern for all of them) above +inf -- a NaN sample is the peak, as in numpy's max / argmax
HPF_DIST_HD uint64_t wave_key(double v) {
    if (v != v) return 0x7ff8000000000000ull;
    union {
        double d;
        uint64_t u;
    } b;
    b.d = fabs(v);
    return b.u;
}

HPF_DIST_HD double wave_key_value(uint64_t key) {
    union {
        double d;
        uint64_t u;
    } b;
    b.u = key;
    return b.d;
}

// the running maximum (key, k) takes the candidate (key2, k2): the larger key, ties to the smaller k -- a total order, so the result does not
// depend on the order in which samples are combined (inside a lane, across the lanes of a wave, serially on the host)
HPF_DIST_HD void wave_peak_combine(uint64_t& key, int& k, uint64_t key2, int k2) {
    if (key2 > key || (key2 == key && k2 < k)) {
        key = key2;
        k = k2;
    }
}

// s = sum_q (re^2 + im^2) sequential over ascending q from 0.0;  rms = sqrt(0.5 s)
HPF_DIST_HD double wave_sumsq(const cplx* U_bus, int Hn) {
    double s = 0.0;
    for (int q = 0; q < Hn; ++q) s = s + (U_bus[q].re * U_bus[q].re + U_bus[q].im * U_bus[q].im);
    return s;
}

HPF_DIST_HD double wave_rms(const cplx* U_bus, int Hn) { return sqrt(0.5 * wave_sumsq(U_bus, Hn)); }

// crest = peak / rms, formed as sqrt(2) (peak / sqrt(s)): a pure sine of ANY amplitude a then gives sqrt 2 to the last bit (sqrt(a a) = a, a / a = 1),
// where peak / sqrt(0.5 s) misses it by an ulp for a = 1, 0.5, 2, 1.03, ...  NaN or inf where s = 0.
HPF_DIST_HD double wave_crest(double peak, double s) { return 1.4142135623730951 * (peak / sqrt(s)); }

// slack = (0.5 w^2) sum_q h^2 |U[q]|, w = pi / T; the sum sequential over ascending q from 0.0, |U| = sqrt(re^2 + im^2)
HPF_DIST_HD double wave_slack(const cplx* U_bus, const int* orders, int Hn, int T) {
    const double w = 3.141592653589793 / (double)T;
    double s = 0.0;
    for (int q = 0; q < Hn; ++q) {
        const double h = (double)orders[q];
        s = s + (h * h) * sqrt(U_bus[q].re * U_bus[q].re + U_bus[q].im * U_bus[q].im);
    }
    return (0.5 * (w * w)) * s;
}

}  // namespace hpf
