// Distortion accumulator (hpf_distortion_*): the per-entry arithmetic that folds one finished scenario into the running per-bus /
// per-harmonic statistics of a sweep.  k_distortion_add (hpf_lib.hip) runs these functions one thread per entry; the host emulation
// (tests/cpu_emul/distortion_emul.cpp) runs the same functions serially.  No floating-point atomics anywhere: one thread owns one entry
// and walks the scenarios in list order, so max / arg / the integer counters do not depend on that order and only the sums do, by
// rounding alone.  Compiled with -ffp-contract=off like the rest of the library (the THD sum is the one of k_stats, bit for bit).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define HPF_DIST_HD __host__ __device__ __forceinline__
#else
#define HPF_DIST_HD inline
#endif

namespace hpf {

enum { DIST_ADD = 0, DIST_SKIP = 1, DIST_DEFER = 2 };

// What happens to a scenario with result record (flags, thd_max): hpf_solve_queue only reports a scenario with flags bit 2, 3 or 6 (it is
// solved again through hpf_solve, which adds it) -> deferred; a scenario that did not converge (bit 0 clear) or has a non-finite THD at
// some bus (thd_max, the maximum over the buses, is then not finite either: k_stats) is skipped.
HPF_DIST_HD int dist_classify(int flags, double thd_max, bool queue) {
    if (queue && (flags & (4 | 8 | 64))) return DIST_DEFER;
    if (!(flags & 1) || !(fabs(thd_max) <= 1.79769313486231570815e308)) return DIST_SKIP;
    return DIST_ADD;
}

// ... and with a start state (hpf_start_*): a scenario that was started from the handle's start state (flags bit 8) and did not converge is
// solved again by the caller from the reference's start, which adds it -> deferred, not skipped (whoever looks: the queue or an explicit add);
// every other record is classified as above.
// The same holds for a scenario whose harmonic steps were applied in rectangular form (option "rectangular_update", flags bit 9) and that did
// not converge: the caller solves it again with the reference's update.
HPF_DIST_HD int dist_classify_start(int flags, double thd_max, bool queue) {
    if ((flags & (256 | 512)) && !(flags & 1)) return DIST_DEFER;
    return dist_classify(flags, thd_max, queue);
}

// x of entry (bus, q) from the bus's Hn raw signed magnitudes: |V_1| for q = 0, the individual harmonic distortion |V_h| / |V_1| above
HPF_DIST_HD double dist_x(const double* Vbus, int q) {
    const double v0 = fabs(Vbus[0]);
    return q == 0 ? v0 : fabs(Vbus[q]) / v0;
}

// THD_F of a bus: the arithmetic of k_stats / api.get_THD (sequential sum over ascending q, one sqrt, one division)
HPF_DIST_HD double dist_thd(const double* Vbus, int Hn) {
    double hs = 0.0;
    for (int q = 1; q < Hn; ++q) hs = hs + Vbus[q] * Vbus[q];
    return sqrt(hs) / fabs(Vbus[0]);
}

// one sample x of scenario `id` into the five statistics of an entry (arg < 0: nothing added yet; ties of the maximum: the smallest id)
HPF_DIST_HD void dist_fold(double x, int id, double limit, double& mx, int& arg, double& sum, double& sumsq, uint32_t& over) {
    if (arg < 0 || x > mx || (x == mx && id < arg)) {
        mx = x;
        arg = id;
    }
    sum = sum + x;
    sumsq = sumsq + x * x;
    if (x > limit) over = over + 1u;
}

// histogram bin of a THD sample: B uniform bins on [0, hist_max), bin B = overflow; inv_w = B / hist_max formed once on the host
HPF_DIST_HD int dist_bin(double thd, double hist_max, double inv_w, int B) {
    if (thd >= hist_max) return B;
    const int b = (int)(thd * inv_w);
    return b > B ? B : b;                  // (thd * inv_w can round up to B just below hist_max: that is bin B by the rule itself)
}

}  // namespace hpf
