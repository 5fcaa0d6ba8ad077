// Sweep accumulators (hpf_distortion_*, hpf_branch_stats_*, hpf_waveform_stats_*): what the three have in common -- the scenario list, the
// walk of the counters thread, the walk of an owner thread, and the five statistics of one quantity of one owner.  k_distortion_add,
// k_branch_add, k_wave_add and k_wave_peaks (hpf_lib.hip) run these functions per thread; the host emulations (tests/cpu_emul/*.cpp) run the
// same functions serially.  No HIP calls, no atomics: one thread owns one entry of the statistics and walks the list in order, so max / arg /
// over / the counters do not depend on the order in which scenarios arrive and only the sums do, by rounding alone.
#pragma once
#include <stddef.h>

#include "../../include/hpf.h"
#include "hpf_distortion.hpp"

namespace hpf {

// one list entry, decoded: slot < 0 ends the list (number and cls are then not set)
struct AccumEntry {
    int slot, number, cls;
};

// The finished scenarios a launch looks at.  Entry l: storage slots[l] (NULL: l; a negative slot ends the list -- the lists of hpf_solve_queue
// are -1 from their end on), scenario number gids[l] (NULL: l) -> record stats[number], id id_base + number.  queue: the caller is
// hpf_solve_queue, so a scenario it only reports is deferred (dist_classify); a warm-started or rectangular-update scenario that did not
// converge is deferred for every caller (dist_classify_start).  stats NULL (k_wave_peaks outside an accumulator): every entry is DIST_ADD.
struct AccumList {
    int L;
    const int* slots;
    const int* gids;
    int id_base;
    int queue;
    const hpf_stat* stats;

    HPF_DIST_HD AccumEntry entry(int l) const {
        AccumEntry e = {slots ? slots[l] : l, 0, DIST_ADD};
        if (e.slot < 0) return e;
        e.number = gids ? gids[l] : l;
        if (stats) {
            const hpf_stat st = stats[e.number];
            e.cls = dist_classify_start(st.flags, st.thd_max, queue != 0);
        }
        return e;
    }
};

// the counters thread: cnt[k] += entries of class k (added, skipped, deferred)
HPF_DIST_HD void accum_count(const AccumList& list, long long* cnt) {
    long long c[3] = {0, 0, 0};
    for (int l = 0; l < list.L; ++l) {
        const AccumEntry e = list.entry(l);
        if (e.slot < 0) break;
        c[e.cls] += 1;
    }
    for (int k = 0; k < 3; ++k) cnt[k] = cnt[k] + c[k];
}

// an owner thread: fold(slot, id) for every DIST_ADD entry, in list order -> whether there was one (if not, the owner stores nothing)
template <class Fold>
HPF_DIST_HD bool accum_walk(const AccumList& list, Fold&& fold) {
    bool any = false;
    for (int l = 0; l < list.L; ++l) {
        const AccumEntry e = list.entry(l);
        if (e.slot < 0) break;
        if (e.cls != DIST_ADD) continue;
        fold(e.slot, list.id_base + e.number);
        any = true;
    }
    return any;
}

// The statistics of quantity k of owner t, of `count` owners: f[3k + a][count] holds max | sum | sum of squares (a = 0, 1, 2), arg[k][count] the
// id of the maximum (-1: nothing added), over[k][count] the samples above the limit (NULL: a quantity without a limit).
struct AccumSlot {
    double max, sum, sumsq;
    int arg;
    uint32_t over;

    HPF_DIST_HD void load(const double* f, const int* a, const uint32_t* o, int k, size_t count, size_t t) {
        max = f[(size_t)(3 * k) * count + t];
        sum = f[(size_t)(3 * k + 1) * count + t];
        sumsq = f[(size_t)(3 * k + 2) * count + t];
        arg = a[(size_t)k * count + t];
        over = o ? o[(size_t)k * count + t] : 0u;
    }
    HPF_DIST_HD void store(double* f, int* a, uint32_t* o, int k, size_t count, size_t t) const {
        f[(size_t)(3 * k) * count + t] = max;
        f[(size_t)(3 * k + 1) * count + t] = sum;
        f[(size_t)(3 * k + 2) * count + t] = sumsq;
        a[(size_t)k * count + t] = arg;
        if (o) o[(size_t)k * count + t] = over;
    }
    // one sample x of scenario `id` (dist_fold; a quantity without a limit goes through branch_stat_fold on max, arg, sum, sumsq)
    HPF_DIST_HD void fold(double x, int id, double limit) { dist_fold(x, id, limit, max, arg, sum, sumsq, over); }
};

}  // namespace hpf
