// TEST INFRASTRUCTURE: the shared part of the sweep accumulators (csrc/hpf_accum.hpp: list entry, counters walk, owner walk, statistic slot) on
// the host under ASan + UBSan (tests/test_accum_host.py).  Every buffer is a heap block of exactly the size the layout asks for, so an index
// one past [3k + a][count], a read of slots / gids / records behind the terminator's position or past L is a sanitizer report; the values are
// checked against a restatement written out plainly below.  Samples are multiples of 1/4, so every sum is exact.  Prints "accum clean" when
// every check holds.
#include <math.h>
#include <stdio.h>

#include <vector>

#include "hpf_accum.hpp"
using namespace hpf;

static int fails = 0;
static const char* what = "";
#define CHECK(c)                                                                       \
    do {                                                                               \
        if (!(c) && ++fails <= 20) printf("FAIL %s:%d  %s  (%s)\n", __FILE__, __LINE__, #c, what); \
    } while (0)

static double sample(int slot, int k, int t) { return 0.25 * ((slot * 7 + k * 3 + t * 5) % 11); }

// the classification restated (hpf_distortion.hpp): 0 added, 1 skipped, 2 deferred
static int cls_of(const hpf_stat& st, bool queue) {
    if ((st.flags & (256 | 512)) && !(st.flags & 1)) return 2;
    if (queue && (st.flags & (4 | 8 | 64))) return 2;
    if (!(st.flags & 1) || !isfinite(st.thd_max)) return 1;
    return 0;
}

struct Arrays {
    std::vector<double> f;
    std::vector<int> arg;
    std::vector<uint32_t> over;
    std::vector<long long> cnt;
    Arrays(int nq, int nover, int count) : f((size_t)3 * nq * count, 0.0), arg((size_t)nq * count, -1), over((size_t)nover * count, 0u), cnt(3, 0) {}
    bool operator==(const Arrays& o) const { return f == o.f && arg == o.arg && over == o.over && cnt == o.cnt; }
};

// nq quantities of `count` owners, the first nover of them with an over row and limit 1.0; slots / gids: empty = NULL
static void run(const char* name, const std::vector<int>& slots, const std::vector<int>& gids, int L, int id_base, bool queue,
                const std::vector<hpf_stat>& stats, int nq, int nover, int count) {
    what = name;
    const AccumList list{L, slots.empty() ? nullptr : slots.data(), gids.empty() ? nullptr : gids.data(), id_base, queue ? 1 : 0, stats.data()};
    Arrays got(nq, nover, count), want(nq, nover, count);
    for (int pass = 0; pass < 2; ++pass) {                // (twice: the second pass loads what the first stored)
        accum_count(list, got.cnt.data());
        for (int t = 0; t < count; ++t) {
            std::vector<AccumSlot> st((size_t)nq);
            for (int k = 0; k < nq; ++k) st[k].load(got.f.data(), got.arg.data(), k < nover ? got.over.data() : nullptr, k, (size_t)count, (size_t)t);
            const bool any = accum_walk(list, [&](int s, int id) {
                for (int k = 0; k < nq; ++k) st[k].fold(sample(s, k, t), id, k < nover ? 1.0 : (double)INFINITY);
            });
            if (!any) continue;
            for (int k = 0; k < nq; ++k) st[k].store(got.f.data(), got.arg.data(), k < nover ? got.over.data() : nullptr, k, (size_t)count, (size_t)t);
        }
        for (int l = 0; l < L; ++l) {
            const int s = slots.empty() ? l : slots[l];
            if (s < 0) break;
            const int g = gids.empty() ? l : gids[l], c = cls_of(stats[g], queue);
            want.cnt[c] += 1;
            if (c != 0) continue;
            for (int k = 0; k < nq; ++k)
                for (int t = 0; t < count; ++t) {
                    const double x = sample(s, k, t);
                    double &mx = want.f[(size_t)(3 * k) * count + t], &sum = want.f[(size_t)(3 * k + 1) * count + t],
                           &sumsq = want.f[(size_t)(3 * k + 2) * count + t];
                    int& arg = want.arg[(size_t)k * count + t];
                    if (arg < 0 || x > mx || (x == mx && id_base + g < arg)) mx = x, arg = id_base + g;
                    sum += x;
                    sumsq += x * x;
                    if (k < nover && x > 1.0) want.over[(size_t)k * count + t] += 1u;
                }
        }
        CHECK(got == want);
    }
    for (int l = 0; l < L; ++l) {                          // the entry decoding k_wave_peaks uses, with and without records
        AccumList bare = list;
        bare.stats = nullptr;
        const AccumEntry e = list.entry(l), b = bare.entry(l);
        const int s = slots.empty() ? l : slots[l];
        CHECK(e.slot == s && b.slot == s);
        if (s < 0) break;                                  // (the queue's lists are -1 from there on; nothing behind it is decodable here)
        const int g = gids.empty() ? l : gids[l];
        CHECK(e.number == g && b.number == g && e.cls == cls_of(stats[g], queue) && b.cls == DIST_ADD);
    }
}

int main() {
    const hpf_stat ok = {3, 1, 1e-9, 0.05}, skip = {9, 2, 1.0, 0.05}, nan = {3, 1, 1e-9, NAN}, warm = {9, 256 | 2, 1.0, 0.05}, rect = {9, 512 | 2, 1.0, 0.05},
                   rep = {3, 1 | 8, 1e-9, 0.05};
    const std::vector<int> none;
    for (int queue = 0; queue < 2; ++queue)
        for (int nover = 0; nover <= 2; ++nover) {
            const int nq = nover == 2 ? 2 : 3, count = 3;        // the branch layout (no over / over for k = 0) and the waveform layout
            run("empty list", none, none, 0, 0, queue, {}, nq, nover, count);
            run("empty list, arrays", std::vector<int>(1, 0), std::vector<int>(1, 0), 0, 5, queue, {}, nq, nover, count);
            run("first slot negative", {-1, 0, 1}, none, 3, 0, queue, {ok}, nq, nover, count);
            run("first slot negative, gids", {-1, 0, 1}, {7, 0, 1}, 3, 0, queue, {ok}, nq, nover, count);
            run("last entry the terminator", {2, 0, -1}, none, 3, 10, queue, {ok, rep}, nq, nover, count);
            run("no terminator", {2, 0, 1}, {1, 2, 0}, 3, 10, queue, {ok, ok, rep}, nq, nover, count);
            run("identity", none, none, 6, 0, queue, {ok, skip, nan, warm, rect, rep}, nq, nover, count);
            run("gids only", none, {5, 4, 3, 2, 1, 0}, 6, 1000, queue, {ok, skip, nan, warm, rect, rep}, nq, nover, count);
            run("slots and gids", {3, 1, 4, 0, -1, -1}, {4, 9, 2, 6, 0, 0}, 6, 1000, queue, {ok, ok, ok, ok, ok, ok, rep, ok, ok, skip}, nq, nover, count);
            run("equal maxima", {0, 0, 0}, {2, 0, 1}, 3, 0, queue, {ok, ok, ok}, nq, nover, count);
        }
    if (fails) {
        printf("%d checks failed\n", fails);
        return 1;
    }
    printf("accum clean\n");
    return 0;
}
