// Stand-alone driver of the resonance mode analysis' host code for ASan + UBSan (tests/test_rma_emul.py): the serial emulation of
// csrc/hpf_resonance.hpp over exactly sized heap buffers -- one bus, sizes on both sides of the 32-bus tile of the sums and the pivot search (31, 32,
// 33, 65), chains, stars and random trees with 0 .. 8 ties, every chunk length class, with and without y_extra, with pf and without, outputs left
// out, the refused iteration counts.  An out-of-bounds access or undefined behaviour aborts it.
#include <stdio.h>
#include <stdlib.h>

#include <set>
#include <utility>

#include "rma_emul.cpp"

static unsigned long long rng_state = 88172645463325252ull;
static unsigned rnd(unsigned m) {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (unsigned)((rng_state >> 11) % m);
}

// random tree on n buses (shape 0 random parents, 1 chain, 2 star) plus `ties` extra pairs -> sorted unique (from < to) lists
static void graph(int n, int shape, int ties, std::vector<int32_t>& from, std::vector<int32_t>& to) {
    std::set<std::pair<int, int>> e;
    for (int i = 1; i < n; ++i) {
        const int p = shape == 1 ? i - 1 : shape == 2 ? 0 : (int)rnd(i);
        e.insert({p, i});
    }
    for (int guard = 0; ties > 0 && guard < 10000; ++guard) {
        const int a = (int)rnd(n), b = (int)rnd(n);
        if (a != b && e.insert({a < b ? a : b, a < b ? b : a}).second) --ties;
    }
    from.clear();
    to.clear();
    for (const auto& p : e) {
        from.push_back(p.first);
        to.push_back(p.second);
    }
}

static int run(int n, int shape, int ties, int F, int iters, int chunk, bool extra, bool full, bool peaks) {
    std::vector<int32_t> from, to;
    graph(n, shape, ties, from, to);
    const int nb = (int)from.size();
    std::vector<double> R(nb), X(nb), gsh(n), bsh(n), xsh(n, 0.0), h(F);
    for (int e = 0; e < nb; ++e) R[e] = 0.01 * (1 + rnd(5)), X[e] = 0.02 * (1 + rnd(4));
    for (int i = 0; i < n; ++i) gsh[i] = 1e-4 * rnd(3), bsh[i] = 1e-3 * rnd(3);
    xsh[0] = 0.005;
    for (int f = 0; f < F; ++f) h[f] = 0.5 + 0.37 * f;
    std::vector<cplx> yx(extra ? (size_t)F * n : 0);
    for (auto& v : yx) v = {0.0, 1e-3 * rnd(7)};
    std::vector<cplx> lam(F), pf(full ? (size_t)F * n : 0);
    std::vector<double> zm(F), res(F);
    std::vector<int32_t> top(F);
    return emul_resonance_modes(n, nb, from.data(), to.data(), R.data(), X.data(), gsh.data(), bsh.data(), xsh.data(), F, h.data(),
                                extra ? yx.data() : nullptr, iters, chunk, peaks ? lam.data() : nullptr, zm.data(), peaks ? res.data() : nullptr,
                                peaks ? top.data() : nullptr, full ? pf.data() : nullptr);
}

int main() {
    int cases = 0;
    for (int n : {1, 2, 31, 32, 33, 65})
        for (int shape = 0; shape < 3; ++shape)
            for (int ties : {0, 1, 8}) {
                const int t = n < 6 ? 0 : ties;
                for (int chunk : {0, 1, 17, 64}) {
                    const int rc = run(n, shape, t, 70, 1 + cases % 4, chunk, cases % 2 == 0, cases % 4 != 3, cases % 5 != 4);
                    if (rc != HPF_OK && rc != HPF_E_SINGULAR) {
                        printf("case %d: code %d\n", cases, rc);
                        return 1;
                    }
                    ++cases;
                }
            }
    if (run(12, 0, 9, 5, 3, 0, false, true, true) != HPF_E_TOPOLOGY) return 2;     // nine ties
    if (run(9, 1, 0, 5, 0, 0, false, true, true) != HPF_E_ARG || run(9, 1, 0, 5, 257, 0, false, true, true) != HPF_E_ARG) return 3;
    if (run(9, 1, 0, 5, 256, 2, false, true, true) != HPF_OK) return 4;
    printf("rma clean: %d cases\n", cases);
    return 0;
}
