// TEST INFRASTRUCTURE: executes the functions of csrc/hpf_branch.hpp (what k_branch_flows / k_branch_add run per thread, and the host's branch
// numbering) serially on the host, in the kernels' own order, so that `-m "not gpu"` tests can check them against the NumPy restatement
// (tests/branch_ref.py).  It is NOT part of libhpf.so and never on the product path.
#include <vector>

#include "hpf_accum.hpp"
#include "hpf_branch.hpp"
using namespace hpf;

extern "C" {

// -> number of branches; from / to / ypos (room for nnz entries each) filled
int emul_branch_table(int n, const int* rowptr, const int* col, int* from, int* to, int* ypos) {
    std::vector<int> f, t, p;
    branch_table(n, rowptr, col, f, t, p);
    for (size_t e = 0; e < f.size(); ++e) {
        from[e] = f[e];
        to[e] = t[e];
        ypos[e] = p[e];
    }
    return (int)f.size();
}

// y [nb][Hn] branch-major, U [S][n][Hn] bus-major (the device layouts); outputs in the ABI's order: I [S][Hn][nb], irms / thd_i / loss /
// loss_harm [S][nb], loss_h [S][Hn] (tiles of BRANCH_TILE like k_branch_flows + k_branch_loss_h)
void emul_branch_flows(int n, int Hn, int nb, int S, const int* from, const int* to, const cplx* y, const cplx* U, cplx* I, double* irms,
                       double* thd_i, double* loss, double* loss_harm, double* loss_h) {
    const int tiles = (nb + BRANCH_TILE - 1) / BRANCH_TILE;
    std::vector<double> part((size_t)tiles * Hn);
    for (int s = 0; s < S; ++s) {
        const cplx* Us = U + (size_t)s * n * Hn;
        for (int tile = 0; tile < tiles; ++tile) {
            const int e0 = tile * BRANCH_TILE, ne = nb - e0 < BRANCH_TILE ? nb - e0 : BRANCH_TILE;
            for (int q = 0; q < Hn; ++q) part[(size_t)tile * Hn + q] = 0.0;
            for (int el = 0; el < ne; ++el) {
                const int e = e0 + el;
                const cplx *ye = y + (size_t)e * Hn, *ui = Us + (size_t)from[e] * Hn, *uj = Us + (size_t)to[e] * Hn;
                BranchSums a;
                branch_sums_start(a);
                for (int q = 0; q < Hn; ++q) {
                    const cplx c = branch_current(ye[q], ui[q], uj[q]);
                    const double l = branch_loss(ye[q], ui[q], uj[q]);
                    I[((size_t)s * Hn + q) * nb + e] = c;
                    branch_sums_step(a, q, branch_abs2(c), l);
                    part[(size_t)tile * Hn + q] = part[(size_t)tile * Hn + q] + l;
                }
                irms[(size_t)s * nb + e] = branch_irms(a);
                thd_i[(size_t)s * nb + e] = branch_thd_i(a);
                loss[(size_t)s * nb + e] = a.loss_all;
                loss_harm[(size_t)s * nb + e] = a.loss_harm;
            }
        }
        for (int q = 0; q < Hn; ++q) {
            double a = 0.0;
            for (int tile = 0; tile < tiles; ++tile) a = a + part[(size_t)tile * Hn + q];
            loss_h[(size_t)s * Hn + q] = a;
        }
    }
}

// the accumulator over a list as on the device (hpf_accum.hpp: L entries, slots / gids [L] or NULL, ids id_base + number; flags, thd_max [nrec]:
// the records by scenario number), branch by branch like k_branch_add; arrays accumulated INTO what the caller passes (zeroed, arg = -1, before
// the first call): f [9][nb] (irms max | sum | sumsq, loss ..., harmonic loss ...), arg [3][nb], over [nb]
void emul_branch_add(int n, int Hn, int nb, int L, const int* slots, const int* gids, int id_base, int nrec, const int* from, const int* to,
                     const cplx* y, const cplx* U, const int* flags, const double* thd_max, int queue, const double* rating, long long* counts,
                     double* f, int* arg, uint32_t* over) {
    std::vector<hpf_stat> stats((size_t)nrec);
    for (int g = 0; g < nrec; ++g) stats[g].flags = flags[g], stats[g].thd_max = thd_max[g];
    const AccumList list{L, slots, gids, id_base, queue, stats.data()};
    accum_count(list, counts);
    for (int e = 0; e < nb; ++e) {
        AccumSlot st[3];
        for (int k = 0; k < 3; ++k) st[k].load(f, arg, k == 0 ? over : nullptr, k, (size_t)nb, (size_t)e);
        const bool any = accum_walk(list, [&](int s, int id) {
            const cplx* Us = U + (size_t)s * n * Hn;
            double irms, thd_i, loss_e, loss_harm;
            branch_fold(y + (size_t)e * Hn, Us + (size_t)from[e] * Hn, Us + (size_t)to[e] * Hn, Hn, irms, thd_i, loss_e, loss_harm);
            st[0].fold(irms, id, rating[e]);
            branch_stat_fold(loss_e, id, st[1].max, st[1].arg, st[1].sum, st[1].sumsq);
            branch_stat_fold(loss_harm, id, st[2].max, st[2].arg, st[2].sum, st[2].sumsq);
        });
        if (!any) continue;
        for (int k = 0; k < 3; ++k) st[k].store(f, arg, k == 0 ? over : nullptr, k, (size_t)nb, (size_t)e);
    }
}
}
