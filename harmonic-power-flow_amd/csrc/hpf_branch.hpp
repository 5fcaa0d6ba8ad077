// Branch flows (hpf_branch_flows, hpf_branch_stats_*): the per-entry arithmetic of the series current and loss of one stored off-diagonal
// pair of the admittance pattern.  k_branch_flows / k_branch_add (hpf_lib.hip) run these functions on the device; the host emulation
// (tests/cpu_emul/branch_emul.cpp) runs the same functions serially.  Every product and sum is rounded on its own (-ffp-contract=off), every
// sum over the harmonics runs over ascending q in one thread, and nothing here is atomic.
//   branch e = (i, j), i < j;  y[q] = -Y[q][pos(i, j)];  d[q] = U[i][q] - U[j][q]
//   I[q] = y[q] d[q]            (positive from the lower-numbered bus to the higher)
//   loss[q] = Re(y[q]) |d[q]|^2 (= R |I|^2 for y = 1 / (R + j h X): never negative)
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

#include "hpf_assembly.hpp"
#include "hpf_distortion.hpp"

namespace hpf {

// loss_h[q] = sum over the branches: tiles of BRANCH_TILE consecutive branches, ascending e inside a tile starting from 0.0, then the tile sums
// in ascending tile order starting from 0.0 -- an order that depends on the number of branches alone
constexpr int BRANCH_TILE = 32;

HPF_DIST_HD cplx branch_current(cplx y, cplx ui, cplx uj) { return cmul_unf(y, csub(ui, uj)); }

HPF_DIST_HD double branch_loss(cplx y, cplx ui, cplx uj) {
    const cplx d = csub(ui, uj);
    return y.re * (d.re * d.re + d.im * d.im);
}

HPF_DIST_HD double branch_abs2(cplx I) { return I.re * I.re + I.im * I.im; }

// the four running sums of one branch over ascending q: |I|^2 over all q and over q >= 1, loss over all q and over q >= 1
struct BranchSums {
    double i2_all, i2_harm, i2_fund, loss_all, loss_harm;
};

HPF_DIST_HD void branch_sums_start(BranchSums& a) { a.i2_all = a.i2_harm = a.i2_fund = a.loss_all = a.loss_harm = 0.0; }

HPF_DIST_HD void branch_sums_step(BranchSums& a, int q, double i2, double loss) {
    a.i2_all = a.i2_all + i2;
    a.loss_all = a.loss_all + loss;
    if (q == 0) {
        a.i2_fund = i2;
    } else {
        a.i2_harm = a.i2_harm + i2;
        a.loss_harm = a.loss_harm + loss;
    }
}

HPF_DIST_HD double branch_irms(const BranchSums& a) { return sqrt(a.i2_all); }
HPF_DIST_HD double branch_thd_i(const BranchSums& a) { return sqrt(a.i2_harm) / sqrt(a.i2_fund); }   // (0 / 0 = NaN, x / 0 = inf: like THD_F)

// the fold of one scenario's Hn harmonics of a branch: y [Hn] (series admittances), ui / uj [Hn] (the two buses' rectangular voltages)
HPF_DIST_HD void branch_fold(const cplx* y, const cplx* ui, const cplx* uj, int Hn, double& irms, double& thd_i, double& loss_e,
                             double& loss_harm) {
    BranchSums a;
    branch_sums_start(a);
    for (int q = 0; q < Hn; ++q) branch_sums_step(a, q, branch_abs2(branch_current(y[q], ui[q], uj[q])), branch_loss(y[q], ui[q], uj[q]));
    irms = branch_irms(a);
    thd_i = branch_thd_i(a);
    loss_e = a.loss_all;
    loss_harm = a.loss_harm;
}

// the statistics of a sweep reuse the distortion accumulator's fold (max, arg with the smaller-id tie rule, sum, sum of squares, count above a
// limit); the two loss quantities have no limit
HPF_DIST_HD void branch_stat_fold(double x, int id, double& mx, int& arg, double& sum, double& sumsq) {
    uint32_t none = 0u;
    dist_fold(x, id, (double)INFINITY, mx, arg, sum, sumsq, none);
}

// the branch numbering (host): stored pairs (i, j), i < j, of the CSR pattern, row-major, columns ascending -> from, to, position in col
inline void branch_table(int n, const int* rowptr, const int* col, std::vector<int>& from, std::vector<int>& to, std::vector<int>& ypos) {
    from.clear();
    to.clear();
    ypos.clear();
    for (int i = 0; i < n; ++i)
        for (int e = rowptr[i]; e < rowptr[i + 1]; ++e)
            if (col[e] > i) {
                from.push_back(i);
                to.push_back(col[e]);
                ypos.push_back(e);
            }
}

}  // namespace hpf
