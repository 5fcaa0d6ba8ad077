// Lazy leaves, 16 scenarios per workgroup (included by hpf_block.hip after hpf_quad.hpp).
//
// A lazy constant-inverse leaf owes the factor sweep only vectors: w = D^-1 y, G w for its parent, its 2x2 core K
// with the position-0 borders, S^-1 and A(k,parent) for the back sweep.  The one O(b^2) piece, Drect^-1 y, multiplies a PER-MODEL
// matrix with a per-scenario vector -- across scenarios that is a GEMM:
//     Drect^-1 y = [u; Vh + Lc u],   V = [0 Lr; 0 Ahh^-1] y,   u = K (y0 + V0),   K = (c0 + Delta_polar S_0^-1)^-1.
// One workgroup takes one leaf and SB = 16 scenarios: V for all 16 is b/4 rank-4 MFMAs per 16-row tile (A operand = the image in
// operand layout, read ONCE per 16 scenarios instead of once per scenario; B operand = the 16 right-hand sides from LDS), the
// roles of k_factor_q (right-hand side with the 2x2-algebra children folded in, S^-1, coupling blocks) run per (scenario, row) /
// (scenario, harmonic) thread.  Results are the same quantities k_factor_q<B, true> leaves for a lazy leaf.
#pragma once

// The factor bodies (leaf_batch_body / sleaf_batch_body) also come with tiles of SB = 8 scenarios, 32 threads per scenario: each thread then
// walks half the rows and harmonics in sequence, for launches too narrow to fill the chip (HPF_BATCH_TILE8_MAX).  What a
// row or a harmonic computes is the same operation for operation; the LDS arrays keep their shape and the MFMAs their 16 B-operand columns
// (columns 8.. are zero).  The back-sweep bodies below, and every per-scenario HBM layout, know tiles of 16 only.
constexpr int LB_SB = 16;      // scenarios per workgroup (the larger tile)
constexpr int LBP = LB_SB + 1; // row stride of the [row][scenario] arrays in LDS (odd: a wave's 16 rows x 4 scenarios spread over the banks
                               // instead of meeting in one bank pair -- LDS bank conflicts per LDS instruction 6.9 -> see profiles/r03)

// per-leaf constants (Tree::d_lbimg): A-operand image [NTR][KS][64] | Lc as real b x 2 | c0 2x2
template <int B>
struct LeafBatchImg {
    static constexpr int NTR = (B + 15) / 16, KS = (B + 3) / 4;
    static constexpr int SZ = NTR * KS * 64 + 2 * B + 4;
};

// per-bus constants of a bordered bus (Tree::d_sbimg): A-operand image [NTR][KS][64] of [0 0; 0 Ahh^-1] -- with the rows of Qb in
// the padding rows B.. of the last row tile when m <= 10 of them fit (QB_ROWS: r = Qb v falls out of the same MFMAs) -- and Pb
// (b x m) as a second A operand [NTR][3][64] (x += Pb y: three rank-4 steps)
template <int B>
struct SleafImg {
    static constexpr int NTR = (B + 15) / 16, KS = (B + 3) / 4, KP = 3;
    static constexpr int MAIN = NTR * KS * 64, SZ = MAIN + NTR * KP * 64;
    static constexpr bool QB_ROWS = 16 * NTR - B >= 10;
};

constexpr int LEAF_BATCH_LDS = 2 * 64 * LBP + LB_SB * 4 + LB_SB * 2;      // doubles

template <int B, int SB>
__device__ __forceinline__ void leaf_batch_body(
    double* __restrict__ smem_, const int bx_, const int by_, const Model& M, const TreeDev& T, const int* __restrict__ nodes, int b, const int* __restrict__ active, int S_cnt,
    const cplx* __restrict__ Uall, const cplx* __restrict__ Eall, const double* __restrict__ fall, double* __restrict__ wall,
    const double* __restrict__ linAall, double* __restrict__ Call, double* __restrict__ Hall, const double* __restrict__ chG,
    const double* __restrict__ chH, const double* __restrict__ chD, const double* __restrict__ chy,
    const double* __restrict__ lbimg, double* __restrict__ lfK, double* __restrict__ lfS, int s0) {
    constexpr int NT = (B + 16) / 16;                       // tile columns of the block kernels (slot stride of C)
    constexpr size_t CT = (size_t)NT * NT * 256;
    constexpr int NTR = LeafBatchImg<B>::NTR, KS = LeafBatchImg<B>::KS, H2 = B / 2;
    const int4* nd = reinterpret_cast<const int4*>(nodes) + (FDESC / 4) * (size_t)bx_;
    const int4 nd0 = nd[0], nd1 = nd[1], nd3 = nd[3];
    const int k = nd0.x, par = nd0.y;
    const int e_dn_k = nd1.x, e_up_k = nd1.y, lin_beg = nd1.z, lin_end = nd1.z + nd1.w;
    const bool via_chain = (nd3.z & 1) != 0;
    const int slot = nd3.w - 1;                              // leaf slot (Tree::d_Minv numbering)
    const int tid = threadIdx.x, lane = tid & 63, lg = lane >> 4, jj = lane & 15;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = M.n, c = M.c, Hn = M.Hn;
    using TL = BatchTile<SB>;                                // role mapping: TL::TPS threads per scenario (hpf_batch_tile.hpp)
    constexpr int RPT = TL::ROWS;                            // rows per thread
    const int sc = TL::scenario(tid), lt = TL::lane(tid);
    const int sl = by_ * SB + sc;                            // scenario inside the launch
    const int ss = sl < S_cnt ? (active ? active[sl + s0] : sl + s0) : -1;      // slot -> scenario (active list; -1: frozen / empty slot)
    const bool live = ss >= 0;
    const int s = live ? ss : 0;
    const size_t so = (size_t)s * n * Hn;
    const cplx* U = Uall + so;
    const cplx* E = Eall + so;
    const double* img = lbimg + (size_t)slot * LeafBatchImg<B>::SZ;
    const double* lcimg = img + NTR * KS * 64;               // R(Lc): [row][2] (rows 0, 1: identity)
    const double* c0img = lcimg + 2 * B;

    double* Y = smem_;                                       // right-hand sides [row][scenario]
    double* V = Y + 64 * LBP;                              // [0 Lr; 0 Ahh^-1] y
    double* DL = V + 64 * LBP;                             // Delta_polar per scenario
    double* UK = DL + LB_SB * 4;                             // u = K (y0 + V0)
    constexpr int QI = TL::harmonics(H2);                    // harmonics per thread
    double sir[QI][4], glr[QI][4];                           // S_q^-1 and A(parent, k) of the thread's harmonics (same mapping in R2, K, F)

    // ---- R1. rows: right-hand side and the 2x2 term of the fundamental, the 2x2-algebra children folded in (k_factor_q, wave 0
    //      role + children, here one thread per (scenario, row) and every child of the bus in list order) -------------------------
    {
        // (the thread's four rows side by side: the children loop runs once, with the loads of all four rows in flight)
        double e0[RPT] = {}, e1[RPT] = {}, ey[RPT] = {};
        double a0[RPT] = {}, a1[RPT] = {}, ay[RPT] = {}, fy[RPT] = {};
        bool ok[RPT];
        cplx ukr[RPT], ekr[RPT];
#pragma unroll
        for (int pz = 0; pz < RPT; ++pz) {
            const int row = TL::row(tid, pz), q = row >> 1, tr_ = row & 1;
            ok[pz] = live && row < b && loc_valid(n, c, k, row);
            ukr[pz] = cplx{0.0, 0.0};
            ekr[pz] = cplx{0.0, 0.0};
            if (ok[pz]) {
                const size_t kq = (size_t)k * Hn + q;
                fy[pz] = fall[((size_t)s * n + k) * B + row];
                if (via_chain) {
                    const size_t o = so + kq;
                    a0[pz] = chD[o * 4 + 2 * tr_];
                    a1[pz] = chD[o * 4 + 2 * tr_ + 1];
                    ay[pz] = chy[o * 2 + tr_];
                }
                if (lin_beg < lin_end) {
                    ukr[pz] = U[kq];
                    ekr[pz] = E[kq];
                }
            }
        }
        const double* ws = wall + (size_t)s * n * B;
        const double* linA = linAall + so * 4;
        const int4* c3 = reinterpret_cast<const int4*>(T.child3);
        for (int cp = lin_beg; cp < lin_end; ++cp) {
            const int4 cr = c3[cp];
            const int ch = cr.x;
#pragma unroll
            for (int pz = 0; pz < RPT; ++pz) {
                if (!ok[pz]) continue;
                const int row = TL::row(tid, pz), q = row >> 1, tr_ = row & 1;
                const cplx uk = ukr[pz], ek = ekr[pz];
                const cplx ydn = M.Y[(size_t)cr.y * Hn + q], yup = M.Y[(size_t)cr.z * Hn + q];
                const cplx uc = U[(size_t)ch * Hn + q], ec = E[(size_t)ch * Hn + q];
                const double2* pic = reinterpret_cast<const double2*>(linA + ((size_t)ch * Hn + q) * 4);
                const double2 ic01 = pic[0], ic23 = pic[1];
                const double2 wc = *reinterpret_cast<const double2*>(ws + (size_t)ch * B + 2 * q);
                const Blk2 g = (q == 0 && k < M.m) ? blk_power_off(ydn, uk, uc, ec) : blk_current(ydn, uc, ec);   // A(k, child)
                const Blk2 hb = (q == 0 && ch < M.m) ? blk_power_off(yup, uc, uk, ek) : blk_current(yup, uk, ek);  // A(child, k)
                const double g0 = pick(g, tr_, 0);
                const double g1 = loc_valid(n, c, ch, 2 * q + 1) ? pick(g, tr_, 1) : 0.0;
                double h4[4];
                mask_block(n, c, q, ch, k, hb, h4);
                const double v0 = fma(g1, ic23.x, g0 * ic01.x), v1 = fma(g1, ic23.y, g0 * ic01.y);
                e0[pz] += fma(v1, h4[2], v0 * h4[0]);
                e1[pz] += fma(v1, h4[3], v0 * h4[1]);
                ey[pz] = fma(g0, wc.x, ey[pz]);
                ey[pz] = fma(g1, wc.y, ey[pz]);
            }
        }
#pragma unroll
        for (int pz = 0; pz < RPT; ++pz) {
            const int row = TL::row(tid, pz);
            Y[row * LBP + sc] = ok[pz] ? fy[pz] + ay[pz] - ey[pz] : 0.0;
            if (SB < BATCH_COLS) Y[row * LBP + SB + sc] = 0.0;      // (the B-operand columns behind the tile)
            if (row < 2) {
                DL[sc * 4 + row * 2] = ok[pz] ? a0[pz] - e0[pz] : 0.0;
                DL[sc * 4 + row * 2 + 1] = ok[pz] ? a1[pz] - e1[pz] : 0.0;
            }
        }
    }
    // ---- R2. harmonics: S_q^-1, the coupling blocks with the parent (H is kept for the back sweep), the position-0 borders ----
#pragma unroll
    for (int it = 0; it < QI; ++it) {
        const int q = TL::harmonic(tid, it);
        double si[4] = {1.0, 0.0, 0.0, 1.0}, g4[4] = {0.0, 0.0, 0.0, 0.0}, h4[4] = {0.0, 0.0, 0.0, 0.0};
        if (live && q < Hn) {
            const cplx uk = U[(size_t)k * Hn + q], ek = E[(size_t)k * Hn + q];
            const double idet = 1.0 / (-(uk.im * ek.im) - ek.re * uk.re);      // S = [-ui er; ur ei]
            si[0] = ek.im * idet;   si[1] = -ek.re * idet;
            si[2] = -uk.re * idet;  si[3] = -uk.im * idet;
            cplx up = {0.0, -1.0}, ep = {0.0, 1.0};
            if (!via_chain || q == 0) {
                up = U[(size_t)par * Hn + q];
                ep = E[(size_t)par * Hn + q];
            }
            if (via_chain) {
                const double2* pg = reinterpret_cast<const double2*>(chG + (so + (size_t)k * Hn + q) * 4);
                const double2* ph = reinterpret_cast<const double2*>(chH + (so + (size_t)k * Hn + q) * 4);
                const double2 ga = pg[0], gb = pg[1], ha = ph[0], hb = ph[1];
                g4[0] = ga.x; g4[1] = ga.y; g4[2] = gb.x; g4[3] = gb.y;
                h4[0] = ha.x; h4[1] = ha.y; h4[2] = hb.x; h4[3] = hb.y;
            } else {
                const cplx ydn = M.Y[(size_t)e_dn_k * Hn + q], yup = M.Y[(size_t)e_up_k * Hn + q];
                const Blk2 g = (q == 0 && par < M.m) ? blk_power_off(ydn, up, uk, ek) : blk_current(ydn, uk, ek);   // row par, col k
                const Blk2 hh = (q == 0 && k < M.m) ? blk_power_off(yup, uk, up, ep) : blk_current(yup, up, ep);     // row k, col par
                mask_block(n, c, q, par, k, g, g4);
                mask_block(n, c, q, k, par, hh, h4);
            }
            double* Hk = Hall + ((size_t)s * n + k) * Hn * 4 + q * 4;
            double* Sk = lfS + (so + (size_t)k * Hn + q) * 4;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                Hk[e] = h4[e];
                Sk[e] = si[e];
            }
            if (q == 0) {                                    // G0 S_c^-1, H0 S_p^-1 for the parent's rebuild
                const double ip = 1.0 / (-(up.im * ep.im) - ep.re * up.re);
                const double sp0 = ep.im * ip, sp1 = -ep.re * ip, sp2 = -up.re * ip, sp3 = -up.im * ip;
                double* kk = lfK + ((size_t)s * n + k) * 12 + 4;
                kk[0] = fma(g4[1], si[2], g4[0] * si[0]);  kk[1] = fma(g4[1], si[3], g4[0] * si[1]);
                kk[2] = fma(g4[3], si[2], g4[2] * si[0]);  kk[3] = fma(g4[3], si[3], g4[2] * si[1]);
                kk[4] = fma(h4[1], sp2, h4[0] * sp0);  kk[5] = fma(h4[1], sp3, h4[0] * sp1);
                kk[6] = fma(h4[3], sp2, h4[2] * sp0);  kk[7] = fma(h4[3], sp3, h4[2] * sp1);
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            sir[it][e] = si[e];
            glr[it][e] = g4[e];
        }
    }
    __syncthreads();
    // ---- M. V = [0 Lr; 0 Ahh^-1] Y for the 16 scenarios: wave w owns rows 16 w .. 16 w + 15 ---------------------------------------
    if (wv < NTR) {
        d4_t acc = {0.0, 0.0, 0.0, 0.0};
        const double* ia = img + (size_t)wv * KS * 64 + lane;
#pragma unroll 4
        for (int ks = 0; ks < KS; ++ks) {
            const double a = ia[(size_t)ks * 64];
            const double bop = Y[(4 * ks + lg) * LBP + jj];
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bop, acc, 0, 0, 0);
        }
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) V[(16 * wv + 4 * reg + lg) * LBP + jj] = acc[reg];
    }
    __syncthreads();
    // ---- K. per scenario: K = (c0 + Delta_polar S_0^-1)^-1, u = K (y0 + V0) --------------------------------------------------------
    if (lt == 0) {
        const double* si = sir[0];                           // (q = 0 belongs to this thread)
        const double* dl = DL + sc * 4;
        const double q00 = c0img[0] + fma(dl[1], si[2], dl[0] * si[0]), q01 = c0img[1] + fma(dl[1], si[3], dl[0] * si[1]);
        const double q10 = c0img[2] + fma(dl[3], si[2], dl[2] * si[0]), q11 = c0img[3] + fma(dl[3], si[3], dl[2] * si[1]);
        double k00, k01, k10, k11;
        inv2(q00, q01, q10, q11, k00, k01, k10, k11);
        const double r0 = Y[sc] + V[sc], r1 = Y[LBP + sc] + V[LBP + sc];
        UK[sc * 2] = fma(k01, r1, k00 * r0);
        UK[sc * 2 + 1] = fma(k11, r1, k10 * r0);
        if (live) {
            double* kk = lfK + ((size_t)s * n + k) * 12;
            kk[0] = k00; kk[1] = k01; kk[2] = k10; kk[3] = k11;
        }
    }
    __syncthreads();
    // ---- F. per (scenario, harmonic): x_rect = [u; Vh + Lc u], w = S_q^-1 x_rect, G w for the parent -----------------------------
    if (live) {
        const double u0 = UK[sc * 2], u1 = UK[sc * 2 + 1];
        double* wk = wall + ((size_t)s * n + k) * B;
        double* Ck = Call + ((size_t)s * n + k) * CT;
#pragma unroll
        for (int it = 0; it < QI; ++it) {
            const int q = TL::harmonic(tid, it);
            if (q >= H2) continue;
            double x0 = u0, x1 = u1;
            if (q > 0) {
                const double* lc = lcimg + (2 * q) * 2;
                x0 = V[(2 * q) * LBP + sc] + fma(lc[1], u1, lc[0] * u0);
                x1 = V[(2 * q + 1) * LBP + sc] + fma(lc[3], u1, lc[2] * u0);
            }
            const double* si = sir[it];
            const bool in = 2 * q < b;
            const double w0 = in ? fma(si[1], x1, si[0] * x0) : 0.0, w1 = in ? fma(si[3], x1, si[2] * x0) : 0.0;
            const double* g = glr[it];
            wk[2 * q] = w0;
            wk[2 * q + 1] = w1;
            Ck[2 * q] = fma(g[1], w1, g[0] * w0);
            Ck[2 * q + 1] = fma(g[3], w1, g[2] * w0);
        }
    }
}

template <int B, int SB>
__global__ __launch_bounds__(256, 4) void k_leaf_batch(
    Model M, TreeDev T, const int* __restrict__ nodes, int b, const int* __restrict__ active, int S_cnt,
    const cplx* __restrict__ Uall, const cplx* __restrict__ Eall, const double* __restrict__ fall, double* __restrict__ wall,
    const double* __restrict__ linAall, double* __restrict__ Call, double* __restrict__ Hall, const double* __restrict__ chG,
    const double* __restrict__ chH, const double* __restrict__ chD, const double* __restrict__ chy,
    const double* __restrict__ lbimg, double* __restrict__ lfK, double* __restrict__ lfS, int s0) {
    __shared__ __attribute__((aligned(16))) double smem[LEAF_BATCH_LDS];
    leaf_batch_body<B, SB>(smem, blockIdx.x, blockIdx.y, M, T, nodes, b, active, S_cnt, Uall, Eall, fall, wall, linAall, Call, Hall, chG, chH, chD, chy,
                           lbimg, lfK, lfS, s0);
}

template <int B, int SB>
int launch_leaf_batch(hpf_handle* h, const LaunchCtx& ctx, const TreeDev& T, const int* nodes, int count) {
    ScopedTimer t(h, T_SOLVE, ctx.stream);
    const dim3 grid((unsigned)count, (unsigned)BatchTile<SB>::tiles(ctx.S));
    hipLaunchKernelGGL((k_leaf_batch<B, SB>), grid, dim3(256), 0, ctx.stream, h->M, T, nodes, 2 * h->Hn, ctx.active, ctx.S, h->d_U,
                       h->d_E, h->d_fb, h->d_w, h->d_linA, h->d_C, h->d_H, h->d_chG, h->d_chH, h->d_chD, h->d_chy,
                       active_tree(h).d_lbimg, h->d_lfK, h->d_lfS, ctx.s0);
    return launch_status(h);
}

// The thread's place in a scenario-batched back-sweep workgroup (16 threads per scenario) and its scenario
struct BatchLane {
    int tid, lane, lg, jj, wv, sc, l16, s;
    bool live;
};

__device__ __forceinline__ BatchLane batch_lane(int by_, const int* __restrict__ active, int S_cnt, int s0) {
    BatchLane L;
    L.tid = threadIdx.x; L.lane = L.tid & 63; L.lg = L.lane >> 4; L.jj = L.lane & 15;
    L.wv = __builtin_amdgcn_readfirstlane(L.tid >> 6);
    L.sc = L.tid >> 4; L.l16 = L.tid & 15;
    const int sl = by_ * LB_SB + L.sc;
    const int ss = sl < S_cnt ? (active ? active[sl + s0] : sl + s0) : -1;      // slot -> scenario (active list; -1: frozen / empty slot)
    L.live = ss >= 0;
    L.s = L.live ? ss : 0;
    return L;
}

// One bus of a batched back-sweep body, from its record (workgroup-uniform).  pslot: where x_parent is -- an LDS slot of k_back_tail's store,
// -1: in HBM since an earlier launch (the load part fetches it), -2: in HBM, written by this very thread earlier in this launch (read when
// the compute part starts); oslot: the LDS slot the bus's own x goes to besides HBM (-1: none)
struct BatchBus {
    int kind, k, par, m, pslot, oslot;    // kind 0: bordered bus, 1: leaf
    const double* img;                    // its per-model image
    const double* qbm;                    // bordered bus: Qb [m][b]
};

// Everything a batched back-sweep body reads from HBM for one bus, held in registers between its load parts and its compute parts (as BackQIn
// is for k_back_q).  One type for both bodies -- tr: the thread's row of T^-1 (bordered bus) or K | Lc of its harmonics (leaf).  The
// operands come in two halves by their last use: `early` ones (A(k,parent), x_parent, W_k^-1, the image column of the first MFMAs) are free
// again after the first half of the compute part, `late` ones (tr, the Pb column, S^-1, w) at its end -- k_back_tail refills each half
// with the next member's there, so those requests are in flight while the current member computes, in no more registers than one bus needs.
template <int B>
struct BatchBackIn {
    static constexpr int KS = SleafImg<B>::KS, KP = SleafImg<B>::KP, QI = (B / 2 + 15) / 16;
    double ia[KS], wi[4], hk[2][4], xp[2][2];                 // early
    double pa[KP], tr[12], si4[QI][4], w4[QI][2];             // late
};

// early operands of both kinds: the lane's image column, A(k,parent) and, where it is in HBM already, x_parent of the harmonics l16, l16 + 16
template <int B>
__device__ __forceinline__ void batch_back_load_early(BatchBackIn<B>& I, const BatchBus& U, const BatchLane& L, const Model& M,
                                                      const double* __restrict__ xall, const double* __restrict__ Hall) {
    constexpr int NTR = SleafImg<B>::NTR, KS = SleafImg<B>::KS;
    const int n = M.n, Hn = M.Hn;
    if (L.wv < NTR) {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) I.ia[ks] = U.img[((size_t)L.wv * KS + ks) * 64 + L.lane];
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int q = L.l16 + 16 * j;
        I.hk[j][0] = I.hk[j][1] = I.hk[j][2] = I.hk[j][3] = 0.0;
        I.xp[j][0] = I.xp[j][1] = 0.0;
        if (L.live && q < Hn) {
            const double* hk = Hall + (((size_t)L.s * n + U.k) * Hn + q) * 4;
            I.hk[j][0] = hk[0]; I.hk[j][1] = hk[1]; I.hk[j][2] = hk[2]; I.hk[j][3] = hk[3];
            if (U.pslot == -1) {
                const double2 xp = *reinterpret_cast<const double2*>(xall + ((size_t)L.s * n + U.par) * B + 2 * q);
                I.xp[j][0] = xp.x; I.xp[j][1] = xp.y;
            }
        }
    }
}

// t = A(k,parent) x_parent of harmonic l16 + 16 j; x_parent from the family's LDS store (the thread's own entries: it wrote them), else from HBM
template <int B>
__device__ __forceinline__ void batch_back_t(const BatchBackIn<B>& I, const BatchBus& U, const BatchLane& L, const Model& M, const double* xall,
                                             const double2* XS, int j, double& t0, double& t1) {
    constexpr int QI = BatchBackIn<B>::QI;
    double2 xp = double2{I.xp[j][0], I.xp[j][1]};
    if (U.pslot >= 0) xp = XS[((size_t)U.pslot * QI + (j < QI ? j : 0)) * 256 + L.tid];
    else if (U.pslot == -2) xp = *reinterpret_cast<const double2*>(xall + ((size_t)L.s * M.n + U.par) * B + 2 * (L.l16 + 16 * j));
    const double* hk = I.hk[j];
    t0 = fma(hk[1], xp.y, hk[0] * xp.x);
    t1 = fma(hk[3], xp.y, hk[2] * xp.x);
}

// Back sweep of the constant-inverse leaves, 16 scenarios per workgroup:  x_k = w_k - S^-1 Drect^-1 t,  t = A(k,parent) x_parent,
// Drect^-1 t = [u; Vh + Lc u],  V = [0 Lr; 0 Ahh^-1] t  (the same per-model image on the matrix cores),  u = K (t0 + V0).
// nodes: Tree::d_bdesc records (bus, parent, leaf slot + 1, 0) of leaves only.
template <int B>
__device__ __forceinline__ BatchBus leaf_back_bus(const int4 kp, int pslot, int oslot, const double* __restrict__ lbimg) {
    return BatchBus{1, kp.x, kp.y, 0, pslot, oslot, lbimg + (size_t)(kp.z - 1) * LeafBatchImg<B>::SZ, nullptr};
}

// late operands: K, and Lc / S^-1 / w of the thread's harmonics (with the early ones: one round trip for everything addressed by the record)
template <int B>
__device__ __forceinline__ void leaf_back_load_late(BatchBackIn<B>& I, const BatchBus& U, const BatchLane& L, const Model& M,
                                                    const double* __restrict__ wall, const double* __restrict__ lfK, const double* __restrict__ lfS) {
    constexpr int NTR = LeafBatchImg<B>::NTR, KS = LeafBatchImg<B>::KS, H2 = B / 2, QI = (H2 + 15) / 16;
    const int k = U.k, n = M.n, Hn = M.Hn, s = L.s, l16 = L.l16;
    const bool live = L.live;
    const double* lcimg = U.img + NTR * KS * 64;
    I.tr[0] = I.tr[1] = I.tr[2] = I.tr[3] = 0.0;
    if (live && l16 == 0) {
        const double* kk = lfK + ((size_t)s * n + k) * 12;
        I.tr[0] = kk[0]; I.tr[1] = kk[1]; I.tr[2] = kk[2]; I.tr[3] = kk[3];
    }
#pragma unroll
    for (int it = 0; it < QI; ++it) {
        const int q = l16 + 16 * it;
        double* lc4 = I.tr + 4 + 4 * it;
        I.w4[it][0] = I.w4[it][1] = 0.0;
        I.si4[it][0] = I.si4[it][3] = 1.0;
        I.si4[it][1] = I.si4[it][2] = 0.0;
        lc4[0] = lc4[1] = lc4[2] = lc4[3] = 0.0;
        if (live && q < H2) {
            const double2* lp = reinterpret_cast<const double2*>(lcimg + (2 * q) * 2);
            const double2 l0 = lp[0], l1 = lp[1];
            lc4[0] = l0.x; lc4[1] = l0.y; lc4[2] = l1.x; lc4[3] = l1.y;
            if (q < Hn) {
                const double2* sp = reinterpret_cast<const double2*>(lfS + (((size_t)s * n + k) * Hn + q) * 4);
                const double2 a = sp[0], c2 = sp[1];
                I.si4[it][0] = a.x; I.si4[it][1] = a.y; I.si4[it][2] = c2.x; I.si4[it][3] = c2.y;
            }
            const double2 w2 = *reinterpret_cast<const double2*>(wall + ((size_t)s * n + k) * B + 2 * q);
            I.w4[it][0] = w2.x;
            I.w4[it][1] = w2.y;
        }
    }
}

// Compute part, first half (the early operands are free after it).  TT: t = A(k,parent) x_parent, [row][scenario]; V [64 * LBP]
template <int B>
__device__ __forceinline__ void leaf_back_compute_a(const BatchBackIn<B>& I, const BatchBus& U, const BatchLane& L, const Model& M, const double* xall,
                                                    double* __restrict__ TT, double* __restrict__ V, const double2* XS) {
    constexpr int NTR = LeafBatchImg<B>::NTR, KS = LeafBatchImg<B>::KS;
    const int lg = L.lg, jj = L.jj, wv = L.wv, sc = L.sc, l16 = L.l16;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int q = l16 + 16 * j;
        double t0 = 0.0, t1 = 0.0;
        if (L.live && q < M.Hn) batch_back_t<B>(I, U, L, M, xall, XS, j, t0, t1);
        TT[(2 * q) * LBP + sc] = t0;
        TT[(2 * q + 1) * LBP + sc] = t1;
    }
    __syncthreads();
    if (wv < NTR) {
        d4_t acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const double bop = TT[(4 * ks + lg) * LBP + jj];
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(I.ia[ks], bop, acc, 0, 0, 0);
        }
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) V[(16 * wv + 4 * reg + lg) * LBP + jj] = acc[reg];
    }
}

// ... second half.  UK [LB_SB * 2]
template <int B>
__device__ __forceinline__ void leaf_back_compute_b(const BatchBackIn<B>& I, const BatchBus& U, const BatchLane& L, const Model& M, double* xall,
                                                    const double* __restrict__ TT, const double* __restrict__ V, double* __restrict__ UK) {
    constexpr int H2 = B / 2, QI = (H2 + 15) / 16;
    const int k = U.k, sc = L.sc, l16 = L.l16;
    double* xs = xall + (size_t)L.s * M.n * B;
    __syncthreads();
    if (l16 == 0) {
        const double r0 = TT[sc] + V[sc], r1 = TT[LBP + sc] + V[LBP + sc];                      // [I Lr] t
        UK[sc * 2] = fma(I.tr[1], r1, I.tr[0] * r0);
        UK[sc * 2 + 1] = fma(I.tr[3], r1, I.tr[2] * r0);
    }
    __syncthreads();
    if (L.live) {
        const double u0 = UK[sc * 2], u1 = UK[sc * 2 + 1];
#pragma unroll
        for (int it = 0; it < QI; ++it) {
            const int q = l16 + 16 * it;
            if (q >= H2) continue;
            const double* lc4 = I.tr + 4 + 4 * it;
            double x0 = u0, x1 = u1;
            if (q > 0) {
                x0 = V[(2 * q) * LBP + sc] + fma(lc4[1], u1, lc4[0] * u0);
                x1 = V[(2 * q + 1) * LBP + sc] + fma(lc4[3], u1, lc4[2] * u0);
            }
            const double d0 = fma(I.si4[it][1], x1, I.si4[it][0] * x0), d1 = fma(I.si4[it][3], x1, I.si4[it][2] * x0);
            *reinterpret_cast<double2*>(xs + (size_t)k * B + 2 * q) = double2{I.w4[it][0] - d0, I.w4[it][1] - d1};
        }
    }
}

template <int B>
__device__ __forceinline__ void leaf_back_batch_body(
    const int bx_, const int by_, const Model& M, const int* __restrict__ nodes, int b, const int* __restrict__ active, int S_cnt, const double* __restrict__ wall,
    double* __restrict__ xall, const double* __restrict__ Hall, const double* __restrict__ lbimg, const double* __restrict__ lfK,
    const double* __restrict__ lfS, int s0) {
    __shared__ double TT[64 * LBP];                        // t = A(k,parent) x_parent, [row][scenario]
    __shared__ double V[64 * LBP];
    __shared__ double UK[LB_SB * 2];
    const BatchLane L = batch_lane(by_, active, S_cnt, s0);
    const BatchBus U = leaf_back_bus<B>(reinterpret_cast<const int4*>(nodes)[bx_], -1, -1, lbimg);
    BatchBackIn<B> I;
    batch_back_load_early<B>(I, U, L, M, xall, Hall);
    leaf_back_load_late<B>(I, U, L, M, wall, lfK, lfS);
    leaf_back_compute_a<B>(I, U, L, M, xall, TT, V, nullptr);
    leaf_back_compute_b<B>(I, U, L, M, xall, TT, V, UK);
}

template <int B>
__global__ __launch_bounds__(256) void k_leaf_back_batch(
    Model M, const int* __restrict__ nodes, int b, const int* __restrict__ active, int S_cnt, const double* __restrict__ wall,
    double* __restrict__ xall, const double* __restrict__ Hall, const double* __restrict__ lbimg, const double* __restrict__ lfK,
    const double* __restrict__ lfS, int s0) {
    leaf_back_batch_body<B>(blockIdx.x, blockIdx.y, M, nodes, b, active, S_cnt, wall, xall, Hall, lbimg, lfK, lfS, s0);
}

template <int B>
int launch_leaf_back_batch(hpf_handle* h, const LaunchCtx& ctx, const int* nodes, int count) {
    const dim3 grid((unsigned)count, (unsigned)((ctx.S + LB_SB - 1) / LB_SB));
    hipLaunchKernelGGL((k_leaf_back_batch<B>), grid, dim3(256), 0, ctx.stream, h->M, nodes, 2 * h->Hn, ctx.active, ctx.S, h->d_w,
                       h->d_x, h->d_H, active_tree(h).d_lbimg, h->d_lfK, h->d_lfS, ctx.s0);
    return launch_status(h);
}

// Back sweep of the super-leaves, 16 scenarios per workgroup:  x_k = w_k - S_k^-1 M_k^-1 (Wd^-1 t),  t = A(k,parent) x_parent,
//     M_k^-1 v = [0 0; 0 Ahh_k^-1] v + Pb (T^-1 (Qb v)),
// the Ahh_k^-1 part on the matrix cores (per-model image in A-operand layout), the m <= 10 border unknowns per thread; T^-1 and
// W_k^-1 were left by the factor kernel at the head of the bus's (otherwise unused) inverse slot.
// nodes: records of 8 ints (bus, parent, slot in Tree::d_sbimg, offset of [Tc | Pb | Qb] in Tree::d_lzimg, m, 0, 0, 0).
template <int B>
__device__ __forceinline__ BatchBus sleaf_back_bus(const int4 r0, const int4 r1, int pslot, int oslot, int b, const double* __restrict__ sbimg,
                                                   const double* __restrict__ lzimg) {
    const int m = r1.x;
    const double* pbm = lzimg + (size_t)r0.w + m * m;           // Pb [b][m]
    return BatchBus{0, r0.x, r0.y, m, pslot, oslot, sbimg + (size_t)r0.z * SleafImg<B>::SZ, pbm + (size_t)b * m};
}

// every operand whose address comes from the record alone is requested in one round trip with A(k,parent) and x_parent (the early ones, and
// W_k^-1 here): the Pb column of the lane's MFMAs, the thread's row of T^-1, S^-1 and w of its harmonics
template <int B>
__device__ __forceinline__ void sleaf_back_load_wi(BatchBackIn<B>& I, const BatchBus& U, const BatchLane& L, const Model& M, const double* __restrict__ Zall) {
    constexpr int NT = (B + 16) / 16;
    constexpr size_t CT = (size_t)NT * NT * 256;
    const double* tk = Zall + ((size_t)L.s * M.n + U.k) * CT;   // T^-1 [10][10] | W_k^-1 [4]
    I.wi[0] = I.wi[1] = I.wi[2] = I.wi[3] = 0.0;
    if (L.live && L.l16 == 0) {                                 // (harmonic 0 belongs to this thread)
        I.wi[0] = tk[100]; I.wi[1] = tk[101]; I.wi[2] = tk[102]; I.wi[3] = tk[103];
    }
}

template <int B>
__device__ __forceinline__ void sleaf_back_load_late(BatchBackIn<B>& I, const BatchBus& U, const BatchLane& L, const Model& M,
                                                     const double* __restrict__ wall, const double* __restrict__ Zall, const double* __restrict__ lfS) {
    constexpr int NT = (B + 16) / 16;
    constexpr size_t CT = (size_t)NT * NT * 256;
    constexpr int NTR = SleafImg<B>::NTR, KP = SleafImg<B>::KP, H2 = B / 2, QI = (H2 + 15) / 16;
    const int k = U.k, m = U.m, n = M.n, Hn = M.Hn, s = L.s, l16 = L.l16;
    const bool live = L.live;
    const double* tk = Zall + ((size_t)s * n + k) * CT;
#pragma unroll
    for (int j = 0; j < 10; ++j) I.tr[j] = (live && l16 < m && j < m) ? tk[l16 * 10 + j] : 0.0;
    if (L.wv < NTR) {
#pragma unroll
        for (int kp = 0; kp < KP; ++kp) I.pa[kp] = U.img[SleafImg<B>::MAIN + ((size_t)L.wv * KP + kp) * 64 + L.lane];
    }
#pragma unroll
    for (int it = 0; it < QI; ++it) {
        const int q = l16 + 16 * it;
        I.w4[it][0] = I.w4[it][1] = 0.0;
        I.si4[it][0] = I.si4[it][3] = 1.0;
        I.si4[it][1] = I.si4[it][2] = 0.0;
        if (live && q < H2) {
            if (q < Hn) {
                const double2* sp = reinterpret_cast<const double2*>(lfS + (((size_t)s * n + k) * Hn + q) * 4);
                const double2 a = sp[0], c2 = sp[1];
                I.si4[it][0] = a.x; I.si4[it][1] = a.y; I.si4[it][2] = c2.x; I.si4[it][3] = c2.y;
            }
            const double2 w2 = *reinterpret_cast<const double2*>(wall + ((size_t)s * n + k) * B + 2 * q);
            I.w4[it][0] = w2.x;
            I.w4[it][1] = w2.y;
        }
    }
}

// Compute part, first half (the early operands are free after it): returns the accumulators of V.  TT: v = Wd^-1 t, [row][scenario];
// RR: r = Qb v, [border unknown][scenario] (16 * LBP)
template <int B>
__device__ __forceinline__ d4_t sleaf_back_compute_a(const BatchBackIn<B>& I, const BatchBus& U, const BatchLane& L, const Model& M, int b,
                                                     const double* xall, double* __restrict__ TT, double* __restrict__ RR, const double2* XS) {
    constexpr int NTR = SleafImg<B>::NTR, KS = SleafImg<B>::KS;
    constexpr bool QBR = SleafImg<B>::QB_ROWS;
    const int m = U.m, lg = L.lg, jj = L.jj, wv = L.wv, sc = L.sc, l16 = L.l16;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int q = l16 + 16 * j;
        double t0 = 0.0, t1 = 0.0;
        if (L.live && q < M.Hn) {
            batch_back_t<B>(I, U, L, M, xall, XS, j, t0, t1);
            if (q == 0) {                                       // power rows of a linear bus arrive in polar form: W_k^-1 (identity otherwise)
                const double a = t0, c2 = t1;
                t0 = fma(I.wi[1], c2, I.wi[0] * a);
                t1 = fma(I.wi[3], c2, I.wi[2] * a);
            }
        }
        TT[(2 * q) * LBP + sc] = t0;
        TT[(2 * q + 1) * LBP + sc] = t1;
    }
    __syncthreads();
    d4_t acc = {0.0, 0.0, 0.0, 0.0};
    if (wv < NTR) {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const double bop = TT[(4 * ks + lg) * LBP + jj];
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(I.ia[ks], bop, acc, 0, 0, 0);
        }
        if (QBR && wv == NTR - 1) {                             // rows B.. of the last row tile: r = Qb v
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int j = 16 * (NTR - 1) + 4 * reg + lg - B;
                if (j >= 0 && j < 16) RR[j * LBP + jj] = acc[reg];
            }
        }
    }
    if (!QBR) {
        double r = 0.0;                                         // r_j = Qb[j][:] v   (thread (scenario, j))
        if (l16 < m) {
            const double* qr = U.qbm + (size_t)l16 * b;
            for (int col = 0; col < b; ++col) r = fma(qr[col], TT[col * LBP + sc], r);
        }
        RR[l16 * LBP + sc] = r;
    }
    return acc;
}

// ... second half.  V [64 * LBP]; YY: y = T^-1 r (16 * LBP); XS: k_back_tail's store of x (slot U.oslot takes the thread's harmonics besides HBM)
template <int B>
__device__ __forceinline__ void sleaf_back_compute_b(const BatchBackIn<B>& I, const BatchBus& U, const BatchLane& L, const Model& M, d4_t acc, double* xall,
                                                     double* __restrict__ V, const double* __restrict__ RR, double* __restrict__ YY, double2* XS) {
    constexpr int NTR = SleafImg<B>::NTR, KP = SleafImg<B>::KP, H2 = B / 2, QI = (H2 + 15) / 16;
    const int k = U.k, m = U.m, lg = L.lg, jj = L.jj, wv = L.wv, sc = L.sc, l16 = L.l16;
    const bool live = L.live;
    double* xs = xall + (size_t)L.s * M.n * B;
    __syncthreads();
    {
        double y = 0.0;                                         // y_i = T^-1[i][:] r
#pragma unroll
        for (int j = 0; j < 10; ++j) y = fma(I.tr[j], (j < m ? RR[j * LBP + sc] : 0.0), y);
        YY[l16 * LBP + sc] = (live && l16 < m) ? y : 0.0;
    }
    __syncthreads();
    if (wv < NTR) {                                             // V = [0 0; 0 Ahh^-1] v + Pb y
#pragma unroll
        for (int kp = 0; kp < KP; ++kp) {
            const double bop = YY[(4 * kp + lg) * LBP + jj];
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(I.pa[kp], bop, acc, 0, 0, 0);
        }
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) V[(16 * wv + 4 * reg + lg) * LBP + jj] = acc[reg];
    }
    __syncthreads();
    if (live) {
#pragma unroll
        for (int it = 0; it < QI; ++it) {
            const int q = l16 + 16 * it;
            if (q >= H2) continue;
            const double x0 = V[(2 * q) * LBP + sc], x1 = V[(2 * q + 1) * LBP + sc];
            const double d0 = fma(I.si4[it][1], x1, I.si4[it][0] * x0), d1 = fma(I.si4[it][3], x1, I.si4[it][2] * x0);
            const double2 x2 = double2{I.w4[it][0] - d0, I.w4[it][1] - d1};
            *reinterpret_cast<double2*>(xs + (size_t)k * B + 2 * q) = x2;
            if (XS && U.oslot >= 0) XS[((size_t)U.oslot * QI + it) * 256 + L.tid] = x2;
        }
    }
}

template <int B>
__device__ __forceinline__ void sleaf_back_batch_body(
    const int bx_, const int by_, const Model& M, const int* __restrict__ nodes, int b, const int* __restrict__ active, int S_cnt, const double* __restrict__ wall,
    double* __restrict__ xall, const double* __restrict__ Hall, const double* __restrict__ sbimg, const double* __restrict__ lzimg,
    const double* __restrict__ Zall, const double* __restrict__ lfS, int s0) {
    __shared__ double TT[64 * LBP];                           // v = Wd^-1 t, [row][scenario]
    __shared__ double V[64 * LBP];
    __shared__ double RR[16 * LBP];                           // r = Qb v, then y = T^-1 r, [border unknown][scenario]
    __shared__ double YY[16 * LBP];
    const int4* rec = reinterpret_cast<const int4*>(nodes) + 2 * (size_t)bx_;
    const BatchLane L = batch_lane(by_, active, S_cnt, s0);
    const BatchBus U = sleaf_back_bus<B>(rec[0], rec[1], -1, -1, b, sbimg, lzimg);
    BatchBackIn<B> I;
    batch_back_load_early<B>(I, U, L, M, xall, Hall);
    sleaf_back_load_wi<B>(I, U, L, M, Zall);
    sleaf_back_load_late<B>(I, U, L, M, wall, Zall, lfS);
    const d4_t acc = sleaf_back_compute_a<B>(I, U, L, M, b, xall, TT, RR, nullptr);
    sleaf_back_compute_b<B>(I, U, L, M, acc, xall, V, RR, YY, nullptr);
}

template <int B>
__global__ __launch_bounds__(256) void k_sleaf_back_batch(
    Model M, const int* __restrict__ nodes, int b, const int* __restrict__ active, int S_cnt, const double* __restrict__ wall,
    double* __restrict__ xall, const double* __restrict__ Hall, const double* __restrict__ sbimg, const double* __restrict__ lzimg,
    const double* __restrict__ Zall, const double* __restrict__ lfS, int s0) {
    sleaf_back_batch_body<B>(blockIdx.x, blockIdx.y, M, nodes, b, active, S_cnt, wall, xall, Hall, sbimg, lzimg, Zall, lfS, s0);
}

template <int B>
int launch_sleaf_back_batch(hpf_handle* h, const LaunchCtx& ctx, const int* nodes, int count) {
    const dim3 grid((unsigned)count, (unsigned)((ctx.S + LB_SB - 1) / LB_SB));
    hipLaunchKernelGGL((k_sleaf_back_batch<B>), grid, dim3(256), 0, ctx.stream, h->M, nodes, 2 * h->Hn, ctx.active, ctx.S, h->d_w,
                       h->d_x, h->d_H, active_tree(h).d_sbimg, active_tree(h).d_lzimg, h->d_Z, h->d_lfS, ctx.s0);
    return launch_status(h);
}

// Back-sweep tail (HPF_BACKTAIL): every bordered bus and constant-inverse leaf of the batched back sweep in ONE launch -- one workgroup per
// (family, 16 scenarios) walks the family's members (Tree::tail_*: a bordered bus under a Gauss-Jordan bus, its nested bordered buses, the
// leaves of any of them; a leaf under a Gauss-Jordan bus alone), each after its parent, with the arithmetic of the two bodies above.  The x of a
// member with children goes to an LDS slot besides HBM, and its children take x_parent from there instead of waiting for a launch boundary
// and a round trip; each half of the next member's operands is requested as soon as the current member has used its own (BatchBackIn).
// A thread reads back from the store exactly the entries it wrote itself (harmonics l16, l16 + 16 of scenario sc), as it would from HBM: the
// store needs no barrier of its own, and the four work arrays are used as in the bodies, whose barriers keep a member's phases apart -- the
// first write of the next member (TT) follows the last barrier of the current one, which nothing reads TT behind.
// recs: [member][4] kind (0 bordered bus, 1 leaf), index of its record in sl_nodes / lf_nodes, slot of x_parent, own slot.
constexpr int BACK_TAIL_WORK = 2 * 64 * LBP + 2 * 16 * LBP + LB_SB * 2;       // doubles: TT | V | RR | YY | UK

template <int B>
constexpr int back_tail_lds_bytes() { return 8 * BACK_TAIL_WORK + TAIL_SLOTS * BatchBackIn<B>::QI * 256 * 16; }

template <int B>
__device__ __forceinline__ BatchBus back_tail_bus(const int4 t, const int* __restrict__ sl_nodes, const int* __restrict__ lf_nodes, int b,
                                                  const double* __restrict__ sbimg, const double* __restrict__ lzimg, const double* __restrict__ lbimg) {
    if (t.x == 0) {
        const int4* rec = reinterpret_cast<const int4*>(sl_nodes) + 2 * (size_t)t.y;
        return sleaf_back_bus<B>(rec[0], rec[1], t.z, t.w, b, sbimg, lzimg);
    }
    return leaf_back_bus<B>(reinterpret_cast<const int4*>(lf_nodes)[t.y], t.z, t.w, lbimg);
}

template <int B>
__global__ __launch_bounds__(256) void k_back_tail(
    Model M, const int* __restrict__ fam_ptr, const int* __restrict__ recs, const int* __restrict__ sl_nodes, const int* __restrict__ lf_nodes, int b,
    const int* __restrict__ active, int S_cnt, const double* __restrict__ wall, double* xall, const double* __restrict__ Hall,
    const double* __restrict__ sbimg, const double* __restrict__ lzimg, const double* __restrict__ lbimg, const double* __restrict__ Zall,
    const double* __restrict__ lfK, const double* __restrict__ lfS, int s0) {
    __shared__ __attribute__((aligned(16))) double smem[back_tail_lds_bytes<B>() / 8];
    double* TT = smem;
    double* V = TT + 64 * LBP;
    double* RR = V + 64 * LBP;
    double* YY = RR + 16 * LBP;
    double* UK = YY + 16 * LBP;
    double2* XS = reinterpret_cast<double2*>(UK + LB_SB * 2);
    const int beg = fam_ptr[blockIdx.x], end = fam_ptr[blockIdx.x + 1];
    if (beg >= end) return;
    const BatchLane L = batch_lane(blockIdx.y, active, S_cnt, s0);
    const int4* tr = reinterpret_cast<const int4*>(recs);
    BatchBus cur = back_tail_bus<B>(tr[beg], sl_nodes, lf_nodes, b, sbimg, lzimg, lbimg), nxt = cur;
    BatchBackIn<B> I;
    batch_back_load_early<B>(I, cur, L, M, xall, Hall);
    if (cur.kind == 0) {
        sleaf_back_load_wi<B>(I, cur, L, M, Zall);
        sleaf_back_load_late<B>(I, cur, L, M, wall, Zall, lfS);
    } else {
        leaf_back_load_late<B>(I, cur, L, M, wall, lfK, lfS);
    }
    for (int i = beg; i < end; ++i) {
        const bool more = i + 1 < end;
        if (more) nxt = back_tail_bus<B>(tr[i + 1], sl_nodes, lf_nodes, b, sbimg, lzimg, lbimg);
        d4_t acc = {0.0, 0.0, 0.0, 0.0};
        if (cur.kind == 0) acc = sleaf_back_compute_a<B>(I, cur, L, M, b, xall, TT, RR, XS);
        else leaf_back_compute_a<B>(I, cur, L, M, xall, TT, V, XS);
        if (more) {
            batch_back_load_early<B>(I, nxt, L, M, xall, Hall);
            if (nxt.kind == 0) sleaf_back_load_wi<B>(I, nxt, L, M, Zall);
        }
        if (cur.kind == 0) sleaf_back_compute_b<B>(I, cur, L, M, acc, xall, V, RR, YY, XS);
        else leaf_back_compute_b<B>(I, cur, L, M, xall, TT, V, UK);
        if (more) {
            if (nxt.kind == 0) sleaf_back_load_late<B>(I, nxt, L, M, wall, Zall, lfS);
            else leaf_back_load_late<B>(I, nxt, L, M, wall, lfK, lfS);
        }
        cur = nxt;
    }
}

template <int B>
int launch_back_tail(hpf_handle* h, const LaunchCtx& ctx, const Tree& tr) {
    const dim3 grid((unsigned)tr.n_tail_fam, (unsigned)((ctx.S + LB_SB - 1) / LB_SB));
    hipLaunchKernelGGL((k_back_tail<B>), grid, dim3(256), 0, ctx.stream, h->M, tr.d_tail_ptr, tr.d_tail_rec, tr.d_bsleaf, tr.d_bleaf, 2 * h->Hn,
                       ctx.active, ctx.S, h->d_w, h->d_x, h->d_H, tr.d_sbimg, tr.d_lzimg, tr.d_lbimg, h->d_Z, h->d_lfK, h->d_lfS, ctx.s0);
    return launch_status(h);
}

// Factor sweep of the super-leaves whose parent rebuilds their Schur complement (HPF_SLLAZY), 16 scenarios per workgroup: such a
// bus owes the sweep vectors only -- w = S^-1 M^-1 Wd^-1 y, G w, T^-1 (+ W^-1), S^-1, A(k,parent), its position-0 borders.
// Roles as in k_leaf_batch (plus the power-row diagonal of a linear bus and the G w of its lazy leaves), T assembled and inverted
// per scenario by the scenario's 16 threads (thread r owns row r; the pivot row goes through LDS), the Ahh^-1 part on the matrix
// cores.  nodes: Tree::d_fdesc records (int 39: slot of the bus's image in Tree::d_sbimg).
constexpr int SLEAF_BATCH_LDS = 2 * 64 * LBP + LB_SB * 100 + LB_SB * 10 + 3 * LB_SB * 4 + 2 * 16 * LBP;      // doubles

template <int B, int SB>
__device__ __forceinline__ void sleaf_batch_body(
    double* __restrict__ smem_, const int bx_, const int by_, const Model& M, const TreeDev& T, const int* __restrict__ nodes, int b, const int* __restrict__ active, int S_cnt,
    const cplx* __restrict__ Uall, const cplx* __restrict__ Eall, const double* __restrict__ fall, double* __restrict__ wall,
    const double* __restrict__ linAall, double* __restrict__ Call, double* __restrict__ Hall, const cplx* __restrict__ I0all,
    const double* __restrict__ chG, const double* __restrict__ chH, const double* __restrict__ chD, const double* __restrict__ chy,
    const double* __restrict__ sbimg, double* __restrict__ Zall, double* __restrict__ lfK, double* __restrict__ lfS, int s0,
    long long* __restrict__ dbg, int ablate) {
#ifdef HPF_FACTOR_STAMPS
    long long tq[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#define HPF_SLSTAMP(i) if (ablate & 16) tq[i] = __builtin_amdgcn_s_memtime()
#else
#define HPF_SLSTAMP(i)
#endif
    HPF_SLSTAMP(0);
    constexpr int NT = (B + 16) / 16;
    constexpr size_t CT = (size_t)NT * NT * 256;
    using TL = BatchTile<SB>;                                    // role mapping: TL::TPS threads per scenario (hpf_batch_tile.hpp)
    constexpr int RPT = TL::ROWS;
    constexpr int NTR = SleafImg<B>::NTR, KS = SleafImg<B>::KS, KP = SleafImg<B>::KP, H2 = B / 2, QI = TL::harmonics(H2);
    constexpr bool QBR = SleafImg<B>::QB_ROWS;
    const int4* nd = reinterpret_cast<const int4*>(nodes) + (FDESC / 4) * (size_t)bx_;
    const int4 nd0 = nd[0], nd1 = nd[1], nd3 = nd[3], lzA = nd[7], lzB = nd[8], lzC = nd[9];
    const int k = nd0.x, par = nd0.y, diag_e = nd0.z;
    const int e_dn_k = nd1.x, e_up_k = nd1.y, lin_beg = nd1.z, lin_end = nd1.z + nd1.w;
    const bool via_chain = (nd3.z & 1) != 0;
    // nested bordered children (at most two): bus, border unknowns; their T (not inverted) sits on this bus's diagonal
    const int L = lzA.y, cs0 = lzC.x, cs1 = lzC.y, mc0 = lzC.z & 0xff, mc1 = (lzC.z >> 8) & 0xff;
    const int m = 2 + 2 * L + mc0 + mc1;
    const double* simg = T.lzimg + (size_t)lzB.w;                // Tc [m][m] | Pb [b][m] | Qb [m][b]
    const double* pbm = simg + m * m;
    const double* qbm = pbm + (size_t)b * m;
    const double* img = sbimg + (size_t)lzC.w * SleafImg<B>::SZ;   // [0 0; 0 Ahh^-1] (+ the rows of Qb), A-operand layout | Pb as an A operand
    const int tid = threadIdx.x, lane = tid & 63, lg = lane >> 4, jj = lane & 15;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = M.n, c = M.c, Hn = M.Hn;
    const int sc = TL::scenario(tid), lt = TL::lane(tid);
    const int sl = by_ * SB + sc;
    const int ss = sl < S_cnt ? (active ? active[sl + s0] : sl + s0) : -1;      // slot -> scenario (active list; -1: frozen / empty slot)
    const bool live = ss >= 0;
    const int s = live ? ss : 0;
    const size_t so = (size_t)s * n * Hn;
    const cplx* U = Uall + so;
    const cplx* E = Eall + so;
    const double* Cs = Call + (size_t)s * n * CT;
    const bool linear_k = k < M.m;

    double* Y = smem_;                                           // v = Wd^-1 y, [row][scenario]
    double* V = Y + 64 * LBP;
    double* AUG = V + 64 * LBP;                                // T, then T^-1, per scenario [10][10]
    double* PR = AUG + LB_SB * 100;                              // pivot row of the step
    double* DL = PR + LB_SB * 10;
    double* S0 = DL + LB_SB * 4;
    double* WI = S0 + LB_SB * 4;
    double* RR = WI + LB_SB * 4;
    double* YY = RR + 16 * LBP;

    // ---- R1. rows --------------------------------------------------------------------------------------------------------------
    {
        double e0[RPT] = {}, e1[RPT] = {}, ey[RPT] = {};
        double a0[RPT] = {}, a1[RPT] = {}, ay[RPT] = {}, fy[RPT] = {};
        bool ok[RPT];
        cplx ukr[RPT], ekr[RPT];
#pragma unroll
        for (int pz = 0; pz < RPT; ++pz) {
            const int row = TL::row(tid, pz), q = row >> 1, tr_ = row & 1;
            ok[pz] = live && row < b && loc_valid(n, c, k, row);
            ukr[pz] = cplx{0.0, 0.0};
            ekr[pz] = cplx{0.0, 0.0};
            if (ok[pz]) {
                const size_t kq = (size_t)k * Hn + q;
                fy[pz] = fall[((size_t)s * n + k) * B + row];
                if (via_chain) {
                    const size_t o = so + kq;
                    a0[pz] = chD[o * 4 + 2 * tr_];
                    a1[pz] = chD[o * 4 + 2 * tr_ + 1];
                    ay[pz] = chy[o * 2 + tr_];
                }
                ukr[pz] = U[kq];
                ekr[pz] = E[kq];
                // G w of the lazy leaves: y -= sum
                const double g0 = lzA.z >= 0 ? Cs[(size_t)lzA.z * CT + row] : 0.0, g1 = lzA.w >= 0 ? Cs[(size_t)lzA.w * CT + row] : 0.0;
                const double g2 = lzB.x >= 0 ? Cs[(size_t)lzB.x * CT + row] : 0.0, g3 = lzB.y >= 0 ? Cs[(size_t)lzB.y * CT + row] : 0.0;
                ay[pz] -= (g0 + g1) + (g2 + g3);
                const double g4 = cs0 >= 0 ? Cs[(size_t)cs0 * CT + row] : 0.0, g5 = cs1 >= 0 ? Cs[(size_t)cs1 * CT + row] : 0.0;
                ay[pz] -= g4 + g5;                                   // ... and of the bordered children
                if (row < 2 && linear_k) {                           // power rows: the state-dependent diagonal of the fundamental
                    const Blk2 blk = blk_power_diag(M.Y[(size_t)diag_e * Hn], ukr[pz], ekr[pz], I0all[(size_t)s * n + k]);
                    a0[pz] += pick(blk, tr_, 0);
                    a1[pz] += pick(blk, tr_, 1);
                }
            }
        }
        const double* ws = wall + (size_t)s * n * B;
        const double* linA = linAall + so * 4;
        const int4* c3 = reinterpret_cast<const int4*>(T.child3);
        for (int cp = lin_beg; cp < lin_end; ++cp) {
            const int4 cr = c3[cp];
            const int ch = cr.x;
#pragma unroll
            for (int pz = 0; pz < RPT; ++pz) {
                if (!ok[pz]) continue;
                const int row = TL::row(tid, pz), q = row >> 1, tr_ = row & 1;
                const cplx uk = ukr[pz], ek = ekr[pz];
                const cplx ydn = M.Y[(size_t)cr.y * Hn + q], yup = M.Y[(size_t)cr.z * Hn + q];
                const cplx uc = U[(size_t)ch * Hn + q], ec = E[(size_t)ch * Hn + q];
                const double2* pic = reinterpret_cast<const double2*>(linA + ((size_t)ch * Hn + q) * 4);
                const double2 ic01 = pic[0], ic23 = pic[1];
                const double2 wc = *reinterpret_cast<const double2*>(ws + (size_t)ch * B + 2 * q);
                const Blk2 g = (q == 0 && k < M.m) ? blk_power_off(ydn, uk, uc, ec) : blk_current(ydn, uc, ec);
                const Blk2 hb = (q == 0 && ch < M.m) ? blk_power_off(yup, uc, uk, ek) : blk_current(yup, uk, ek);
                const double g0 = pick(g, tr_, 0);
                const double g1 = loc_valid(n, c, ch, 2 * q + 1) ? pick(g, tr_, 1) : 0.0;
                double h4[4];
                mask_block(n, c, q, ch, k, hb, h4);
                const double v0 = fma(g1, ic23.x, g0 * ic01.x), v1 = fma(g1, ic23.y, g0 * ic01.y);
                e0[pz] += fma(v1, h4[2], v0 * h4[0]);
                e1[pz] += fma(v1, h4[3], v0 * h4[1]);
                ey[pz] = fma(g0, wc.x, ey[pz]);
                ey[pz] = fma(g1, wc.y, ey[pz]);
            }
        }
#pragma unroll
        for (int pz = 0; pz < RPT; ++pz) {
            const int row = TL::row(tid, pz);
            Y[row * LBP + sc] = ok[pz] ? fy[pz] + ay[pz] - ey[pz] : 0.0;
            if (SB < BATCH_COLS) Y[row * LBP + SB + sc] = 0.0;          // (the B-operand columns behind the tile)
            if (row < 2) {
                DL[sc * 4 + row * 2] = ok[pz] ? a0[pz] - e0[pz] : 0.0;
                DL[sc * 4 + row * 2 + 1] = ok[pz] ? a1[pz] - e1[pz] : 0.0;
            }
        }
    }
    HPF_SLSTAMP(1);
    // ---- R2. harmonics ---------------------------------------------------------------------------------------------------------
    double sir[QI][4], glr[QI][4];
#pragma unroll
    for (int it = 0; it < QI; ++it) {
        const int q = TL::harmonic(tid, it);
        double si[4] = {1.0, 0.0, 0.0, 1.0}, g4[4] = {0.0, 0.0, 0.0, 0.0}, h4[4] = {0.0, 0.0, 0.0, 0.0};
        if (live && q < Hn) {
            const cplx uk = U[(size_t)k * Hn + q], ek = E[(size_t)k * Hn + q];
            const double idet = 1.0 / (-(uk.im * ek.im) - ek.re * uk.re);
            si[0] = ek.im * idet;   si[1] = -ek.re * idet;
            si[2] = -uk.re * idet;  si[3] = -uk.im * idet;
            cplx up = {0.0, -1.0}, ep = {0.0, 1.0};
            if (!via_chain || q == 0) {
                up = U[(size_t)par * Hn + q];
                ep = E[(size_t)par * Hn + q];
            }
            if (via_chain) {
                const double2* pg = reinterpret_cast<const double2*>(chG + (so + (size_t)k * Hn + q) * 4);
                const double2* ph = reinterpret_cast<const double2*>(chH + (so + (size_t)k * Hn + q) * 4);
                const double2 ga = pg[0], gb = pg[1], ha = ph[0], hb = ph[1];
                g4[0] = ga.x; g4[1] = ga.y; g4[2] = gb.x; g4[3] = gb.y;
                h4[0] = ha.x; h4[1] = ha.y; h4[2] = hb.x; h4[3] = hb.y;
            } else {
                const cplx ydn = M.Y[(size_t)e_dn_k * Hn + q], yup = M.Y[(size_t)e_up_k * Hn + q];
                const Blk2 g = (q == 0 && par < M.m) ? blk_power_off(ydn, up, uk, ek) : blk_current(ydn, uk, ek);
                const Blk2 hh = (q == 0 && k < M.m) ? blk_power_off(yup, uk, up, ep) : blk_current(yup, up, ep);
                mask_block(n, c, q, par, k, g, g4);
                mask_block(n, c, q, k, par, hh, h4);
            }
            double* Hk = Hall + ((size_t)s * n + k) * Hn * 4 + q * 4;
            double* Sk = lfS + (so + (size_t)k * Hn + q) * 4;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                Hk[e] = h4[e];
                Sk[e] = si[e];
            }
            if (q == 0) {
                const double ip = 1.0 / (-(up.im * ep.im) - ep.re * up.re);
                const double sp0 = ep.im * ip, sp1 = -ep.re * ip, sp2 = -up.re * ip, sp3 = -up.im * ip;
                double* kk = lfK + ((size_t)s * n + k) * 12 + 4;
                kk[0] = fma(g4[1], si[2], g4[0] * si[0]);  kk[1] = fma(g4[1], si[3], g4[0] * si[1]);
                kk[2] = fma(g4[3], si[2], g4[2] * si[0]);  kk[3] = fma(g4[3], si[3], g4[2] * si[1]);
                kk[4] = fma(h4[1], sp2, h4[0] * sp0);  kk[5] = fma(h4[1], sp3, h4[0] * sp1);
                kk[6] = fma(h4[3], sp2, h4[2] * sp0);  kk[7] = fma(h4[3], sp3, h4[2] * sp1);
                double w00 = 1.0, w01 = 0.0, w10 = 0.0, w11 = 1.0;      // W_k^-1 = W_k / |U|^2 for a linear bus
                if (linear_k) {
                    const double iu = 1.0 / fma(uk.re, uk.re, uk.im * uk.im);
                    w00 = uk.re * iu; w01 = uk.im * iu; w10 = w01; w11 = -w00;
                }
                WI[sc * 4] = w00; WI[sc * 4 + 1] = w01; WI[sc * 4 + 2] = w10; WI[sc * 4 + 3] = w11;
                double* tk = Zall + ((size_t)s * n + k) * CT + 100;
                tk[0] = w00; tk[1] = w01; tk[2] = w10; tk[3] = w11;
            }
        }
        if (q == 0) {
#pragma unroll
            for (int e = 0; e < 4; ++e) S0[sc * 4 + e] = si[e];
            if (!(live && q < Hn)) { WI[sc * 4] = 1.0; WI[sc * 4 + 1] = 0.0; WI[sc * 4 + 2] = 0.0; WI[sc * 4 + 3] = 1.0; }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            sir[it][e] = si[e];
            glr[it][e] = g4[e];
        }
    }
    // T <- Tc (per scenario copy), rows by the scenario's threads
    if (lt < m)
        for (int c2 = 0; c2 < m; ++c2) AUG[sc * 100 + lt * 10 + c2] = simg[lt * m + c2];
    HPF_SLSTAMP(2);
    __syncthreads();
    HPF_SLSTAMP(3);
    // ---- T. per-scenario parts of T (as in k_factor_q's super-leaf branch), v = Wd^-1 y -----------------------------------------
    {
        double* aug = AUG + sc * 100;
        const double* wi = WI + sc * 4;
        if (lt == 0) {
            const double* si = S0 + sc * 4;
            const double* dl = DL + sc * 4;
            const double e00 = fma(dl[1], si[2], dl[0] * si[0]), e01 = fma(dl[1], si[3], dl[0] * si[1]);
            const double e10 = fma(dl[3], si[2], dl[2] * si[0]), e11 = fma(dl[3], si[3], dl[2] * si[1]);
            aug[0] += fma(wi[1], e10, wi[0] * e00);
            aug[1] += fma(wi[1], e11, wi[0] * e01);
            aug[10] += fma(wi[3], e10, wi[2] * e00);
            aug[11] += fma(wi[3], e11, wi[2] * e01);
            const double y0 = Y[sc], y1 = Y[LBP + sc];                  // right-hand side rows 0 / 1: W_k^-1
            Y[sc] = fma(wi[1], y1, wi[0] * y0);
            Y[LBP + sc] = fma(wi[3], y1, wi[2] * y0);
        } else if (lt <= L && live) {
            const int i = lt - 1, bc = 2 + 2 * i;
            const int leaf = i == 0 ? lzA.z : (i == 1 ? lzA.w : (i == 2 ? lzB.x : lzB.y));
            const double* kk = lfK + ((size_t)s * n + leaf) * 12;
            double q00, q01, q10, q11;
            inv2(kk[0], kk[1], kk[2], kk[3], q00, q01, q10, q11);
            aug[bc * 10 + bc] += q00;
            aug[bc * 10 + bc + 1] += q01;
            aug[(bc + 1) * 10 + bc] += q10;
            aug[(bc + 1) * 10 + bc + 1] += q11;
            aug[bc] -= fma(wi[1], kk[6], wi[0] * kk[4]);
            aug[bc + 1] -= fma(wi[1], kk[7], wi[0] * kk[5]);
            aug[10 + bc] -= fma(wi[3], kk[6], wi[2] * kk[4]);
            aug[10 + bc + 1] -= fma(wi[3], kk[7], wi[2] * kk[5]);
            aug[bc * 10] -= kk[8];
            aug[bc * 10 + 1] -= kk[9];
            aug[(bc + 1) * 10] -= kk[10];
            aug[(bc + 1) * 10 + 1] -= kk[11];
        } else if (live && lt - L - 1 < (cs0 >= 0) + (cs1 >= 0)) {
            // bordered child: its T_c in the place of K_c^-1; of its border columns only the first (the child's own position 0)
            // reaches position 0 here: -W_k^-1 (G0 S_c^-1) above, -W_c^-1 (H0 S_k^-1) on the left
            const int zc = lt - L - 1;
            const int cb = zc == 0 ? cs0 : cs1, mc = zc == 0 ? mc0 : mc1, bc = 2 + 2 * L + (zc ? mc0 : 0);
            const double* tcd = Zall + ((size_t)s * n + cb) * CT;     // T_c^-1 [10][10] | W_c^-1 [4] | T_c [10][10]
            const double* kk = lfK + ((size_t)s * n + cb) * 12;
            for (int i = 0; i < mc; ++i)
                for (int j = 0; j < mc; ++j) aug[(bc + i) * 10 + bc + j] += tcd[104 + i * 10 + j];
            aug[bc] -= fma(wi[1], kk[6], wi[0] * kk[4]);
            aug[bc + 1] -= fma(wi[1], kk[7], wi[0] * kk[5]);
            aug[10 + bc] -= fma(wi[3], kk[6], wi[2] * kk[4]);
            aug[10 + bc + 1] -= fma(wi[3], kk[7], wi[2] * kk[5]);
            const double* wc = tcd + 100;
            aug[bc * 10] -= fma(wc[1], kk[10], wc[0] * kk[8]);
            aug[bc * 10 + 1] -= fma(wc[1], kk[11], wc[0] * kk[9]);
            aug[(bc + 1) * 10] -= fma(wc[3], kk[10], wc[2] * kk[8]);
            aug[(bc + 1) * 10 + 1] -= fma(wc[3], kk[11], wc[2] * kk[9]);
        }
    }
    __syncthreads();
    HPF_SLSTAMP(4);
    // ---- I. in-place inversion with partial pivoting, one scenario per 16 threads (thread r = row r; pivot row through LDS).  With 32 threads
    //      per scenario the rows of T sit in its first 16 lanes, one DPP row: the upper 16 enter the reduction of their own DPP row as used
    //      (-1), never own a pivot (pi < 16 <= lt) and store nothing ------------------------------------------------------------------
    {
        double* aug = AUG + sc * 100;
        double* pr = PR + sc * 10;
        double row[10];
#pragma unroll
        for (int c2 = 0; c2 < 10; ++c2) row[c2] = (lt < m && c2 < m) ? aug[lt * 10 + c2] : 0.0;
        if (live && lt < m) {                                   // T itself for a bordered parent (behind T^-1 and W^-1)
            double* tk = Zall + ((size_t)s * n + k) * CT + 104 + lt * 10;
#pragma unroll
            for (int c2 = 0; c2 < 10; ++c2)
                if (c2 < m) tk[c2] = row[c2];
        }
        bool used = lt >= m;
        int mycol = 0, pcol[10];
#pragma unroll
        for (int j = 0; j < 10; ++j) {
            pcol[j] = 0;
            if (j < m) {
                const double cand = used ? -1.0 : fabs(row[j]);
                double mx = cand;
                mx = fmax(mx, dpp_f64<0xB1>(mx));
                mx = fmax(mx, dpp_f64<0x4E>(mx));
                mx = fmax(mx, dpp_f64<0x141>(mx));
                mx = fmax(mx, dpp_f64<0x140>(mx));
                const unsigned long long bal = __builtin_amdgcn_ballot_w64(!used && cand == mx);
                const unsigned grp = (unsigned)((bal >> (16 * lg)) & 0xffffull);
                const int pi = __builtin_ctz(grp | 0x8000u);
                const bool me = lt == pi;
                if (me) {
#pragma unroll
                    for (int c2 = 0; c2 < 10; ++c2) pr[c2] = row[c2];
                }
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                __builtin_amdgcn_wave_barrier();
                double prow[10];
#pragma unroll
                for (int c2 = 0; c2 < 10; ++c2) prow[c2] = pr[c2];
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                __builtin_amdgcn_wave_barrier();
                const double ipv = 1.0 / prow[j];
                const double f = me ? 0.0 : row[j] * ipv;
#pragma unroll
                for (int c2 = 0; c2 < 10; ++c2)
                    row[c2] = c2 == j ? (me ? ipv : -f) : (me ? prow[c2] * ipv : fma(-f, prow[c2], row[c2]));
                used = used || me;
                mycol = me ? j : mycol;
                pcol[j] = pi;
            }
        }
        if (lt < m) {
            double* tk = Zall + ((size_t)s * n + k) * CT;
#pragma unroll
            for (int c2 = 0; c2 < 10; ++c2)
                if (c2 < m) {
                    aug[mycol * 10 + pcol[c2]] = row[c2];
                    if (live) tk[mycol * 10 + pcol[c2]] = row[c2];
                }
        }
    }
    __syncthreads();
    HPF_SLSTAMP(5);
    // ---- M. V = [0 0; 0 Ahh^-1] v on the matrix cores; r = Qb v (rows B.. of the same MFMAs where they fit) ------------------------
    d4_t acc = {0.0, 0.0, 0.0, 0.0};
    if (wv < NTR) {
        const double* ia = img + (size_t)wv * KS * 64 + lane;
#pragma unroll 4
        for (int ks = 0; ks < KS; ++ks) {
            const double a = ia[(size_t)ks * 64];
            const double bop = Y[(4 * ks + lg) * LBP + jj];
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bop, acc, 0, 0, 0);
        }
        if (QBR && wv == NTR - 1) {
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int j = 16 * (NTR - 1) + 4 * reg + lg - B;
                if (j >= 0 && j < 16) RR[j * LBP + jj] = acc[reg];
            }
        }
    }
    if (!QBR && lt < 16) {
        double r = 0.0;
        if (lt < m) {
            const double* qr = qbm + (size_t)lt * b;
            for (int col = 0; col < b; ++col) r = fma(qr[col], Y[col * LBP + sc], r);
        }
        RR[lt * LBP + sc] = r;
    }
    __syncthreads();
    if (lt < 16) {
        double y = 0.0;
        if (lt < m) {
            const double* tr = AUG + sc * 100 + lt * 10;
            for (int j = 0; j < m; ++j) y = fma(tr[j], RR[j * LBP + sc], y);
        }
        YY[lt * LBP + sc] = y;
        if (SB < BATCH_COLS) YY[lt * LBP + SB + sc] = 0.0;
    }
    __syncthreads();
    if (wv < NTR) {                                              // ... + Pb y: three more rank-4 steps on the same accumulators
        const double* pa = img + SleafImg<B>::MAIN + (size_t)wv * KP * 64 + lane;
#pragma unroll
        for (int kp = 0; kp < KP; ++kp) {
            const double a = pa[(size_t)kp * 64];
            const double bop = YY[(4 * kp + lg) * LBP + jj];
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bop, acc, 0, 0, 0);
        }
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) V[(16 * wv + 4 * reg + lg) * LBP + jj] = acc[reg];
    }
    __syncthreads();
    HPF_SLSTAMP(6);
    // ---- F. x_rect = V + Pb y, w = S^-1 x_rect, G w --------------------------------------------------------------------------
    if (live) {
        double* wk = wall + ((size_t)s * n + k) * B;
        double* Ck = Call + ((size_t)s * n + k) * CT;
#pragma unroll
        for (int it = 0; it < QI; ++it) {
            const int q = TL::harmonic(tid, it);
            if (q >= H2) continue;
            const double x0 = V[(2 * q) * LBP + sc], x1 = V[(2 * q + 1) * LBP + sc];
            const double* si = sir[it];
            const bool in = 2 * q < b;
            const double w0 = in ? fma(si[1], x1, si[0] * x0) : 0.0, w1 = in ? fma(si[3], x1, si[2] * x0) : 0.0;
            const double* g = glr[it];
            wk[2 * q] = w0;
            wk[2 * q + 1] = w1;
            Ck[2 * q] = fma(g[1], w1, g[0] * w0);
            Ck[2 * q + 1] = fma(g[3], w1, g[2] * w0);
        }
    }
#ifdef HPF_FACTOR_STAMPS
    if ((ablate & 16) && dbg && live && lt == 0) {     // phases of this scenario's 16 threads (cycles): rows | harmonics | wait | T | inversion | MFMA + Qb v | T^-1 r | tail
        HPF_SLSTAMP(7);
        long long* o = dbg + ((size_t)s * n + k) * 8;
        o[0] = tq[1] - tq[0];
        o[1] = tq[2] - tq[1];
        o[2] = tq[3] - tq[2];
        o[3] = ((tq[4] - tq[3]) & 0xfffff) | (((tq[5] - tq[4]) & 0xfffff) << 20) | (((tq[6] - tq[5]) & 0xfffff) << 40);
        o[4] = tq[7] - tq[6];
        o[5] = tq[7] - tq[0];
        o[6] = 1000 + m;
        o[7] = (k >= M.m) | ((lin_end - lin_beg) << 1);
    }
#endif
#undef HPF_SLSTAMP
}

template <int B, int SB>
__global__ __launch_bounds__(256, 4) void k_sleaf_batch(
    Model M, TreeDev T, const int* __restrict__ nodes, int b, const int* __restrict__ active, int S_cnt,
    const cplx* __restrict__ Uall, const cplx* __restrict__ Eall, const double* __restrict__ fall, double* __restrict__ wall,
    const double* __restrict__ linAall, double* __restrict__ Call, double* __restrict__ Hall, const cplx* __restrict__ I0all,
    const double* __restrict__ chG, const double* __restrict__ chH, const double* __restrict__ chD, const double* __restrict__ chy,
    const double* __restrict__ sbimg, double* __restrict__ Zall, double* __restrict__ lfK, double* __restrict__ lfS, int s0,
    long long* __restrict__ dbg, int ablate) {
    __shared__ __attribute__((aligned(16))) double smem[SLEAF_BATCH_LDS];
    sleaf_batch_body<B, SB>(smem, blockIdx.x, blockIdx.y, M, T, nodes, b, active, S_cnt, Uall, Eall, fall, wall, linAall, Call, Hall, I0all, chG, chH, chD,
                            chy, sbimg, Zall, lfK, lfS, s0, dbg, ablate);
}

template <int B, int SB>
int launch_sleaf_batch(hpf_handle* h, const LaunchCtx& ctx, const TreeDev& T, const int* nodes, int count) {
    ScopedTimer t(h, T_SOLVE, ctx.stream);
    const dim3 grid((unsigned)count, (unsigned)BatchTile<SB>::tiles(ctx.S));
    hipLaunchKernelGGL((k_sleaf_batch<B, SB>), grid, dim3(256), 0, ctx.stream, h->M, T, nodes, 2 * h->Hn, ctx.active, ctx.S, h->d_U,
                       h->d_E, h->d_fb, h->d_w, h->d_linA, h->d_C, h->d_H, h->d_I0, h->d_chG, h->d_chH, h->d_chD, h->d_chy,
                       active_tree(h).d_sbimg, h->d_Z, h->d_lfK, h->d_lfS, ctx.s0, h->d_dbg, h->sw.debug_ablate);
    return launch_status(h);
}
