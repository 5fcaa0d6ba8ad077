// libhpf.so — C ABI (include/hpf.h), assembly kernels and the dense (rocSOLVER) Newton step.
//
// Data layout in HBM (all FP64 / complex128, scenario index slowest):
//   model, shared by all scenarios:  rowptr[n+1], col[nnz], erow[nnz] (row of each stored entry), diag[n],
//       Y[Hn][nnz] complex (one CSR pattern for all harmonics: lanes sweep the entries of one harmonic, so the
//       admittance read of the Jacobian kernel is a fully coalesced 16 B/lane stream), dev[n],
//       Y_N[n_dev][Hn][Hn], I_N[n_dev][Hn].
//   state: Vm,Va[S][Hn*n]; U,E[S][Hn*n] complex (polar -> rectangular once per iteration, reused by mismatch and
//       Jacobian; stacked harmonic-major so that for a fixed harmonic consecutive lanes touch consecutive buses);
//       P,Q[S][n]; f[S][N]; dense J[S][N*N] column-major in the reference's row/column order (HG:469-472).
// Kernels and what bounds them (algorithmic bytes per NR iteration per scenario):
//   k_mismatch   HBM: 16*Hn*nnz (Y) + 16*Hn*n (U) + 8*N (f) + pattern;   k_jac_*  HBM: Y + U,E + 32*E_cplx written;
//   dense solve  FP64 matrix pipe: 2/3 N^3 + 2 N^2 flop (rocSOLVER getrf/getrs).
#include <math.h>
#include <chrono>
#include <functional>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <rocsolver/rocsolver.h>

#include "hpf_accum.hpp"
#include "hpf_branch.hpp"
#include "hpf_distortion.hpp"
#include "hpf_groups.hpp"
#include "hpf_internal.hpp"
#include "hpf_sources.hpp"
#include "hpf_update.hpp"
#include "hpf_waveform.hpp"

using namespace hpf;

#define HIPCHK(expr)                              \
    do {                                          \
        hipError_t _e = (expr);                   \
        if (_e != hipSuccess) {                   \
            h->last_detail = (int)_e;             \
            return HPF_E_HIP;                     \
        }                                         \
    } while (0)

#define BLASCHK(expr)                             \
    do {                                          \
        rocblas_status _s = (expr);               \
        if (_s != rocblas_status_success) {       \
            h->last_detail = (int)_s;             \
            return HPF_E_ROCSOLVER;               \
        }                                         \
    } while (0)

// ------------------------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------------------------
namespace {

constexpr int TPB = 256;

// polar -> rectangular for `count` stacked entries of every scenario (count = Hn*n, or n for the fundamental pf)
// Device layout of Vm, Va, U, E: bus-major, entry (bus i, harmonic position q) at i*Hn + q (Model::vi); the C ABI keeps the
// reference's stacked order and hpf_set_state / hpf_get_state transpose.  FUND: the n entries of harmonic position 0.
template <bool FUND>
__global__ void k_polar(int count, int stride, int Hn, const double* __restrict__ Vm, const double* __restrict__ Va,
                        cplx* __restrict__ U, cplx* __restrict__ E) {
    const int k = blockIdx.x * TPB + threadIdx.x;
    if (k >= count) return;
    const size_t o = (size_t)blockIdx.y * stride + (FUND ? (size_t)k * Hn : (size_t)k);
    cplx u, e;
    polar<FUND>(Vm[o], Va[o], u, e);
    U[o] = u;
    E[o] = e;
}

// XCD-aware launch geometry of the per-element kernels (thread per (bus, harmonic) of one scenario): workgroups are dealt round-robin
// over the 8 XCDs by their linear id (MI355X_MICROARCH.md, workgroup dispatch), and every XCD has its own 4 MiB L2.  A 1-D grid
// whose id is (scenario block, x block, scenario mod 8) keeps ALL workgroups of a scenario on one XCD, so the scenario's voltages --
// gathered again by the neighbours' rows and by the Norton rows of the same bus -- are fetched into one L2 instead of eight.
// With fewer than 8 scenarios that placement would leave XCDs empty (ONE scenario: the whole kernel on 32 of the 256 CUs -- 196 us
// instead of 30 for the mismatch of the 10 000-bus x 49-harmonic feeder): the workgroups are then dealt over the whole chip.
// ... realised WITHOUT index arithmetic through a 3-D grid (the linear workgroup id is x + gx (y + gy z)): S >= 8: grid (8, nbx, ceil(S/8))
// -> x = scenario mod 8 = the XCD, y = x block, z = scenario block; S < 8: grid (nbx, S, 1).  (The decode of a 1-D id took two integer
// divisions by run-time values per workgroup: ~50 scalar instructions and two quarter-rate reciprocals in front of the first load.)
__device__ __forceinline__ bool xcd_map(int S, int& bx, int& slot) {
    if (S < 8) {
        bx = blockIdx.x;
        slot = blockIdx.y;
        return true;
    }
    bx = blockIdx.y;
    slot = blockIdx.z * 8 + blockIdx.x;
    return slot < S;
}
__host__ inline dim3 xcd_grid(int nbx, int S) {
    return S < 8 ? dim3((unsigned)nbx, (unsigned)S, 1) : dim3(8, (unsigned)nbx, (unsigned)((S + 7) / 8));
}
// unsigned division of t < 2^32 / d by a run-time d through its reciprocal m = floor(2^32 / d) + 1 (host: div_magic): exact there
// (hpf_create refuses models with (n Hn + 256) Hn >= 2^32).  d = 1 has no 32-bit reciprocal: magic 0 stands for "t itself" (a model
// with the fundamental alone, H_MAX = 1 or 2).
__device__ __forceinline__ int div_by(int t, unsigned magic) { return magic ? (int)__umulhi((unsigned)t, magic) : t; }
__host__ inline unsigned div_magic(int d) { return d <= 1 ? 0u : (unsigned)((1ull << 32) / (unsigned)d + 1ull); }

// ||.||_inf with NaN propagation: |x| as its IEEE bit pattern is monotone for non-negative doubles, and every NaN
// pattern compares above +inf, so an unsigned max reproduces np.linalg.norm(f, inf) including its NaN result
// (HG:389) and is independent of the reduction order.
__device__ __forceinline__ unsigned long long abs_bits(double v) {
    return (unsigned long long)__double_as_longlong(fabs(v));
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}

// Norton injection of harmonic position q (HG:313-323: I_N[q] - sum_p Y_N[q,p] U_p) with both operands in LDS: the device type's
// Y_N^T (ynl[p*Hn + q]) and the bus's Hn voltages (ul[p]).  Same operations in the same order as norton_injection (hpf_assembly.hpp):
// the reference's zgemv_n rounding -- 4-column groups of FMA chains, groups added in order; the Hn % 4 tail rows fused per column.
// norton_injection_lds_in: with the source current `in` of (bus, q) supplied by the caller (the source variants of the kernels fetch it with
// their first batch of loads); norton_injection_lds: src = the bus's Hn per-scenario source currents, nullptr = the model's I_N.
__device__ __forceinline__ cplx norton_injection_lds_in(const Model& M, const cplx* __restrict__ ynl, const cplx* __restrict__ ul, int q, cplx in) {
    const int Hn = M.Hn;
    cplx acc = {0.0, 0.0};
    const cplx* yq = ynl + q;
    if (q < (Hn & ~3)) {
        int p0 = 0;
        for (; p0 + 4 <= Hn; p0 += 4) {                  // a full group: its eight LDS reads first, then the four FMA chains
            cplx y4[4], u4[4];
#pragma unroll
            for (int pp = 0; pp < 4; ++pp) {
                y4[pp] = yq[(p0 + pp) * Hn];
                u4[pp] = ul[p0 + pp];
            }
            double rr = 0, ii = 0, ri = 0, ir = 0;
#pragma unroll
            for (int pp = 0; pp < 4; ++pp) {
                rr = fma(y4[pp].re, u4[pp].re, rr);
                ri = fma(y4[pp].re, u4[pp].im, ri);
                ii = fma(y4[pp].im, u4[pp].im, ii);
                ir = fma(y4[pp].im, u4[pp].re, ir);
            }
            acc.re += rr - ii;
            acc.im += ri + ir;
        }
        if (p0 < Hn) {                                   // the last, shorter group
            double rr = 0, ii = 0, ri = 0, ir = 0;
            for (int p = p0; p < Hn; ++p) {
                const cplx u = ul[p], y = yq[p * Hn];
                rr = fma(y.re, u.re, rr);
                ri = fma(y.re, u.im, ri);
                ii = fma(y.im, u.im, ii);
                ir = fma(y.im, u.re, ir);
            }
            acc.re += rr - ii;
            acc.im += ri + ir;
        }
    } else {
        for (int p = 0; p < Hn; ++p) {
            const cplx u = ul[p], y = yq[p * Hn];
            acc.re += fma(y.re, u.re, -(y.im * u.im));
            acc.im += fma(y.re, u.im, y.im * u.re);
        }
    }
    return csub(in, acc);
}

__device__ __forceinline__ cplx norton_injection_lds(const Model& M, int d, const cplx* __restrict__ ynl, const cplx* __restrict__ ul, int q,
                                                     const cplx* __restrict__ src = nullptr) {
    return norton_injection_lds_in(M, ynl, ul, q, src ? src[q] : M.IN[(size_t)d * M.Hn + q]);
}

// harmonic_mismatch (HG:360-390).  One workgroup = one scenario x a tile of consecutive buses (thread t = i*Hn + q: bus-major, so a
// workgroup's 256 rows are ~10 whole buses and their voltages one contiguous run).  Staged in LDS per workgroup (coupled Norton data):
// the device type's Y_N^T (Hn x Hn complex: 10.8 KB at K = 25, shared by every bus of that type -- L2-resident) and the tile's bus
// voltages; the Norton coupling rows of a nonlinear bus (HG:313-323: the only O(Hn^2) part of the mismatch) then run out of LDS.
// The network part walks the CSR row (ascending columns, csr_matvec order) with 16-byte gathers of the neighbours' voltages, which
// the XCD-aware placement (xcd_map) keeps in ONE L2 per scenario.  ||f||_inf: wave shuffle + one partial maximum per wavefront.
// f: the reference's stacked real layout (HG:388; dense solver, C ABI) or nullptr; fb: bus-major image [bus][2q + (Re|Im)] with
// stride Bst and zeros where there is no equation (tree kernels) or nullptr.
// SRC (harmonic variant only; launched when the batch has sources, hpf_set_sources): the Norton rows take I_src[s][i - m][q] (src: [S][n - m][Hn],
// thread t = i*Hn + q -> a wavefront reads one contiguous run of 16-byte values) in place of I_N[dev(i)][q].  The value is fetched with batch A
// below -- independent of every other load -- so the kernel's chain of dependent fetches is as long as without sources.
template <bool FUND, bool SRC>
__global__ __launch_bounds__(TPB, 8) void k_mismatch(Model M, int count, int N, int Nc, const int* __restrict__ active, const cplx* __restrict__ U,
                           const double* __restrict__ P, const double* __restrict__ Q, double* __restrict__ f,
                           unsigned long long* __restrict__ errpart, int pstride, cplx* __restrict__ I0, double* __restrict__ fb, int Bst,
                           int s0, int S_cnt, unsigned hn_magic, const cplx* __restrict__ src) {
    static_assert(!(FUND && SRC), "the fundamental pf never reads sources");
    extern __shared__ cplx mm_lds[];                    // [Hn*Hn] Y_N^T of the tile's first device type | [tile buses][Hn] voltages
    int bx, slot;
    if (!xcd_map(S_cnt, bx, slot)) return;
    const int s = active ? active[slot + s0] : slot + s0;   // slot -> scenario (active list; -1: frozen / empty slot)
    if (s < 0) return;
    const int tid = threadIdx.x;
    const int t = bx * TPB + tid;
    const cplx* Us = U + (size_t)s * M.n * M.Hn;
    const int Hn = M.Hn;
    const bool live = t < count;
    const int i = live ? (FUND ? t : div_by(t, hn_magic)) : M.n - 1, q = (FUND || !live) ? 0 : t - i * Hn;
    // The kernel is bound by the chain of dependent fetches of a wavefront, so the harmonic variant issues them in BATCHES of independent,
    // branch-free loads (indices clamped into the row, values masked afterwards): A = the row bounds, Y_N^T and the tile's bus voltages
    // (for LDS); B = Y of the row's first PF entries AND the neighbours' voltages (their columns come with the row bounds in the bus's row
    // record: two dependent round trips, not three).  Longer rows finish in a loop.  Same
    // operations in the same order as mismatch_row / row_current: bit-identical results.
    constexpr int PF = 3;                               // (a feeder row holds 3 entries on average)
    int d0 = -1, i_first = 0;
    int e0 = 0, e1 = 0;
    cplx yv[PF], ug[PF];
    cplx sv = {0.0, 0.0};
    if (!FUND) {
        const int4 rr = reinterpret_cast<const int4*>(M.rowrec)[2 * i];          // (rowptr[i], rowptr[i+1], col[e0], col[e0+1])
        const int rr2 = M.rowrec[8 * i + 4];                                      //  col[e0+2]
        if (SRC) sv = src[((size_t)s * (M.n - M.m) + (i >= M.m ? i - M.m : 0)) * Hn + q];   // (linear buses: a valid address, value unused)
        e0 = rr.x;
        e1 = rr.y;
        const bool has_nl = M.coupled && M.YNt;
        i_first = div_by(bx * TPB, hn_magic);
        int i_last = div_by(bx * TPB + TPB - 1, hn_magic);
        if (i_last > M.n - 1) i_last = M.n - 1;
        const bool stage = has_nl && i_last >= M.m;     // the tile holds nonlinear buses (they come last in the bus order, HG:83)
        const int nyn = Hn * Hn, nv = (i_last - i_first + 1) * Hn;          // nv <= 2 TPB
        double2 tv0 = {0.0, 0.0}, tv1 = {0.0, 0.0};
        if (stage) {
            d0 = M.dev[i_first > M.m ? i_first : M.m];
            const double2* Ut = reinterpret_cast<const double2*>(Us + (size_t)i_first * Hn);
            tv0 = Ut[tid < nv ? tid : 0];
            tv1 = Ut[tid + TPB < nv ? tid + TPB : 0];
            const double2* src = reinterpret_cast<const double2*>(M.YNt + (size_t)d0 * nyn);
            double2* dst = reinterpret_cast<double2*>(mm_lds);
            for (int base = tid; base < nyn; base += 4 * TPB) {                 // (26 harmonics: one pass of three loads in flight)
                const double2 y0 = src[base], y1 = src[base + TPB < nyn ? base + TPB : 0], y2 = src[base + 2 * TPB < nyn ? base + 2 * TPB : 0],
                              y3 = src[base + 3 * TPB < nyn ? base + 3 * TPB : 0];
                dst[base] = y0;
                if (base + TPB < nyn) dst[base + TPB] = y1;
                if (base + 2 * TPB < nyn) dst[base + 2 * TPB] = y2;
                if (base + 3 * TPB < nyn) dst[base + 3 * TPB] = y3;
            }
        }
        static_assert(PF == 3, "row records hold the first three neighbours");
        const int jc[PF] = {rr.z, rr.w, rr2};               // (clamped into the row by the host: entries past the row's end repeat its last)
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            const int e = e0 + u < e1 ? e0 + u : e1 - 1;
            yv[u] = M.Y[(size_t)e * Hn + q];
        }
#pragma unroll
        for (int u = 0; u < PF; ++u) ug[u] = Us[(size_t)jc[u] * Hn + q];
        if (stage) {
            double2* ul = reinterpret_cast<double2*>(mm_lds + nyn);
            if (tid < nv) ul[tid] = tv0;
            if (tid + TPB < nv) ul[tid + TPB] = tv1;
        }
        if (has_nl) __syncthreads();
    }
    unsigned long long b = 0;
    if (live) {
        const int k = q * M.n + i;
        cplx v = {0.0, 0.0};
        if (k >= 1) {
            if (FUND) {
                v = mismatch_row_qi<true>(M, Us, P + (size_t)s * M.n, Q + (size_t)s * M.n, 0, i, I0 ? I0 + (size_t)s * M.n : nullptr);   // (pf's tree kernels read the row currents back)
            } else {
                cplx I = {0.0, 0.0};                    // row_current: ascending columns, every product and sum rounded (csr_matvec)
#pragma unroll
                for (int u = 0; u < PF; ++u) {
                    const cplx nx = cadd(I, cmul_unf(yv[u], ug[u]));
                    const bool has = e0 + u < e1;       // (component selects: a select of the struct goes through scratch)
                    I.re = has ? nx.re : I.re;
                    I.im = has ? nx.im : I.im;
                }
                for (int e = e0 + PF; e < e1; ++e) I = cadd(I, cmul_unf(M.Y[(size_t)e * Hn + q], Us[(size_t)M.col[e] * Hn + q]));
                if (q == 0 && i < M.m) {                // power row (HG:372-380)
                    if (I0) I0[(size_t)s * M.n + i] = I;
                    const cplx sl = cmul_npy(Us[(size_t)i * Hn], cconj(I));
                    v = {P[(size_t)s * M.n + i] + sl.re, Q[(size_t)s * M.n + i] + sl.im};
                } else if (d0 >= 0 && i >= M.m && M.dev[i] == d0) {
                    // current-balance row of a nonlinear bus (HG:351,354): network current + Norton injection out of LDS
                    v = cadd(I, SRC ? norton_injection_lds_in(M, mm_lds, mm_lds + Hn * Hn + (i - i_first) * Hn, q, sv)
                                    : norton_injection_lds(M, d0, mm_lds, mm_lds + Hn * Hn + (i - i_first) * Hn, q));
                } else if (i >= M.m) {
                    v = cadd(I, SRC ? norton_injection_in(M, Us, q, i, sv) : norton_injection(M, Us, q, i));
                } else {
                    v = I;
                }
            }
            if (f) store_mismatch(f + (size_t)s * N, Nc, M.c, k, v);
            b = abs_bits(v.re);
            if (k >= M.c) {
                const unsigned long long bi = abs_bits(v.im);
                b = bi > b ? bi : b;
            }
        }
        if (!FUND && fb) {
            double* o = fb + ((size_t)s * M.n + i) * Bst + 2 * q;
            *reinterpret_cast<double2*>(o) = double2{k >= 1 ? v.re : 0.0, k >= M.c ? v.im : 0.0};
        }
    }
    // ||f||_inf of the scenario: every WAVEFRONT leaves its partial maximum (no LDS, no workgroup barrier, no atomic -- 102 workgroups of a
    // scenario used to meet on one L2 line); the consumer of the norm (k_finalize, k_queue_first, k_err_reduce) takes the maximum of the
    // scenario's partials.  A maximum does not depend on the order: the result is the same word as before.
    b = wave_max_u64(b);
    if ((tid & 63) == 0) errpart[(size_t)s * pstride + (size_t)bx * (TPB / 64) + (tid >> 6)] = b;
}

// Residual check of a Newton step (option "step_residual_check"): r = f - J dx row by row without forming J, between the linear solve and
// the state update.  Shaped like k_mismatch: one thread per complex row (t = i*Hn + q), XCD-aware placement, slot list; a tile with
// nonlinear buses stages the device type's Y_N^T and the tile's U, E and step (d theta, d V per column) in LDS, so that the Hn cross terms
// of a nonlinear row -- the only O(Hn^2) part -- and its Norton injection run out of LDS.  Per-entry arithmetic: hpf_assembly.hpp
// (step_residual_row / JResid: the entries and masks of hpf_jacobian_csr); f is evaluated again exactly as k_mismatch evaluates it (the
// step overwrote d_f on the stacked paths, the tree sweeps own d_fb).  It never reads a debug switch: the step is judged against the true J.
// Every wavefront leaves four partial maxima (|r|, row sums of |J|, |dx|, |f|) -> respart[s][4][pstride]; k_step_eta forms eta.
// BUSX: the step is the bus-major image (stride Bst) of the multi-wave block-tree sweep, else the stacked vector.  stage: the launch has the LDS.
// SRC: the batch has sources (hpf_set_sources) -- f is formed with I_src[s][i - m][q], fetched before the staging loads, as k_mismatch<false, true> forms it.
template <bool BUSX, bool SRC>
__global__ __launch_bounds__(TPB) void k_step_residual(Model M, int count, int N, int Nc, const int* __restrict__ active, const cplx* __restrict__ U,
                           const cplx* __restrict__ E, const double* __restrict__ P, const double* __restrict__ Q,
                           const double* __restrict__ step, int Bst, unsigned long long* __restrict__ respart, int pstride,
                           int s0, int S_cnt, unsigned hn_magic, int stage_ok, const cplx* __restrict__ src) {
    extern __shared__ cplx rs_lds[];                    // [Hn*Hn] Y_N^T of the tile's first device type | [tile buses][Hn] U | E | step
    int bx, slot;
    if (!xcd_map(S_cnt, bx, slot)) return;
    const int s = active ? active[slot + s0] : slot + s0;
    if (s < 0) return;
    const int tid = threadIdx.x;
    const int t = bx * TPB + tid;
    const int Hn = M.Hn;
    const cplx* Us = U + (size_t)s * M.n * Hn;
    const cplx* Es = E + (size_t)s * M.n * Hn;
    const double* ds = step + (BUSX ? (size_t)s * M.n * Bst : (size_t)s * N);
    const StepBusMajor dxb{ds, Bst};
    const StepStacked dxs{ds, Nc, M.c};
    const bool live = t < count;
    const int i = live ? div_by(t, hn_magic) : M.n - 1, q = live ? t - i * Hn : 0;
    cplx sv = {0.0, 0.0};
    if (SRC) sv = src[((size_t)s * (M.n - M.m) + (i >= M.m ? i - M.m : 0)) * Hn + q];
    const int i_first = div_by(bx * TPB, hn_magic);
    int i_last = div_by(bx * TPB + TPB - 1, hn_magic);
    if (i_last > M.n - 1) i_last = M.n - 1;
    const int nyn = Hn * Hn, nv = (i_last - i_first + 1) * Hn;          // nv <= (TPB / Hn + 2) Hn: the launch sized the LDS for it
    const bool stage = stage_ok && M.coupled && M.YNt && i_last >= M.m;   // (uniform over the workgroup)
    int d0 = -1;
    cplx *ul = rs_lds + nyn, *el = ul + nv, *xl = el + nv;
    if (stage) {
        d0 = M.dev[i_first > M.m ? i_first : M.m];
        const double2* src = reinterpret_cast<const double2*>(M.YNt + (size_t)d0 * nyn);
        double2* dst = reinterpret_cast<double2*>(rs_lds);
        for (int x = tid; x < nyn; x += TPB) dst[x] = src[x];
        const size_t o = (size_t)i_first * Hn;
        for (int x = tid; x < nv; x += TPB) {
            ul[x] = Us[o + x];
            el[x] = Es[o + x];
            const int ib = i_first + div_by(x, hn_magic), p = x - (ib - i_first) * Hn;
            xl[x] = BUSX ? dxb(0, p, ib) : dxs(p * M.n + ib, p, ib);
        }
        __syncthreads();
    }
    unsigned long long br = 0, bw = 0, bd = 0, bf = 0;
    const int k = q * M.n + i;
    if (live && k >= 1) {
        const bool mine = d0 >= 0 && i >= M.m && M.dev[i] == d0;       // nonlinear bus of the staged device type
        const int loc = (i - i_first) * Hn;
        const cplx f = mine ? cadd(row_current(M, Us, q, i), SRC ? norton_injection_lds_in(M, rs_lds, ul + loc, q, sv)
                                                                 : norton_injection_lds(M, d0, rs_lds, ul + loc, q))
                       : (SRC && i >= M.m) ? cadd(row_current(M, Us, q, i), norton_injection_in(M, Us, q, i, sv))
                                           : mismatch_row_qi<false>(M, Us, P + (size_t)s * M.n, Q + (size_t)s * M.n, q, i);
        StepRow rw;
        if (stage && i >= M.m) {
            // A nonlinear row of a staged tile: the entries of jcsr_walk with the cross terms' operands out of LDS.  The admittance row comes
            // FIRST, for all lanes together, then the cross terms in ascending column p != q: inside the column loop (jcsr_walk's order) the lane
            // with p == q made its whole wavefront wait for the row's dependent fetches at EVERY p (measured: 155 us for one workgroup at Hn = 26,
            // 6 us per column).  Only the order of the sum differs from the host's row function; the rounding bound does not depend on it.
            // Y_N^T of another device type than the staged one comes from memory (the lanes of a bus read one contiguous run per column).
            JResid<StepStacked> res{M, Us, Es, jcsr_row_qi(M, q, i), dxs, {f, {0.0, 0.0}, {0.0, 0.0}}};
            for (int e = M.rowptr[i]; e < M.rowptr[i + 1]; ++e) {
                const int j = M.col[e];
                if (!jcsr_has_entry(M, res.R, e, j)) continue;
                const Blk2 b = jac_current_entry(M, Us, Es, q, i, j, e);
                res.term(k - i + j, b, BUSX ? dxb(0, q, j) : dxs(k - i + j, q, j));
            }
            const cplx* yq = (mine ? rs_lds : M.YNt + (size_t)M.dev[i] * nyn) + q;
            for (int p = 0; p < Hn; ++p) {
                const cplx yn = yq[(size_t)p * Hn];
                if (p != q && (yn.re != 0.0 || yn.im != 0.0)) res.term(p * M.n + i, norton_cross_blk(yn, ul[loc + p], el[loc + p]), xl[loc + p]);
            }
            rw = res.s;
        } else if (BUSX) {
            rw = step_residual_row(M, Us, Es, q, i, f, dxb);
        } else {
            rw = step_residual_row(M, Us, Es, q, i, f, dxs);
        }
        const cplx d = BUSX ? dxb(k, q, i) : dxs(k, q, i);
        br = abs_bits(rw.r.re);
        bw = abs_bits(rw.w.re);
        bd = abs_bits(d.re);
        bf = abs_bits(f.re);
        if (k >= M.c) {
            unsigned long long v;
            v = abs_bits(rw.r.im); br = v > br ? v : br;
            v = abs_bits(rw.w.im); bw = v > bw ? v : bw;
            v = abs_bits(d.im); bd = v > bd ? v : bd;
            v = abs_bits(f.im); bf = v > bf ? v : bf;
        }
    }
    br = wave_max_u64(br);
    bw = wave_max_u64(bw);
    bd = wave_max_u64(bd);
    bf = wave_max_u64(bf);
    if ((tid & 63) == 0) {
        unsigned long long* o = respart + (size_t)s * 4 * pstride + (size_t)bx * (TPB / 64) + (tid >> 6);
        o[0] = br;
        o[pstride] = bw;
        o[2 * (size_t)pstride] = bd;
        o[3 * (size_t)pstride] = bf;
    }
}

// Dense Jacobian, network entries: one thread per (harmonic position, stored admittance entry) of one scenario.
template <bool FUND>
__global__ void k_jac_dense(Model M, int total, int N, int Nc, size_t J_stride, const int* __restrict__ active,
                            const int* __restrict__ erow, const cplx* __restrict__ U, const cplx* __restrict__ E,
                            double* __restrict__ J) {
    const int s = active ? active[blockIdx.y] : (int)blockIdx.y;
    if (s < 0) return;
    const int t = blockIdx.x * TPB + threadIdx.x;
    if (t >= total) return;
    const int q = t / M.nnz, e = t - q * M.nnz;
    const int i = erow[e];
    DenseEmit em{J + (size_t)s * J_stride, N, Nc, M.c};
    const size_t so = (size_t)s * M.n * M.Hn;
    if (FUND)
        jac_entry_fund(M, U + so, E + so, i, e, em);
    else
        jac_entry(M, U + so, E + so, q, i, e, em);
}

// Dense Jacobian, coupled Norton cross terms q != p at nonlinear buses (HG:425-435).
__global__ void k_jac_cross_dense(Model M, int total, int N, int Nc, size_t J_stride, const int* __restrict__ active,
                                  const cplx* __restrict__ U, const cplx* __restrict__ E, double* __restrict__ J) {
    const int s = active ? active[blockIdx.y] : (int)blockIdx.y;
    if (s < 0) return;
    const int t = blockIdx.x * TPB + threadIdx.x;
    if (t >= total) return;
    // consecutive threads -> consecutive buses (coalesced U/E reads for a fixed column harmonic p)
    const int nnl = M.n - M.m;
    const int i = M.m + t % nnl;
    const int qp = t / nnl;
    const int q = qp / M.Hn, p = qp - q * M.Hn;
    if (p == q) return;
    DenseEmit em{J + (size_t)s * J_stride, N, Nc, M.c};
    const size_t so = (size_t)s * M.n * M.Hn;
    jac_cross(M, U + so, E + so, q, p, i, em);
}

// The Jacobian in CSR form (HG:469-472 as the reference returns it, hpf_jacobian_csr): one thread per real row.  k_jcsr_count leaves
// the row lengths, k_jcsr_scan turns them into indptr (one workgroup: chunk sums, LDS scan of the 1 024 partials, chunk prefixes),
// k_jcsr_fill writes column indices and values of scenario `s` behind indptr[r] (per-entry arithmetic: hpf_assembly.hpp, the same
// functions as the dense target).
__global__ void k_jcsr_count(Model M, int N, int Nc, int* __restrict__ cnt) {
    const int r = blockIdx.x * TPB + threadIdx.x;
    if (r >= N) return;
    const JCount c = jcsr_count_row(M, Nc, r);
    cnt[r] = c.n_theta + c.n_v;
}

__global__ __launch_bounds__(1024) void k_jcsr_scan(int N, int* __restrict__ indptr, long long* __restrict__ total) {
    __shared__ long long part[1024];
    const int tid = threadIdx.x;
    const int chunk = (N + 1023) / 1024;
    const int b = tid * chunk < N ? tid * chunk : N, e = b + chunk < N ? b + chunk : N;
    long long s = 0;
    for (int i = b; i < e; ++i) s += indptr[i];
    part[tid] = s;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const long long v = tid >= off ? part[tid - off] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    long long base = tid ? part[tid - 1] : 0;
    for (int i = b; i < e; ++i) {
        const int c = indptr[i];
        indptr[i] = (int)base;
        base += c;
    }
    if (tid == 1023) {
        *total = part[1023];
        indptr[N] = part[1023] < 0x7fffffffll ? (int)part[1023] : 0x7fffffff;
    }
}

__global__ void k_jcsr_fill(Model M, int N, int Nc, const int* __restrict__ indptr, const cplx* __restrict__ U,
                            const cplx* __restrict__ E, int* __restrict__ col, double* __restrict__ val) {
    const int r = blockIdx.x * TPB + threadIdx.x;
    if (r >= N) return;
    jcsr_fill_row(M, U, E, Nc, r, indptr[r], col, val);
}

// x <- x - step, scattered back into (Va, Vm) (HG:478,484-485 / HG:229,234-235), then refresh U, E of the entry.
template <bool FUND>
__global__ void k_update(int n, int Hn, int c, int count, int stride, int N, int Nc, const int* __restrict__ active,
                         const double* __restrict__ step, double* __restrict__ Vm, double* __restrict__ Va,
                         cplx* __restrict__ U, cplx* __restrict__ E,
                         const double* __restrict__ xbus, int Bst, int s0, unsigned hn_magic) {
    const int s = active ? active[blockIdx.y + s0] : (int)blockIdx.y + s0;   // slot -> scenario (active list; -1: frozen / empty slot)
    if (s < 0) return;
    const int t = blockIdx.x * TPB + threadIdx.x;
    if (t >= count) return;
    const int i = FUND ? t : div_by(t, hn_magic), q = FUND ? 0 : t - i * Hn;          // thread t = i*Hn + q: bus-major state arrays
    const int k = q * n + i;                                             // stacked index (HG:139-143)
    const size_t o = (size_t)s * stride + (size_t)i * Hn + q;
    double va = Va[o], vm = Vm[o];
    if (xbus) {
        // multi-wave block-tree sweep: the Newton step stays in its bus-major image [bus][2q+t] (no scattered copy into the
        // reference's stacked order by the back-substitution kernels)
        const double2 dx = *reinterpret_cast<const double2*>(xbus + ((size_t)s * n + i) * Bst + 2 * q);
        if (k >= 1) va = va - dx.x;
        if (k >= c) vm = vm - dx.y;
    } else {
        const double* d = step + (size_t)s * N;
        if (k >= 1) va = va - d[k - 1];
        if (k >= c) vm = vm - d[Nc + k - c];
    }
    Va[o] = va;
    Vm[o] = vm;
    cplx u, e;
    polar<FUND>(vm, va, u, e);
    U[o] = u;
    E[o] = e;
}

// k_update<false> with the step applied in rectangular form (option "rectangular_update", hpf_update.hpp): same grid, same thread <-> entry map,
// same two step sources and slot list; it additionally reads the U, E of the entry (what polar<false> left there for the state it reads) before
// it overwrites them.  Entries whose magnitude is not a state variable (k < c) take the reference's update, bit for bit.
__global__ void k_update_rect(int n, int Hn, int c, int count, int stride, int N, int Nc, const int* __restrict__ active,
                              const double* __restrict__ step, double* __restrict__ Vm, double* __restrict__ Va,
                              cplx* __restrict__ U, cplx* __restrict__ E,
                              const double* __restrict__ xbus, int Bst, int s0, unsigned hn_magic) {
    const int s = active ? active[blockIdx.y + s0] : (int)blockIdx.y + s0;
    if (s < 0) return;
    const int t = blockIdx.x * TPB + threadIdx.x;
    if (t >= count) return;
    const int i = div_by(t, hn_magic), q = t - i * Hn;
    const int k = q * n + i;
    const size_t o = (size_t)s * stride + (size_t)i * Hn + q;
    double va = Va[o], vm = Vm[o], dth = 0.0, dv = 0.0;
    if (xbus) {
        const double2 dx = *reinterpret_cast<const double2*>(xbus + ((size_t)s * n + i) * Bst + 2 * q);
        dth = dx.x;
        dv = dx.y;
    } else {
        const double* d = step + (size_t)s * N;
        if (k >= 1) dth = d[k - 1];
        if (k >= c) dv = d[Nc + k - c];
    }
    update_rect(vm, va, U[o], E[o], k, c, dth, dv);
    Va[o] = va;
    Vm[o] = vm;
    cplx u, e;
    if (k >= c)
        update_rect_polar(vm, va, u, e);
    else
        polar<false>(vm, va, u, e);
    U[o] = u;
    E[o] = e;
}

// Per-scenario bookkeeping of the NR loop (HG:536-542 / HG:259-265).  The set of running scenarios is a SLOT LIST: active[i] =
// scenario id that slot i runs, or -1 (frozen scenario / empty slot); every kernel of the loop maps its blockIdx.y through it.
// first: slot i <- scenario i, record the initial mismatch, apply the stop rule (mask: a repeat pass starts masked scenarios only).
// else: one thread per slot; a scenario that meets the stop rule freezes (its slot becomes -1).
// max over the np partial maxima a scenario's mismatch launch left (k_mismatch), taken by one wavefront; every lane receives it
__device__ __forceinline__ unsigned long long slot_err_bits(const unsigned long long* __restrict__ part, int np) {
    unsigned long long b = 0ull;
    for (int i = threadIdx.x & 63; i < np; i += 64) {
        const unsigned long long v = part[i];
        b = v > b ? v : b;
    }
    return wave_max_u64(b);
}

// (one wavefront per slot: it first reduces the scenario's partial maxima)
__global__ __launch_bounds__(64) void k_finalize(int S, int first, double thresh, int max_iter, int hist_cap, int hist_off,
                           const unsigned long long* __restrict__ errpart, int pstride, int np, double* __restrict__ err,
                           int* __restrict__ niter, int* __restrict__ active, int* __restrict__ nactive,
                           double* __restrict__ hist, int s0, const int* __restrict__ mask) {
    const int sl = blockIdx.x;
    if (sl >= S) return;
    const int slot = sl + s0;
    if (first) {
        const int s = slot;
        if (mask && !mask[s]) {           // repeat pass: the other scenarios keep their result and stay frozen
            if (threadIdx.x == 0) active[slot] = -1;
            return;
        }
        const double e = __longlong_as_double((long long)slot_err_bits(errpart + (size_t)s * pstride, np));
        if (threadIdx.x != 0) return;
        err[s] = e;
        niter[s] = 0;
        if (hist && hist_off == 0) hist[(size_t)s * hist_cap] = e;
        const int a = (e > thresh) && (0 < max_iter);
        active[slot] = a ? s : -1;
        if (a) atomicAdd(nactive, 1);
        return;
    }
    const int s = active[slot];
    if (s < 0) return;
    const double e = __longlong_as_double((long long)slot_err_bits(errpart + (size_t)s * pstride, np));
    if (threadIdx.x != 0) return;
    const int it = niter[s] + 1;
    err[s] = e;
    niter[s] = it;
    if (hist) hist[(size_t)s * hist_cap + it - 1 + (hist_off == 0 ? 1 : 0)] = e;
    const int a = (e > thresh) && (it < max_iter);
    if (!a) active[slot] = -1;
}

// ||f||_inf of every scenario -> out[s] as the bit pattern of the double (hpf_mismatch: the host copies it)
__global__ __launch_bounds__(64) void k_err_reduce(const unsigned long long* __restrict__ errpart, int pstride, int np,
                                                   unsigned long long* __restrict__ out) {
    const unsigned long long b = slot_err_bits(errpart + (size_t)blockIdx.x * pstride, np);
    if (threadIdx.x == 0) out[blockIdx.x] = b;
}

// eta = |f - J dx|_inf / (| |J| |_inf |dx|_inf + |f|_inf) of the step k_step_residual just judged (the normwise backward error of
// tests/stepcheck.py), one wavefront per slot: eta[s] the last step's, eta[S_alloc + s] the largest of the solve (-1: no step yet; a
// non-finite eta stays); eta > limit or not finite sets pivflag bit 3.
__global__ __launch_bounds__(64) void k_step_eta(int S, const int* __restrict__ active, const unsigned long long* __restrict__ respart, int pstride,
                                                 int np, double limit, double* __restrict__ eta, int eta_stride, int* __restrict__ pivflag, int s0) {
    const int sl = blockIdx.x;
    if (sl >= S) return;
    const int s = active ? active[sl + s0] : sl + s0;
    if (s < 0) return;
    const unsigned long long* part = respart + (size_t)s * 4 * pstride;
    const double r = __longlong_as_double((long long)slot_err_bits(part, np));
    const double w = __longlong_as_double((long long)slot_err_bits(part + pstride, np));
    const double d = __longlong_as_double((long long)slot_err_bits(part + 2 * (size_t)pstride, np));
    const double f = __longlong_as_double((long long)slot_err_bits(part + 3 * (size_t)pstride, np));
    if (threadIdx.x != 0) return;
    const double den = w * d + f;
    const double e = den > 0.0 ? r / den : r;
    eta[s] = e;
    const double m = eta[eta_stride + s];
    if (e != e || e > m) eta[eta_stride + s] = e;
    if (!(e <= limit)) atomicOr(pivflag + s, 8);
}

// Stable compaction of the slot list (running scenarios to the front, -1 behind them) and their count -> *count.  One workgroup;
// runs between two chunks of iterations, so that the next chunk launches grids over the running scenarios only and the
// 16-scenario tiles of the leaf kernels stay full.
__global__ __launch_bounds__(1024) void k_compact(int S, int* __restrict__ active, int* __restrict__ count) {
    __shared__ int wsum[16];
    __shared__ int base;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) base = 0;
    __syncthreads();
    for (int i0 = 0; i0 < S; i0 += 1024) {
        const int i = i0 + tid;
        const int v = i < S ? active[i] : -1;
        const unsigned long long bal = __builtin_amdgcn_ballot_w64(v >= 0);
        const int before = __builtin_popcountll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[wv] = __builtin_popcountll(bal);
        __syncthreads();                  // (also: every read of active[i0 .. i0+1023] precedes the writes below)
        int off = base;
        for (int w = 0; w < wv; ++w) off += wsum[w];
        int tot = 0;
        for (int w = 0; w < 16; ++w) tot += wsum[w];
        if (v >= 0) active[off + before] = v;        // off + before <= i: never overtakes an unread entry of a later tile
        __syncthreads();
        if (tid == 0) base += tot;
        __syncthreads();
    }
    for (int i = base + tid; i < S; i += 1024) active[i] = -1;
    if (tid == 0) *count = base;
}

__global__ void k_fill(double* p, size_t count, double v) {
    const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
    if (i < count) p[i] = v;
}

__global__ void k_set_int(int* p, int count, int v) {
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i < count) p[i] = v;
}

// scenarios that need the repeat pass with partial pivoting: a static pivot block went over the limit (pivflag bit 0), a step missed the
// residual check (bit 3, option "step_residual_check") or the mismatch became non-finite.  mask[s] = 1, pivflag[s] |= 2 ("repeated");
// k_restore_masked then resets their state.  The residual verdict of the first pass moves to bit 4, so that bit 3 is the repeat's own;
// eta (nullptr: check off) starts again for the repeated scenarios.
__global__ void k_mark_repeat(int S, const double* __restrict__ err, int* __restrict__ pivflag, int* __restrict__ mask,
                              int* __restrict__ count, double* __restrict__ eta, int eta_stride) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const double e = err[s];
    const int pf = pivflag[s];
    const int m = ((pf & 1) || (pf & 8) || e != e || isinf(e)) ? 1 : 0;
    mask[s] = m;
    if (m) {
        pivflag[s] = (pf & 1) | 2 | ((pf & 8) ? 16 : 0);      // bit 1: repeated (bits 0 and 4 stay: why)
        if (eta) {
            eta[s] = NAN;
            eta[eta_stride + s] = -1.0;
        }
        atomicAdd(count, 1);
    }
}

// hpf_stat.flags bits 6 and 7 from the pivflag word: a step of the first pass / of the pass whose result is returned missed the residual check
__device__ __forceinline__ int resid_flag_bits(int pf) {
    return (((pf & 2) ? (pf & 16) : (pf & 8)) ? 64 : 0) | ((pf & 8) ? 128 : 0);
}

// option "keep_previous_state": before a Newton step, the running scenarios' voltages -> the "previous state" copy (the reference
// returns the Jacobian of the LAST iteration, HG:537/560, i.e. the one built at the state before the last update)
__global__ void k_keep_prev(int count, const int* __restrict__ active, const double* __restrict__ Vm, const double* __restrict__ Va,
                            double* __restrict__ Vmp, double* __restrict__ Vap, int s0) {
    const int s = active ? active[blockIdx.y + s0] : (int)blockIdx.y + s0;
    if (s < 0) return;
    const int k = blockIdx.x * TPB + threadIdx.x;
    if (k < count) {
        Vmp[(size_t)s * count + k] = Vm[(size_t)s * count + k];
        Vap[(size_t)s * count + k] = Va[(size_t)s * count + k];
    }
}

// mask (per scenario, 0 / 1) -> slot list of a repeat pass: slot s runs scenario s or nothing
__global__ void k_mask_to_list(int S, const int* __restrict__ mask, int* __restrict__ list) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < S) list[s] = mask[s] ? s : -1;
}

__global__ void k_restore_masked(int count, const int* __restrict__ mask, const double* __restrict__ Vm0,
                                 const double* __restrict__ Va0, double* __restrict__ Vm, double* __restrict__ Va,
                                 double* __restrict__ hist, int hist_cap) {
    const int s = blockIdx.y;
    if (!mask[s]) return;
    const int k = blockIdx.x * TPB + threadIdx.x;
    if (k < count) {
        Vm[(size_t)s * count + k] = Vm0[(size_t)s * count + k];
        Va[(size_t)s * count + k] = Va0[(size_t)s * count + k];
    }
    if (hist && k < hist_cap) hist[(size_t)s * hist_cap + k] = NAN;
}

__global__ void k_init_voltages(int Hn, int count, double* Vm, double* Va) {
    const int k = blockIdx.x * TPB + threadIdx.x;
    if (k >= count) return;
    const size_t o = (size_t)blockIdx.y * count + k;
    Vm[o] = (k % Hn) == 0 ? 1.0 : 0.1;     // HG:181-183 (bus-major: harmonic position k % Hn)
    Va[o] = 0.0;
}

// ---- start state of the handle (hpf_start_*): sVm, sVa, sU, sE [n*Hn] bus-major like one scenario of the state.  One thread per (bus, harmonic)
// entry k = i*Hn + q, consecutive threads on consecutive doubles of the bus-major side.
// hpf_start_set: the caller's arrays in the ABI's stacked order q*n + i (uploaded as they are) -> bus-major, with U and E from polar<false>
__global__ void k_start_set(int n, int Hn, const double* __restrict__ Vm0, const double* __restrict__ Va0, double* __restrict__ sVm,
                            double* __restrict__ sVa, cplx* __restrict__ sU, cplx* __restrict__ sE) {
    const int k = blockIdx.x * TPB + threadIdx.x;
    if (k >= n * Hn) return;
    const int i = k / Hn, q = k - i * Hn;
    const double vm = Vm0[(size_t)q * n + i], va = Va0[(size_t)q * n + i];
    cplx u, e;
    polar<false>(vm, va, u, e);
    sVm[k] = vm;
    sVa[k] = va;
    sU[k] = u;
    sE[k] = e;
}

// hpf_start_capture: scenario `scen` of the batch -> the start state (U and E formed here, not copied: the batch's own are whatever the last
// solver kernel left).  *bad (zeroed by the caller) becomes 1 if an entry is one hpf_start_set refuses: non-finite, or a zero magnitude
__global__ void k_start_capture(int count, int scen, const double* __restrict__ Vm, const double* __restrict__ Va, double* __restrict__ sVm,
                                double* __restrict__ sVa, cplx* __restrict__ sU, cplx* __restrict__ sE, int* __restrict__ bad) {
    const int k = blockIdx.x * TPB + threadIdx.x;
    if (k >= count) return;
    const double vm = Vm[(size_t)scen * count + k], va = Va[(size_t)scen * count + k];
    if (!isfinite(vm) || !isfinite(va) || vm == 0.0) *bad = 1;
    cplx u, e;
    polar<false>(vm, va, u, e);
    sVm[k] = vm;
    sVa[k] = va;
    sU[k] = u;
    sE[k] = e;
}

// hpf_start_apply: the start state -> every scenario of the batch (blockIdx.y)
__global__ void k_start_apply(int count, const double* __restrict__ sVm, const double* __restrict__ sVa, const cplx* __restrict__ sU,
                              const cplx* __restrict__ sE, double* __restrict__ Vm, double* __restrict__ Va, cplx* __restrict__ U,
                              cplx* __restrict__ E) {
    const int k = blockIdx.x * TPB + threadIdx.x;
    if (k >= count) return;
    const size_t o = (size_t)blockIdx.y * count + k;
    Vm[o] = sVm[k];
    Va[o] = sVa[k];
    U[o] = sU[k];
    E[o] = sE[k];
}

// get_THD (HG:563-572) THD_F per bus, max over buses, plus the result flags; one block per scenario.  start_bit: 256 when the batch was started
// from the handle's start state (hpf_start_apply; k_queue_harvest: the queue ran with a start state set), else 0.  It also carries 512 when
// the harmonic steps of the solve are applied in rectangular form (option "rectangular_update": flags bit 9), and 1024 when the batch was solved
// with per-scenario source currents (hpf_set_sources: flags bit 10).
__global__ void k_stats(int n, int Hn, double thresh, int max_iter, const double* __restrict__ Vm,
                        const double* __restrict__ err, const int* __restrict__ niter, const int* __restrict__ pivflag,
                        int start_bit, hpf_stat* __restrict__ out) {
    const int s = blockIdx.x;
    const double* V = Vm + (size_t)s * n * Hn;
    double best = 0.0;
    bool nan = false;
    for (int b = threadIdx.x; b < n; b += TPB) {
        double hs = 0.0;
        for (int q = 1; q < Hn; ++q) hs = hs + V[(size_t)b * Hn + q] * V[(size_t)b * Hn + q];
        const double t = sqrt(hs) / fabs(V[(size_t)b * Hn]);
        if (t != t) nan = true;
        best = t > best ? t : best;
    }
    unsigned long long bits = nan ? 0x7ff8000000000000ull : (unsigned long long)__double_as_longlong(best);
    bits = wave_max_u64(bits);
    __shared__ unsigned long long red[TPB / 64];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = bits;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long r = red[0];
        for (int w = 1; w < TPB / 64; ++w) r = red[w] > r ? red[w] : r;
        hpf_stat st;
        st.n_iter = niter[s];
        const double e = err[s];
        st.err = e;
        const int pf = pivflag ? pivflag[s] : 0;
        st.flags = (e <= thresh ? 1 : 0) | ((niter[s] >= max_iter && !(e <= thresh)) ? 2 : 0) | ((e != e || isinf(e)) ? 4 : 0) |
                   ((pf & 1) ? 8 : 0) | ((pf & 2) ? 16 : 0) | ((pf & 4) ? 32 : 0) | resid_flag_bits(pf) | start_bit;
        st.thd_max = __longlong_as_double((long long)r);
        out[s] = st;
    }
}


// ---- hpf_solve_queue: a sweep of more scenarios than the handle has slots -------------------------------------------------------------
// Slot storage s in [0, S_max) holds scenario slot_scen[s] (global id, -1: free).  Between two chunks of iterations (after k_compact:
// running storages in front of the slot list, their count in *count): every storage that is not running and still holds a scenario has
// met the stop rule -> harvest list; every free storage takes the next pending scenario -> new list, appended to the slot list.
// One workgroup; the storage table sits in LDS and one thread walks it in order (deterministic assignment).
__global__ __launch_bounds__(1024) void k_queue_refill(int S_max, int n_total, int* __restrict__ active, int* __restrict__ count,
                                                        int* __restrict__ slot_scen, int* __restrict__ next, int* __restrict__ hlist,
                                                        int* __restrict__ hg, int* __restrict__ newlist, int* __restrict__ base_out) {
    extern __shared__ int q_lds[];                      // [S_max] busy | [S_max] scenario of the storage
    int* busy = q_lds;
    int* scen = q_lds + S_max;
    const int tid = threadIdx.x, cnt = *count;
    for (int s = tid; s < S_max; s += 1024) {
        busy[s] = 0;
        scen[s] = slot_scen[s];
        hlist[s] = -1;
        newlist[s] = -1;
    }
    __syncthreads();
    for (int i = tid; i < cnt; i += 1024) busy[active[i]] = 1;
    __syncthreads();
    if (tid == 0) {
        int nh = 0, nn = 0, nx = *next;
        for (int s = 0; s < S_max; ++s) {
            if (busy[s]) continue;
            if (scen[s] >= 0) {
                hlist[nh] = s;
                hg[nh] = scen[s];
                ++nh;
                scen[s] = -1;
            }
            if (nx < n_total) {
                scen[s] = nx++;
                newlist[nn] = s;
                active[cnt + nn] = s;
                ++nn;
            }
        }
        *next = nx;
        *base_out = cnt;
        *count = cnt + nn;
    }
    __syncthreads();
    for (int s = tid; s < S_max; s += 1024) slot_scen[s] = scen[s];
}

// result record (k_stats) and, if asked for, the raw voltages in the ABI's stacked order q*n + i of every harvested storage -> the
// per-scenario outputs of the sweep
__global__ void k_queue_harvest(int n, int Hn, double thresh, int max_iter, const int* __restrict__ hlist, const int* __restrict__ hg,
                                const double* __restrict__ Vm, const double* __restrict__ Va, const double* __restrict__ err,
                                const int* __restrict__ niter, const int* __restrict__ pivflag, int start_bit, hpf_stat* __restrict__ qstats,
                                double* __restrict__ qVm, double* __restrict__ qVa) {
    const int s = hlist[blockIdx.x];
    if (s < 0) return;
    const int g = hg[blockIdx.x];
    const double* V = Vm + (size_t)s * n * Hn;
    const double* A = Va + (size_t)s * n * Hn;
    double best = 0.0;
    bool nan = false;
    for (int b = threadIdx.x; b < n; b += TPB) {
        double hs = 0.0;
        for (int q = 1; q < Hn; ++q) hs = hs + V[(size_t)b * Hn + q] * V[(size_t)b * Hn + q];
        const double t = sqrt(hs) / fabs(V[(size_t)b * Hn]);
        if (t != t) nan = true;
        best = t > best ? t : best;
    }
    unsigned long long bits = nan ? 0x7ff8000000000000ull : (unsigned long long)__double_as_longlong(best);
    bits = wave_max_u64(bits);
    __shared__ unsigned long long red[TPB / 64];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = bits;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long r = red[0];
        for (int w = 1; w < TPB / 64; ++w) r = red[w] > r ? red[w] : r;
        hpf_stat st;
        st.n_iter = niter[s];
        const double e = err[s];
        st.err = e;
        const int pf = pivflag[s];
        st.flags = (e <= thresh ? 1 : 0) | ((niter[s] >= max_iter && !(e <= thresh)) ? 2 : 0) | ((e != e || isinf(e)) ? 4 : 0) |
                   ((pf & 1) ? 8 : 0) | ((pf & 4) ? 32 : 0) | resid_flag_bits(pf) | start_bit;
        st.thd_max = __longlong_as_double((long long)r);
        qstats[g] = st;
    }
    if (qVm) {
        double* om = qVm + (size_t)g * n * Hn;
        double* oa = qVa + (size_t)g * n * Hn;
        for (int k = threadIdx.x; k < n * Hn; k += TPB) {       // k = q*n + i (coalesced stores), source bus-major
            const int q = k / n, i = k - q * n;
            om[k] = V[(size_t)i * Hn + q];
            oa[k] = A[(size_t)i * Hn + q];
        }
    }
}

// Distortion accumulator: the finished scenarios of a list (hpf_accum.hpp: the list, id and classification rules) are folded into the per-entry
// statistics (hpf_distortion.hpp).  One thread owns one entry -- t < n*Hn: x of (bus, harmonic position) = t (bus-major like the state:
// consecutive threads read consecutive doubles and share the bus's fundamental), t < n*Hn + n: the THD of a bus and its histogram row,
// t = n*Hn + n: the three scenario counters -- and walks the list in order: plain loads and stores, no atomics, max / arg / counters independent
// of the order in which scenarios arrive.  acc_f [3][T] max | sum | sumsq, acc_arg [T], acc_u [T] over | [n][B + 1] histogram.
__global__ void k_distortion_add(int n, int Hn, AccumList list, const double* __restrict__ Vm, const double* __restrict__ limit, double thd_limit,
                                 double hist_max, double inv_w, int B, double* __restrict__ acc_f, int* __restrict__ acc_arg,
                                 uint32_t* __restrict__ acc_u, long long* __restrict__ cnt) {
    const int E = n * Hn, T = E + n;
    const int t = blockIdx.x * TPB + threadIdx.x;
    if (t > T) return;
    if (t == T) return accum_count(list, cnt);
    const int bus = t < E ? t / Hn : t - E, q = t < E ? t - bus * Hn : 0;
    const double lim = t < E ? limit[q] : thd_limit;
    AccumSlot st;
    st.load(acc_f, acc_arg, acc_u, 0, T, t);
    uint32_t* hist = acc_u + (size_t)T + (size_t)bus * (B + 1);
    const bool any = accum_walk(list, [&](int s, int id) {
        const double* Vbus = Vm + (size_t)s * E + (size_t)bus * Hn;
        const double x = t < E ? dist_x(Vbus, q) : dist_thd(Vbus, Hn);
        st.fold(x, id, lim);
        if (t >= E) {
            const int b = dist_bin(x, hist_max, inv_w, B);
            hist[b] = hist[b] + 1u;
        }
    });
    if (any) st.store(acc_f, acc_arg, acc_u, 0, T, t);
}

// U alone from (Vm, Va): hpf_branch_flows evaluates at the handle's current state, and hpf_set_state uploads Vm / Va only (E is left as the
// last solver kernel wrote it -- fund_pf and the harmonic NR normalise it differently)
__global__ void k_branch_refresh_u(int count, const double* __restrict__ Vm, const double* __restrict__ Va, cplx* __restrict__ U) {
    const int k = blockIdx.x * TPB + threadIdx.x;
    if (k >= count) return;
    const size_t o = (size_t)blockIdx.y * count + k;
    cplx u, e;
    polar<false>(Vm[o], Va[o], u, e);
    U[o] = u;
}

// Branch flows of every scenario of the batch (hpf_branch.hpp).  Workgroup (tile, scenario): BRANCH_TILE consecutive branches.  Lanes run over q
// within a branch (item t = e_local * Hn + q), so the runs U[i][0..Hn), U[j][0..Hn) and yb[e][0..Hn) are read as whole lines; I, |I|^2 and the
// loss go to LDS; then ONE lane per branch forms the ascending-q sums, one lane per q the tile's share of loss_h (ascending e), and I leaves
// transposed through LDS in the ABI's stacked order [Hn][nb] (e fastest: runs of BRANCH_TILE x 16 bytes).  Any output pointer may be NULL.
__global__ void k_branch_flows(int nb, int Hn, int n, int tiles, const int* __restrict__ from, const int* __restrict__ to,
                               const cplx* __restrict__ yb, const cplx* __restrict__ U, cplx* __restrict__ I, double* __restrict__ irms,
                               double* __restrict__ thd_i, double* __restrict__ loss, double* __restrict__ loss_harm, double* __restrict__ part) {
    extern __shared__ __align__(16) unsigned char br_lds[];
    cplx* sI = reinterpret_cast<cplx*>(br_lds);
    double* si2 = reinterpret_cast<double*>(sI + (size_t)BRANCH_TILE * Hn);
    double* sl = si2 + (size_t)BRANCH_TILE * Hn;
    const int tile = blockIdx.x, s = blockIdx.y, e0 = tile * BRANCH_TILE;
    const int ne = nb - e0 < BRANCH_TILE ? nb - e0 : BRANCH_TILE;
    const cplx* Us = U + (size_t)s * n * Hn;
    for (int t = threadIdx.x; t < ne * Hn; t += TPB) {
        const int el = t / Hn, q = t - el * Hn, e = e0 + el;
        const cplx y = yb[(size_t)e * Hn + q], ui = Us[(size_t)from[e] * Hn + q], uj = Us[(size_t)to[e] * Hn + q];
        const cplx c = branch_current(y, ui, uj);
        sI[t] = c;
        si2[t] = branch_abs2(c);
        sl[t] = branch_loss(y, ui, uj);
    }
    __syncthreads();
    if ((int)threadIdx.x < ne) {
        const int el = threadIdx.x;
        BranchSums a;
        branch_sums_start(a);
        for (int q = 0; q < Hn; ++q) branch_sums_step(a, q, si2[el * Hn + q], sl[el * Hn + q]);
        const size_t o = (size_t)s * nb + e0 + el;
        if (irms) irms[o] = branch_irms(a);
        if (thd_i) thd_i[o] = branch_thd_i(a);
        if (loss) loss[o] = a.loss_all;
        if (loss_harm) loss_harm[o] = a.loss_harm;
    }
    if (part)
        for (int q = threadIdx.x; q < Hn; q += TPB) {
            double a = 0.0;
            for (int el = 0; el < ne; ++el) a = a + sl[el * Hn + q];
            part[((size_t)s * tiles + tile) * Hn + q] = a;
        }
    if (I)
        for (int t = threadIdx.x; t < ne * Hn; t += TPB) {
            const int q = t / ne, el = t - q * ne;
            I[((size_t)s * Hn + q) * nb + e0 + el] = sI[el * Hn + q];
        }
}

// loss_h[s][q] = the tile sums of k_branch_flows in ascending tile order (one thread per (scenario, q): the fixed order of hpf_branch.hpp)
__global__ void k_branch_loss_h(int Hn, int tiles, const double* __restrict__ part, double* __restrict__ loss_h) {
    const int s = blockIdx.y, q = blockIdx.x * TPB + threadIdx.x;
    if (q >= Hn) return;
    double a = 0.0;
    for (int t = 0; t < tiles; ++t) a = a + part[((size_t)s * tiles + t) * Hn + q];
    loss_h[(size_t)s * Hn + q] = a;
}

// Branch statistics accumulator: the finished scenarios of a list (hpf_accum.hpp: the list, id and classification rules) are folded into the
// per-branch statistics of irms, loss and harmonic loss.  One thread owns branch t (t = nb: the three scenario counters), walks the list in order
// and forms each scenario's ascending-q sums itself (branch_fold): plain loads and stores, no atomics, so max / arg / over / counters do not
// depend on the order in which scenarios arrive.  Workgroups of 64: the nb owners spread over nb / 64 compute units.
// acc_f [9][nb], acc_arg [3][nb]: quantities irms, loss, harmonic loss; acc_over [nb]: irms alone has a limit, the rating.
constexpr int BR_TPB = 64;
__global__ __launch_bounds__(BR_TPB) void k_branch_add(int nb, int Hn, int n, AccumList list, const cplx* __restrict__ U, const int* __restrict__ from,
                                                       const int* __restrict__ to, const cplx* __restrict__ yb, const double* __restrict__ rating,
                                                       double* __restrict__ acc_f, int* __restrict__ acc_arg, uint32_t* __restrict__ acc_over,
                                                       long long* __restrict__ cnt) {
    const int t = blockIdx.x * BR_TPB + threadIdx.x;
    if (t > nb) return;
    if (t == nb) return accum_count(list, cnt);
    AccumSlot st[3];
    for (int k = 0; k < 3; ++k) st[k].load(acc_f, acc_arg, k == 0 ? acc_over : nullptr, k, nb, t);
    const double lim = rating[t];
    const cplx* y = yb + (size_t)t * Hn;
    const size_t oi = (size_t)from[t] * Hn, oj = (size_t)to[t] * Hn;
    const bool any = accum_walk(list, [&](int s, int id) {
        const cplx* Us = U + (size_t)s * n * Hn;
        double irms, thd_i, loss_e, loss_harm;
        branch_fold(y, Us + oi, Us + oj, Hn, irms, thd_i, loss_e, loss_harm);
        st[0].fold(irms, id, lim);
        branch_stat_fold(loss_e, id, st[1].max, st[1].arg, st[1].sum, st[1].sumsq);
        branch_stat_fold(loss_harm, id, st[2].max, st[2].arg, st[2].sum, st[2].sumsq);
    });
    if (!any) return;
    for (int k = 0; k < 3; ++k) st[k].store(acc_f, acc_arg, k == 0 ? acc_over : nullptr, k, nb, t);
}

// Voltage waveforms (hpf_waveform.hpp): the T samples of v(t) at a bus, their peak (value, sample), crest factor and sampling slack.
// Workgroup (4 buses, list entry): one wavefront per (scenario, bus).  The scenario list is the accumulators' (hpf_accum.hpp; id_base unused): a
// negative slot: nothing to do (as k_queue_harvest relies on); with `stats` given, a scenario the accumulator would not add is not evaluated
// either.  buslist NULL: buses 0 .. nbus - 1.
// The table ct | st is staged in LDS once per workgroup: 16 T bytes, and LDS decides the occupancy -- T <= 1024: 16 KiB or less, the 8 workgroups
// (32 waves) a CU can hold fit; T = 2048: 32 KiB -> 5 workgroups; T = 4096: 64 KiB -> 2 workgroups = 2 waves per SIMD.
// Lane l evaluates the samples k = l, l + 64, ... in chunks of C per lane (C accumulators in registers), the harmonics in the OUTER loop, so each
// sample's sum still runs over ascending q from 0.0 and the bus's U[q] and orders[q] are wave-uniform loads, once per chunk.  The 32 lanes of
// an LDS lane group read the table at stride orders[q] doubles: a permutation of the 32 eight-byte banks for every ODD order (all orders of this
// project's harmonic sets are odd) -- conflict-free; an even order 2^e m maps 2^e lanes onto one bank: correct, 2^e times slower on that term.
// Reduction of (|v| key, k) over the wave by shuffles with the total order of wave_peak_combine; lane 0 writes.  v (optional): every lane stores
// its samples, [list entry's storage][b][T].  No atomics.
constexpr int WV_TPB = 256, WV_BUSES = WV_TPB / 64;
template <int C>
__global__ __launch_bounds__(WV_TPB) void k_wave_peaks(int n, int Hn, int T, int nbus, const int* __restrict__ buslist, AccumList list,
                                                       const cplx* __restrict__ U, const int* __restrict__ orders, const double* __restrict__ ct,
                                                       const double* __restrict__ st, double* __restrict__ v, double* __restrict__ peak,
                                                       int* __restrict__ kpeak, double* __restrict__ crest, double* __restrict__ slack) {
    extern __shared__ __align__(16) unsigned char wv_lds[];
    double* lc = reinterpret_cast<double*>(wv_lds);
    double* ls = lc + T;
    const AccumEntry e = list.entry(blockIdx.y);
    const int s = e.slot;
    if (s < 0 || e.cls != DIST_ADD) return;              // (the whole workgroup: before the barrier)
    for (int j = threadIdx.x; j < T; j += WV_TPB) {
        lc[j] = ct[j];
        ls[j] = st[j];
    }
    __syncthreads();
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int b = blockIdx.x * WV_BUSES + w;
    if (b >= nbus) return;
    const int bus = buslist ? buslist[b] : b;
    const cplx* Ub = U + ((size_t)s * n + bus) * Hn;
    const int mask = T - 1;
    uint64_t key = 0;                                    // (|v| = 0 at k = lane: never beats the lane's first sample)
    int kbest = lane;
    for (int c0 = 0; c0 < T / 64; c0 += C) {
        double acc[C];
#pragma unroll
        for (int i = 0; i < C; ++i) acc[i] = 0.0;
        const int k0 = lane + 64 * c0;
        for (int q = 0; q < Hn; ++q) {
            const cplx u = Ub[q];
            const int h = orders[q];
            int j = h * k0;                              // (h <= 32767, k < 4096: below 2^27)
            const int step = h * 64;
#pragma unroll
            for (int i = 0; i < C; ++i) {
                const int jj = j & mask;                 // = wave_phase(h, k0 + 64 i, T)
                acc[i] = acc[i] + wave_term(u, lc[jj], ls[jj]);
                j += step;
            }
        }
#pragma unroll
        for (int i = 0; i < C; ++i) {
            const int k = k0 + 64 * i;
            if (v) v[((size_t)s * nbus + b) * T + k] = acc[i];
            wave_peak_combine(key, kbest, wave_key(acc[i]), k);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long key2 = __shfl_xor((unsigned long long)key, off, 64);
        const int k2 = __shfl_xor(kbest, off, 64);
        wave_peak_combine(key, kbest, (uint64_t)key2, k2);
    }
    if (lane != 0) return;
    const size_t o = (size_t)s * n + bus;
    const double pk = wave_key_value(key);
    if (peak) peak[o] = pk;
    if (kpeak) kpeak[o] = kbest;
    if (crest) crest[o] = wave_crest(pk, wave_sumsq(Ub, Hn));
    if (slack) slack[o] = wave_slack(Ub, orders, Hn, T);
}

// Waveform statistics accumulator, the twin of k_branch_add: one thread owns bus t (t = n: the three scenario counters), walks the list in order
// and folds the peak and the crest factor k_wave_peaks left in the handle's scratch [storage][n] (same list, hpf_accum.hpp): plain loads and
// stores, no atomics.  acc_f [6][n], acc_arg, acc_over [2][n]: quantities peak, crest.
__global__ __launch_bounds__(BR_TPB) void k_wave_add(int n, AccumList list, const double* __restrict__ peak, const double* __restrict__ crest,
                                                     const double* __restrict__ peak_limit, double crest_limit, double* __restrict__ acc_f,
                                                     int* __restrict__ acc_arg, uint32_t* __restrict__ acc_over, long long* __restrict__ cnt) {
    const int t = blockIdx.x * BR_TPB + threadIdx.x;
    if (t > n) return;
    if (t == n) return accum_count(list, cnt);
    AccumSlot st[2];
    for (int k = 0; k < 2; ++k) st[k].load(acc_f, acc_arg, acc_over, k, n, t);
    const double lim = peak_limit[t];
    const bool any = accum_walk(list, [&](int s, int id) {
        const size_t o = (size_t)s * n + t;
        st[0].fold(peak[o], id, lim);
        st[1].fold(crest[o], id, crest_limit);
    });
    if (!any) return;
    for (int k = 0; k < 2; ++k) st[k].store(acc_f, acc_arg, acc_over, k, n, t);
}

// a new scenario moves into every storage of the new list: loads, the reference's start (HG:174-184) with the fundamental entries from
// its power-flow seed, U / E, counters
__global__ void k_queue_init(int n, int Hn, const int* __restrict__ newlist, const int* __restrict__ slot_scen, const double* __restrict__ qP,
                             const double* __restrict__ qQ, const double* __restrict__ seedVm, const double* __restrict__ seedVa,
                             double* __restrict__ P, double* __restrict__ Q, double* __restrict__ Vm, double* __restrict__ Va,
                             cplx* __restrict__ U, cplx* __restrict__ E, int* __restrict__ niter, int* __restrict__ pivflag) {
    const int s = newlist[blockIdx.y];
    if (s < 0) return;
    const int g = slot_scen[s];
    const int k = blockIdx.x * TPB + threadIdx.x;
    if (k >= n * Hn) return;
    const int i = k / Hn, q = k - i * Hn;
    const size_t o = (size_t)s * n * Hn + k;
    const double vm = q == 0 ? seedVm[(size_t)g * n + i] : 0.1, va = q == 0 ? seedVa[(size_t)g * n + i] : 0.0;
    Vm[o] = vm;
    Va[o] = va;
    cplx u, e;
    polar<false>(vm, va, u, e);
    U[o] = u;
    E[o] = e;
    if (q == 0) {
        P[(size_t)s * n + i] = qP[(size_t)g * n + i];
        Q[(size_t)s * n + i] = qQ[(size_t)g * n + i];
    }
    if (k == 0) {
        niter[s] = 0;
        pivflag[s] = 0;
    }
}

// ... with a start state set: the same move-in with Vm, Va, U, E copied from the start state (no power-flow seed)
__global__ void k_queue_init_start(int n, int Hn, const int* __restrict__ newlist, const int* __restrict__ slot_scen, const double* __restrict__ qP,
                                   const double* __restrict__ qQ, const double* __restrict__ sVm, const double* __restrict__ sVa,
                                   const cplx* __restrict__ sU, const cplx* __restrict__ sE, double* __restrict__ P, double* __restrict__ Q,
                                   double* __restrict__ Vm, double* __restrict__ Va, cplx* __restrict__ U, cplx* __restrict__ E,
                                   int* __restrict__ niter, int* __restrict__ pivflag) {
    const int s = newlist[blockIdx.y];
    if (s < 0) return;
    const int g = slot_scen[s];
    const int k = blockIdx.x * TPB + threadIdx.x;
    if (k >= n * Hn) return;
    const int i = k / Hn, q = k - i * Hn;
    const size_t o = (size_t)s * n * Hn + k;
    Vm[o] = sVm[k];
    Va[o] = sVa[k];
    U[o] = sU[k];
    E[o] = sE[k];
    if (q == 0) {
        P[(size_t)s * n + i] = qP[(size_t)g * n + i];
        Q[(size_t)s * n + i] = qQ[(size_t)g * n + i];
    }
    if (k == 0) {
        niter[s] = 0;
        pivflag[s] = 0;
    }
}

// Source currents, input form 1 -> slot storage (hpf_sources.hpp): one thread per (scenario, nonlinear bus, harmonic position).  ab [.][nnl][2] =
// (a, phi) per (scenario, nonlinear bus), orders [Hn], dst [S_max][nnl][Hn].  Without lists (newlist == nullptr): scenario blockIdx.y of the batch
// reads row g0 + blockIdx.y of ab (hpf_set_sources: g0 = 0; the waves of hpf_solve_queue: their first scenario).  With lists: storage
// s = newlist[blockIdx.y] takes scenario slot_scen[s] of the queue (the freed slots of hpf_solve_queue, next to k_queue_init).
__global__ void k_source_expand(int nnl, int Hn, int m, const int* __restrict__ newlist, const int* __restrict__ slot_scen, int g0,
                                const double* __restrict__ ab, const int* __restrict__ orders, const int* __restrict__ dev,
                                const cplx* __restrict__ IN, cplx* __restrict__ dst) {
    const int s = newlist ? newlist[blockIdx.y] : (int)blockIdx.y;
    if (s < 0) return;
    const int g = newlist ? slot_scen[s] : g0 + (int)blockIdx.y;
    const int k = blockIdx.x * TPB + threadIdx.x;
    if (k >= nnl * Hn) return;
    const int ib = k / Hn, q = k - ib * Hn;
    const double2 v = reinterpret_cast<const double2*>(ab)[(size_t)g * nnl + ib];
    dst[(size_t)s * nnl * Hn + k] = source_expand(v.x, v.y, orders[q], IN[(size_t)dev[m + ib] * Hn + q]);
}

// ... and input form 0: the queue's array in HBM [n_total][nnl][Hn] -> the storages of the new list
__global__ void k_source_gather(int count, const int* __restrict__ newlist, const int* __restrict__ slot_scen, const cplx* __restrict__ qsrc,
                                cplx* __restrict__ dst) {
    const int s = newlist[blockIdx.y];
    if (s < 0) return;
    const int g = slot_scen[s];
    const int k = blockIdx.x * TPB + threadIdx.x;
    if (k >= count) return;
    dst[(size_t)s * count + k] = qsrc[(size_t)g * count + k];
}

// the initial mismatch of the new scenarios against the stop rule (HG:531,536): a scenario that meets it at once leaves the slot list
__global__ __launch_bounds__(64) void k_queue_first(int S_max, double thresh, int max_iter, const int* __restrict__ newlist, const int* __restrict__ base,
                              const unsigned long long* __restrict__ errpart, int pstride, int np, double* __restrict__ err,
                              int* __restrict__ active) {
    const int idx = blockIdx.x;                          // one wavefront per entry of the new list
    if (idx >= S_max) return;
    const int s = newlist[idx];
    if (s < 0) return;
    const double e = __longlong_as_double((long long)slot_err_bits(errpart + (size_t)s * pstride, np));
    if (threadIdx.x != 0) return;
    err[s] = e;
    if (!((e > thresh) && (0 < max_iter))) active[*base + idx] = -1;
}

// fundamental entries (harmonic position 0) of the first S scenarios' voltages -> seed arrays of scenarios g0 .. g0 + S - 1
__global__ void k_queue_keep_seed(int n, int Hn, int g0, const double* __restrict__ Vm, const double* __restrict__ Va,
                                  double* __restrict__ seedVm, double* __restrict__ seedVa) {
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const size_t o = (size_t)blockIdx.y * n * Hn + (size_t)i * Hn;
    seedVm[(size_t)(g0 + blockIdx.y) * n + i] = Vm[o];
    seedVa[(size_t)(g0 + blockIdx.y) * n + i] = Va[o];
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------------
namespace {

inline dim3 grid2(int count, int S) { return dim3((unsigned)((count + TPB - 1) / TPB), (unsigned)S, 1); }

int ensure_dense(hpf_handle* h, int Nsys) {
    size_t want = (size_t)Nsys * Nsys;                         // (N * N >= 2^31: rocSOLVER's 64-bit entry points, dense_solve)
    if (h->solver == HPF_SOLVER_DENSE && (size_t)h->N * h->N > want) want = (size_t)h->N * h->N;
    if (h->d_J && h->J_elems_per_scen >= want) return HPF_OK;
    h->dense_mem.clear();
    const int Nmax = h->N > h->Nf ? h->N : h->Nf;
    int r;
    if ((r = h->dense_mem.alloc(&h->d_J, want * (size_t)h->S_max)) ||
        (r = h->dense_mem.alloc(&h->d_ipiv, 2 * (size_t)Nmax * h->S_max)) ||          // (room for the int64 pivots of the 64-bit path)
        (r = h->dense_mem.alloc(&h->d_info, 2 * (size_t)h->S_max))) {
        h->dense_mem.clear();
        return r;
    }
    HIPCHK(hipMemset(h->d_info, 0, sizeof(int) * 2 * h->S_max));
    h->J_elems_per_scen = want;
    return HPF_OK;
}

int resolve_spans(hpf_handle* h) {
    if (h->spans.empty() && h->ts_next == 0) return HPF_OK;
    HIPCHK(hipStreamSynchronize(h->stream));
    for (auto& sp : h->spans) {
        float ms = 0.f;
        hipEventElapsedTime(&ms, sp.e0, sp.e1);
        h->t_ms[sp.which] += ms;
        h->t_n[sp.which] += 1;
        hipEventDestroy(sp.e0);
        hipEventDestroy(sp.e1);
    }
    h->spans.clear();
    if (h->d_tstamp && h->ts_next > 0) {              // device-clock durations of the stamped general-factor-kernel launches
        std::vector<unsigned long long> ts(2 * (size_t)h->ts_next);
        HIPCHK(hipMemcpy(ts.data(), h->d_tstamp, sizeof(unsigned long long) * ts.size(), hipMemcpyDeviceToHost));
        int khz = 100000;
        hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, h->device);
        for (int i = 0; i < h->ts_next; ++i)
            if (ts[2 * i + 1] > ts[2 * i] && ts[2 * i] != ~0ull) {
                h->t_ms[T_GJ_DEV] += (double)(ts[2 * i + 1] - ts[2 * i]) / (double)khz;
                h->t_n[T_GJ_DEV] += 1;
            }
        h->ts_next = 0;
        std::vector<unsigned long long> init(2 * (size_t)hpf_handle::TS_CAP);
        for (size_t i = 0; i < init.size(); i += 2) {
            init[i] = ~0ull;
            init[i + 1] = 0ull;
        }
        HIPCHK(hipMemcpy(h->d_tstamp, init.data(), sizeof(unsigned long long) * init.size(), hipMemcpyHostToDevice));
    }
    return HPF_OK;
}


// U, E of the whole batch from its polar state (always every scenario, on the handle's stream)
template <bool FUND>
int launch_polar(hpf_handle* h) {
    const int count = FUND ? h->n : h->n * h->Hn;
    hipLaunchKernelGGL((k_polar<FUND>), grid2(count, h->S), dim3(TPB), 0, h->stream, count, h->n * h->Hn, h->Hn, h->d_Vm,
                       h->d_Va, h->d_U, h->d_E);
    return launch_status(h);
}

// the Newton step of the multi-wave block-tree sweep works on bus-major images of the mismatch and of the step
static bool bus_images(const hpf_handle* h) { return h->solver == HPF_SOLVER_BLOCK_TREE && h->has_ctree && h->gj_mode == 1; }
static int tree_bst(const hpf_handle* h) { const int b = 2 * h->Hn; return b <= 12 ? 12 : (b <= 28 ? 28 : (b <= 52 ? 52 : (b <= 100 ? 100 : b))); }   // = wave_block_size, or b

// partial maxima a mismatch launch leaves per scenario (one per wavefront of its workgroups): fundamental pf / harmonic mismatch
template <bool FUND>
static int err_parts(const hpf_handle* h) { return (TPB / 64) * (((FUND ? h->n : h->n * h->Hn) + TPB - 1) / TPB); }

// stacked: also write the mismatch in the reference's stacked order (C ABI, dense solver, single-wave / generic tree kernels)
template <bool FUND>
int launch_mismatch(hpf_handle* h, const LaunchCtx& ctx, bool stacked = true) {
    ScopedTimer t(h, T_MISMATCH, ctx.stream);
    const int count = FUND ? h->n : h->n * h->Hn;
    const int N = FUND ? h->Nf : h->N;
    const int Nc = FUND ? h->n - 1 : h->Nc;
    const bool img = !FUND && h->d_fb && bus_images(h);
    if (count > 1) {
        const int nbx = (count + TPB - 1) / TPB;
        // LDS: Y_N^T of one device type + the voltages of the workgroup's tile of buses (harmonic mismatch with coupled Norton data)
        const size_t lds = (!FUND && h->coupled && h->n > h->m)
                               ? sizeof(cplx) * ((size_t)h->Hn * h->Hn + (size_t)(TPB / h->Hn + 2) * h->Hn) : 0;
        // the batch has sources (hpf_set_sources): the source variant of the harmonic kernel; without them exactly the launch of a handle that never had any
        auto kern = (!FUND && h->src_set) ? &k_mismatch<false, true> : &k_mismatch<FUND, false>;
        if (lds > 64 * 1024) {                      // Hn >= 62 (H_MAX >= 123): beyond the default dynamic-LDS limit of a kernel
            if (lds > 160 * 1024) return HPF_E_ARG;
            // (per launch: the attribute belongs to the device the handle runs on, and the call costs nothing next to the launch)
            HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        }
        hipLaunchKernelGGL(kern, xcd_grid(nbx, ctx.S), dim3(TPB), lds, ctx.stream, h->M, count, N, Nc,
                           ctx.active, h->d_U, h->d_P, h->d_Q, (stacked || !img) ? h->d_f : nullptr, h->d_errpart, h->errpart_stride, h->d_I0,
                           img ? h->d_fb : nullptr, tree_bst(h), ctx.s0, ctx.S, div_magic(h->Hn),
                           (!FUND && h->src_set) ? h->d_src : (const cplx*)nullptr);
        if (launch_status(h)) return HPF_E_HIP;
    }
    return HPF_OK;
}

template <bool FUND>
int launch_jacobian_dense(hpf_handle* h, const LaunchCtx& ctx) {
    ScopedTimer t(h, T_JACOBIAN, ctx.stream);
    const int N = FUND ? h->Nf : h->N;
    const int Nc = FUND ? h->n - 1 : h->Nc;
    // (the dense solver never runs in scenario groups: its slice is the whole batch, ctx.s0 == 0)
    HIPCHK(hipMemsetAsync(h->d_J, 0, sizeof(double) * h->J_elems_per_scen * (size_t)ctx.S, ctx.stream));
    const int total = (FUND ? 1 : h->Hn) * h->nnz;
    hipLaunchKernelGGL((k_jac_dense<FUND>), grid2(total, ctx.S), dim3(TPB), 0, ctx.stream, h->M, total, N, Nc,
                       h->J_elems_per_scen, ctx.active, h->d_erow, h->d_U, h->d_E, h->d_J);
    if (launch_status(h)) return HPF_E_HIP;
    if (!FUND && h->coupled && h->n > h->m) {
        const int tot = (h->n - h->m) * h->Hn * h->Hn;
        hipLaunchKernelGGL(k_jac_cross_dense, grid2(tot, ctx.S), dim3(TPB), 0, ctx.stream, h->M, tot, N, Nc,
                           h->J_elems_per_scen, ctx.active, h->d_U, h->d_E, h->d_J);
        if (launch_status(h)) return HPF_E_HIP;
    }
    return HPF_OK;
}

// f <- J^{-1} f for every scenario (rocSOLVER LU with partial pivoting)
int dense_solve(hpf_handle* h, int Nsys) {
    ScopedTimer t(h, T_SOLVE, h->stream);
    if (Nsys <= 0) return HPF_OK;
    if (ensure_blas(h)) return HPF_E_ROCSOLVER;
    BLASCHK(rocblas_set_stream(h->blas, h->stream));
    if ((long long)Nsys * Nsys >= (1ll << 31)) {
        // beyond 32-bit element offsets (N > 46 340, e.g. the 1 000-bus x 26-harmonic feeder as a dense system: 21.6 GB per scenario):
        // rocSOLVER's 64-bit entry points, one scenario after the other; int64 pivots / info (check_info reads them as such)
        const int Nmax = h->N > h->Nf ? h->N : h->Nf;
        int64_t* ip = reinterpret_cast<int64_t*>(h->d_ipiv);
        int64_t* inf = reinterpret_cast<int64_t*>(h->d_info);
        for (int sc = 0; sc < h->S; ++sc) {
            double* Js = h->d_J + (size_t)sc * h->J_elems_per_scen;
            BLASCHK(rocsolver_dgetrf_64(h->blas, Nsys, Nsys, Js, Nsys, ip + (size_t)sc * Nmax, inf + sc));
            BLASCHK(rocsolver_dgetrs_64(h->blas, rocblas_operation_none, Nsys, 1, Js, Nsys, ip + (size_t)sc * Nmax, h->d_f + (size_t)sc * Nsys, Nsys));
        }
        h->info64 = true;
        return HPF_OK;
    }
    h->info64 = false;
    if (h->S == 1) {
        BLASCHK(rocsolver_dgetrf(h->blas, Nsys, Nsys, h->d_J, Nsys, h->d_ipiv, h->d_info));
        BLASCHK(rocsolver_dgetrs(h->blas, rocblas_operation_none, Nsys, 1, h->d_J, Nsys, h->d_ipiv, h->d_f, Nsys));
    } else {
        const rocblas_stride sA = (rocblas_stride)h->J_elems_per_scen;
        const int Nmax = h->N > h->Nf ? h->N : h->Nf;
        const rocblas_stride sF = (rocblas_stride)Nsys;
        BLASCHK(rocsolver_dgetrf_strided_batched(h->blas, Nsys, Nsys, h->d_J, Nsys, sA, h->d_ipiv, Nmax, h->d_info, h->S));
        BLASCHK(rocsolver_dgetrs_strided_batched(h->blas, rocblas_operation_none, Nsys, 1, h->d_J, Nsys, sA, h->d_ipiv,
                                                 Nmax, h->d_f, Nsys, sF, h->S));
    }
    return HPF_OK;
}

template <bool FUND>
int launch_update(hpf_handle* h, const LaunchCtx& ctx) {
    ScopedTimer t(h, T_UPDATE, ctx.stream);
    const int count = FUND ? h->n : h->n * h->Hn;
    const int N = FUND ? h->Nf : h->N;
    const int Nc = FUND ? h->n - 1 : h->Nc;
    const bool busx = !FUND && bus_images(h);
    const int bw = tree_bst(h);
    if (!FUND && h->rect_update)
        hipLaunchKernelGGL(k_update_rect, grid2(count, ctx.S), dim3(TPB), 0, ctx.stream, h->n, h->Hn, h->c, count,
                           h->n * h->Hn, N, Nc, ctx.active, h->d_f, h->d_Vm, h->d_Va, h->d_U, h->d_E,
                           busx ? h->d_x : nullptr, bw, ctx.s0, div_magic(h->Hn));
    else
        hipLaunchKernelGGL((k_update<FUND>), grid2(count, ctx.S), dim3(TPB), 0, ctx.stream, h->n, h->Hn, h->c, count,
                           h->n * h->Hn, N, Nc, ctx.active, h->d_f, h->d_Vm, h->d_Va, h->d_U, h->d_E,
                           busx ? h->d_x : nullptr, bw, ctx.s0, div_magic(h->Hn));
    return launch_status(h);
}

// eta of no step yet, for every slot (hpf_solve entry, hpf_set_state, switching the check on)
int reset_step_eta(hpf_handle* h) {
    if (!h->d_eta) return HPF_OK;
    const size_t S = (size_t)h->S_alloc;
    hipLaunchKernelGGL(k_fill, dim3((unsigned)((S + TPB - 1) / TPB)), dim3(TPB), 0, h->stream, h->d_eta, S, (double)NAN);
    hipLaunchKernelGGL(k_fill, dim3((unsigned)((S + TPB - 1) / TPB)), dim3(TPB), 0, h->stream, h->d_eta + S, S, -1.0);
    return launch_status(h);
}

// LDS of k_step_residual: Y_N^T of one device type + U, E and the step of the workgroup's tile of buses; 0: nothing to stage (uncoupled, no
// nonlinear bus) or beyond what a workgroup can have -- the kernel then reads every operand from memory
static size_t step_residual_lds(const hpf_handle* h) {
    if (!(h->coupled && h->n > h->m)) return 0;
    const size_t lds = sizeof(cplx) * ((size_t)h->Hn * h->Hn + 3 * (size_t)(TPB / h->Hn + 2) * h->Hn);
    return lds > 160 * 1024 ? 0 : lds;
}

// The residual check of the step newton_step just left (in d_x or d_f, as launch_update will read it), before the update moves the state.
int launch_step_residual(hpf_handle* h, const LaunchCtx& ctx) {
    ScopedTimer t(h, T_RESID, ctx.stream);
    const int count = h->n * h->Hn;
    if (count <= 1) return HPF_OK;
    const bool busx = bus_images(h);
    const int nbx = (count + TPB - 1) / TPB;
    const size_t lds = step_residual_lds(h);
    auto kern = h->src_set ? (busx ? &k_step_residual<true, true> : &k_step_residual<false, true>)
                           : (busx ? &k_step_residual<true, false> : &k_step_residual<false, false>);
    if (lds > 64 * 1024)        // beyond the default dynamic-LDS limit of a kernel (as launch_mismatch)
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    hipLaunchKernelGGL(kern, xcd_grid(nbx, ctx.S), dim3(TPB), lds, ctx.stream, h->M, count, h->N, h->Nc, ctx.active, h->d_U, h->d_E,
                       h->d_P, h->d_Q, busx ? h->d_x : h->d_f, tree_bst(h), h->d_respart, h->errpart_stride, ctx.s0, ctx.S,
                       div_magic(h->Hn), lds > 0 ? 1 : 0, h->src_set ? h->d_src : (const cplx*)nullptr);
    hipLaunchKernelGGL(k_step_eta, dim3((unsigned)ctx.S), dim3(64), 0, ctx.stream, ctx.S, ctx.active, h->d_respart, h->errpart_stride,
                       err_parts<false>(h), h->resid_limit, h->d_eta, h->S_alloc, h->d_pivflag, ctx.s0);
    return launch_status(h);
}

// One Newton step: Jacobian at the current state, step = J^{-1} f into d_f.
template <bool FUND>
int newton_step(hpf_handle* h, const LaunchCtx& ctx) {
    int r;
    if (h->solver == HPF_SOLVER_BLOCK_TREE && h->n_ties == 0)
        return FUND ? tree_fund_step(h, ctx) : tree_newton_step(h, ctx, FACTOR_AND_BACK);
    if (h->solver == HPF_SOLVER_BLOCK_TREE && !FUND) return tree_newton_step_bordered(h, ctx);
    // (a meshed network on the block-tree path takes its fundamental power flow through the dense LU: Nf = 2n - 1 - c is small)
    const int Nsys = FUND ? h->Nf : h->N;
    if ((r = ensure_dense(h, Nsys))) return r;
    if ((r = launch_jacobian_dense<FUND>(h, ctx))) return r;
    return dense_solve(h, Nsys);
}

// what one Newton iteration of a launch context launches besides step, update and mismatch; the defaults: nothing (hpf_iterate)
struct IterSpec {
    bool keep_prev = false;        // k_keep_prev before the step (hpf_solve with keep_previous_state)
    bool finalize = false;         // k_finalize behind the mismatch (the device's stop rule; it owns d_active and d_nactive) ...
    double thresh = 0.0;           // ... and its arguments
    int max_iter = 0, hist_cap = 1, hist_off = 0;
    double* hist = nullptr;        // nullptr, with hist_cap 1: no error history (the queue)
};

template <bool FUND>
int launch_iteration(hpf_handle* h, const LaunchCtx& ctx, const IterSpec& it) {
    int r;
    if (it.keep_prev)
        hipLaunchKernelGGL(k_keep_prev, grid2(h->n * h->Hn, ctx.S), dim3(TPB), 0, ctx.stream, h->n * h->Hn, ctx.active, h->d_Vm, h->d_Va,
                           h->d_Vmp, h->d_Vap, ctx.s0);
    if ((r = newton_step<FUND>(h, ctx))) return r;
    if (!FUND && h->resid_check && (r = launch_step_residual(h, ctx))) return r;
    if ((r = launch_update<FUND>(h, ctx))) return r;
    if ((r = launch_mismatch<FUND>(h, ctx, false))) return r;
    if (it.finalize)
        hipLaunchKernelGGL(k_finalize, dim3((unsigned)ctx.S), dim3(64), 0, ctx.stream, ctx.S, 0, it.thresh, it.max_iter, it.hist_cap,
                           it.hist_off, h->d_errpart, h->errpart_stride, err_parts<FUND>(h), h->d_err, h->d_niter, h->d_active, h->d_nactive,
                           it.hist, ctx.s0, (const int*)nullptr);
    return HPF_OK;
}

enum GroupOrder {
    GROUP_MAJOR,           // every iteration of a group before the next group's first (the chunks of hpf_solve and of the queue)
    ITERATION_MAJOR        // all groups' step i before any group's step i + 1: keeps the group pipelines in phase (hpf_iterate)
};

// `iters` iterations of slots [0, slots) of the slot list `active` (nullptr: of the batch), split over the scenario groups (hpf_groups.hpp), each group on its
// own stream between a fork and a join with the handle's stream.  One group, as the fundamental pass always is, runs on the handle's stream
// without any event call.  An error ends the launches but not the joins: what was forked is joined, then the first error comes back.
template <bool FUND>
int enqueue_iterations(hpf_handle* h, int slots, const int* active, int iters, const IterSpec& it, GroupOrder order) {
    const int G = FUND ? 1 : group_count(h->solver == HPF_SOLVER_BLOCK_TREE && h->n_ties == 0, h->n_groups, slots);
    if (G > 1) HIPCHK(hipEventRecord(h->fork_ev, h->stream));
    int rc = HPF_OK;
    auto ev = [&](hipError_t e) {
        if (e != hipSuccess && rc == HPF_OK) {
            h->last_detail = (int)e;
            rc = HPF_E_HIP;
        }
    };
    auto fork = [&](int g) { if (G > 1) ev(hipStreamWaitEvent(group_stream(h, g), h->fork_ev, 0)); };
    auto join = [&](int g) { if (G > 1) ev(hipEventRecord(h->join_ev[g], group_stream(h, g))); };
    auto iteration = [&](int g) {
        if (rc != HPF_OK) return;
        const int s0 = group_bound(slots, G, g);
        rc = launch_iteration<FUND>(h, LaunchCtx{group_stream(h, g), s0, group_bound(slots, G, g + 1) - s0, active}, it);
    };
    if (order == GROUP_MAJOR) {
        for (int g = 0; g < G; ++g) {
            fork(g);
            for (int i = 0; i < iters; ++i) iteration(g);
            join(g);
        }
    } else {
        for (int g = 0; g < G; ++g) fork(g);
        for (int i = 0; i < iters; ++i)
            for (int g = 0; g < G; ++g) iteration(g);
        for (int g = 0; g < G; ++g) join(g);
    }
    for (int g = 0; G > 1 && g < G; ++g) ev(hipStreamWaitEvent(h->stream, h->join_ev[g], 0));
    return rc;
}

int check_info(hpf_handle* h, const std::vector<int>& was_active) {
    if (!h->d_info) return HPF_OK;
    std::vector<int> info(2 * (size_t)h->S);
    HIPCHK(hipMemcpyAsync(info.data(), h->d_info, sizeof(int) * 2 * h->S, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int s = 0; s < h->S; ++s) {
        const long long v = h->info64 ? reinterpret_cast<const int64_t*>(info.data())[s] : (long long)info[s];
        if (was_active[s] >= 0 && v != 0) {
            h->last_detail = (int)v;
            return HPF_E_SINGULAR;
        }
    }
    return HPF_OK;
}

// state of every scenario after iteration `it` -> the caller's trace arrays (hpf_set_trace), ABI order q*n + i.  A first pass that may be
// repeated records into the staging copy instead (trace_staged; trace_finish sorts the rows out), the repeat pass only the scenarios it runs
// (trace_only): a scenario's rows never hold states of a pass its result does not come from.
int trace_record(hpf_handle* h, int it) {
    if (!h->trace_Vm || it >= h->trace_cap) return HPF_OK;
    const size_t count = (size_t)h->n * h->Hn, cnt = (size_t)h->S * count, all = (size_t)h->S * h->trace_cap * count;
    std::vector<double> tm(cnt), ta(cnt);
    HIPCHK(hipMemcpyAsync(tm.data(), h->d_Vm, sizeof(double) * cnt, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(ta.data(), h->d_Va, sizeof(double) * cnt, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    double* const bm = h->trace_staged ? h->trace_stage.data() : h->trace_Vm;
    double* const ba = h->trace_staged ? h->trace_stage.data() + all : h->trace_Va;
    for (int sc = 0; sc < h->S; ++sc) {
        if (!h->trace_only.empty() && !h->trace_only[sc]) continue;
        double* om = bm + ((size_t)sc * h->trace_cap + it) * count;
        double* oa = ba + ((size_t)sc * h->trace_cap + it) * count;
        for (int i = 0; i < h->n; ++i)
            for (int q = 0; q < h->Hn; ++q) {
                om[(size_t)q * h->n + i] = tm[(size_t)sc * count + (size_t)i * h->Hn + q];
                oa[(size_t)q * h->n + i] = ta[(size_t)sc * count + (size_t)i * h->Hn + q];
            }
    }
    h->trace_last = it;
    return HPF_OK;
}

// The trace of a solve whose first pass was staged, after its last pass.  mask[s] != 0: scenario s was repeated (its rows 1 .. it_rep are the
// repeat's, already in the caller's arrays); niter1: the iteration counts the first pass left.  Rows 0 .. L are written, L = the largest
// iteration count among the results the call returns: a scenario that was not repeated gets its first-pass rows, a repeated one row 0 (the
// entering state) from the stage; behind its own pass every scenario repeats its last state up to L.  Rows beyond L stay the caller's.
void trace_finish(hpf_handle* h, const std::vector<int>& mask, const std::vector<int>& niter1, int it_rep) {
    const size_t count = (size_t)h->n * h->Hn, all = (size_t)h->S * h->trace_cap * count;
    const int top = h->trace_cap - 1;
    int Lu = 0;
    for (int s = 0; s < h->S; ++s)
        if (!mask[s] && niter1[s] > Lu) Lu = niter1[s];
    Lu = Lu < top ? Lu : top;
    it_rep = it_rep < top ? it_rep : top;
    const int L = Lu > it_rep ? Lu : it_rep;
    for (int v = 0; v < 2; ++v) {
        double* out = v ? h->trace_Va : h->trace_Vm;
        const double* stage = h->trace_stage.data() + (v ? all : 0);
        for (int s = 0; s < h->S; ++s) {
            double* rows = out + (size_t)s * h->trace_cap * count;
            const int own = mask[s] ? it_rep : Lu;                 // the last row the scenario's own pass recorded
            memcpy(rows, stage + (size_t)s * h->trace_cap * count, sizeof(double) * count * (mask[s] ? 1 : (size_t)Lu + 1));
            for (int k = own + 1; k <= L; ++k) memcpy(rows + (size_t)k * count, rows + (size_t)own * count, sizeof(double) * count);
        }
    }
}

// pinned double buffer + events through which the host reads the slot counters one chunk late (every object under its own check: a failed
// creation is retried by the next call instead of leaving a null event behind)
int ensure_poll_buffers(hpf_handle* h) {
    for (int i = 0; i < 2; ++i) {
        if (!h->h_act[i]) HIPCHK(hipHostMalloc((void**)&h->h_act[i], sizeof(int) * 4, hipHostMallocDefault));
        if (!h->poll_ev[i]) HIPCHK(hipEventCreateWithFlags(&h->poll_ev[i], hipEventDisableTiming));
    }
    return HPF_OK;
}

// device counters `src` -> words 0, 1, .. of the pinned buffer `buf`, behind everything the handle's stream holds so far
int poll_post(hpf_handle* h, int buf, std::initializer_list<const int*> src) {
    int* dst = h->h_act[buf];
    for (const int* d : src) HIPCHK(hipMemcpyAsync(dst++, d, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipEventRecord(h->poll_ev[buf], h->stream));
    return HPF_OK;
}

// the words of poll_post(buf), once they have arrived; nullptr: the wait failed (last_detail)
const int* poll_wait(hpf_handle* h, int buf) {
    const hipError_t e = hipEventSynchronize(h->poll_ev[buf]);
    if (e == hipSuccess) return h->h_act[buf];
    h->last_detail = (int)e;
    return nullptr;
}

// One pass of the NR loop (HG:530-542 / HG:257-265) from the current state over the scenarios selected by `mask` (nullptr: all).
template <bool FUND>
int nr_pass(hpf_handle* h, double thresh, int max_iter, const int* mask) {
    int r;
    const int S = h->S;
    const int hist_off = FUND ? 1 : 0;                // pf records only post-update errors (HG:264)
    if ((r = launch_polar<FUND>(h))) return r;
    if (mask) hipLaunchKernelGGL(k_mask_to_list, dim3((S + 63) / 64), dim3(64), 0, h->stream, S, mask, h->d_active);
    if ((r = launch_mismatch<FUND>(h, batch_ctx(h, mask ? h->d_active : nullptr), false))) return r;
    HIPCHK(hipMemsetAsync(h->d_nactive, 0, sizeof(int), h->stream));
    hipLaunchKernelGGL(k_finalize, dim3((unsigned)S), dim3(64), 0, h->stream, S, 1, thresh, max_iter, h->hist_cap,
                       hist_off, h->d_errpart, h->errpart_stride, err_parts<FUND>(h), h->d_err, h->d_niter, h->d_active, h->d_nactive, h->d_hist, 0, mask);
    const bool trace = !FUND && h->trace_Vm != nullptr;
    h->trace_last = 0;
    if (trace && !mask && (r = trace_record(h, 0))) return r;
    // The per-scenario stop rule lives on the device (k_finalize after every iteration, in the scenario group's own pipeline):
    // frozen scenarios are skipped by every kernel, so the host only has to notice when NO scenario is active any more, and
    // noticing late changes nothing in the results.  BLOCK_TREE: the host looks every `chunk` iterations, and it looks at chunk
    // c - 1 while chunk c is already queued (pinned double buffer + events), so the device never drains between chunks.
    const bool pipelined = !FUND && h->solver == HPF_SOLVER_BLOCK_TREE && !trace && h->n_ties == 0;
    const int chunk = pipelined ? (S >= 8 ? 4 : 2) : 1;
    const IterSpec spec = {!FUND && h->keep_prev && h->d_Vmp, true, thresh, max_iter, h->hist_cap, hist_off, h->d_hist};
    if (pipelined) {
        if ((r = ensure_poll_buffers(h))) return r;
        // Between two chunks the slot list is compacted on the device (running scenarios first) and their count goes to the
        // host; the count the host knows is one chunk old, i.e. an upper bound (the count only falls): it sizes the grids and
        // the scenario groups of the next chunk.  Slots behind the true count hold -1 and their workgroups exit at once.
        auto compact_and_post = [&](int buf) -> int {
            hipLaunchKernelGGL(k_compact, dim3(1), dim3(1024), 0, h->stream, S, h->d_active, h->d_nactive);
            return poll_post(h, buf, {h->d_nactive});
        };
        int it = 0, c = 0, n_ub = S;
        if ((r = compact_and_post(0))) return r;
        for (;;) {
            // With few scenarios left the device is not kept busy anyway: look at the count of the chunk just queued before queueing
            // the next one (no trailing chunk of empty launches).  Otherwise queue chunk c + 1 (iterations it .. it + todo) BEFORE
            // looking at the count chunk c left, so that the device never drains between chunks.
            const bool lagged = n_ub > 8 || S <= 8;      // (a handle of a few scenarios keeps the queue fed: its chunks are short anyway)
            const int ch = lagged ? chunk : 2;
            if (!lagged) {
                const int* left = poll_wait(h, c & 1);
                if (!left) return HPF_E_HIP;
                if (left[0] == 0 || it >= max_iter) break;
                n_ub = left[0];
            }
            const int todo = (max_iter - it) < ch ? (max_iter - it) : ch;
            if (todo > 0) {
                if ((r = enqueue_iterations<FUND>(h, n_ub, h->d_active, todo, spec, GROUP_MAJOR))) return r;
                if ((r = compact_and_post((c + 1) & 1))) return r;
                it += todo;
            }
            if (!lagged) {
                ++c;
                continue;
            }
            const int* left = poll_wait(h, c & 1);
            if (!left) return HPF_E_HIP;
            if (left[0] == 0 || todo == 0) break;
            n_ub = left[0];
            ++c;
        }
        HIPCHK(hipStreamSynchronize(h->stream));
        return HPF_OK;
    }
    auto count_active = [&](const int* a) {
        int c = 0;
        for (int s = 0; s < S; ++s) c += a[s] >= 0;
        return c;
    };
    std::vector<int> act(S), was(S);
    HIPCHK(hipMemcpyAsync(act.data(), h->d_active, sizeof(int) * S, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    int nactive = count_active(act.data());
    int it = 0;
    while (nactive > 0 && it < max_iter) {
        was = act;                        // (no compaction on this path: slot i runs scenario i)
        h->host_act = act;                // (the bordered step of a meshed network walks the running scenarios on the host)
        if ((r = enqueue_iterations<FUND>(h, S, h->d_active, 1, spec, GROUP_MAJOR))) return r;
        HIPCHK(hipMemcpyAsync(act.data(), h->d_active, sizeof(int) * S, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        nactive = count_active(act.data());
        if (h->solver == HPF_SOLVER_DENSE)
            if ((r = check_info(h, was))) return r;
        ++it;
        if (trace && (r = trace_record(h, it))) return r;
    }
    return HPF_OK;
}

// ---- sweep accumulators: the host lifecycle of an Accum, written once (hpf_accum.hpp) ----------------------------------------
// the limit vector: the caller's `count` values, or +inf each (nothing is ever over); false: a NaN among them
bool accum_limits(const double* src, size_t count, std::vector<double>& lim) {
    lim.assign(count, (double)INFINITY);
    for (size_t k = 0; src && k < count; ++k) {
        if (src[k] != src[k]) return false;
        lim[k] = src[k];
    }
    return true;
}

void accum_close(Accum& a) {
    a.mem.clear();
    a.open = false;
}

// a (an open one is reset) <- nf statistics, narg ids, nover counters, all "nothing added yet", and the limits; whatever else the feature keeps
// in a.mem is allocated by the caller afterwards (accum_close on failure)
int accum_open(hpf_handle* h, Accum& a, size_t nf, size_t narg, size_t nover, const std::vector<double>& lim) {
    HIPCHK(hipStreamSynchronize(h->stream));
    accum_close(a);
    int r;
    if ((r = a.mem.alloc(&a.f, nf)) || (r = a.mem.alloc(&a.arg, narg)) || (r = a.mem.alloc(&a.over, nover)) || (r = a.mem.alloc(&a.cnt, (size_t)3)) ||
        (r = a.mem.upload(&a.limit, lim))) {
        accum_close(a);
        return r;
    }
    HIPCHK(hipMemsetAsync(a.f, 0, sizeof(double) * (nf ? nf : 1), h->stream));           // (a feeder without branches: blocks of one element)
    HIPCHK(hipMemsetAsync(a.arg, 0xff, sizeof(int) * (narg ? narg : 1), h->stream));
    HIPCHK(hipMemsetAsync(a.over, 0, sizeof(uint32_t) * (nover ? nover : 1), h->stream));
    HIPCHK(hipMemsetAsync(a.cnt, 0, sizeof(long long) * 3, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    a.nf = nf;
    a.narg = narg;
    a.nover = nover;
    a.open = true;
    return HPF_OK;
}

// hpf_*_end
int accum_end(hpf_handle* h, Accum hpf_handle::*which) {
    if (!h) return HPF_E_ARG;
    if (!(h->*which).open) return HPF_OK;
    HIPCHK(hipStreamSynchronize(h->stream));
    accum_close(h->*which);
    return HPF_OK;
}

// hpf_*_add: the finished hpf_solve of the current batch, scenario s under id first_id + s, through the feature's launch
int accum_add(hpf_handle* h, Accum hpf_handle::*which, int (*launch)(hpf_handle*, const AccumList&), int first_id) {
    if (!h || first_id < 0) return HPF_E_ARG;
    if (!(h->*which).open || !h->loads_set || !h->state_set || h->S < 1 || !h->solve_done) return HPF_E_STATE;
    int r;
    if ((r = launch(h, AccumList{h->S, nullptr, nullptr, first_id, 0, h->d_stats}))) return r;
    HIPCHK(hipStreamSynchronize(h->stream));
    return HPF_OK;
}

// hpf_*_get: the three scenario counters, after everything queued on the handle's stream ...
int accum_counts(hpf_handle* h, const Accum& a, int64_t* counts) {
    long long cnt[3];
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(cnt, a.cnt, sizeof(cnt), hipMemcpyDeviceToHost));
    for (int k = 0; counts && k < 3; ++k) counts[k] = cnt[k];
    return HPF_OK;
}

// ... and row k of `count` elements of one of its arrays (dst NULL: not wanted)
template <class T>
int accum_row(hpf_handle* h, const T* src, size_t k, size_t count, T* dst) {
    if (dst && count) HIPCHK(hipMemcpy(dst, src + k * count, sizeof(T) * count, hipMemcpyDeviceToHost));
    return HPF_OK;
}

// hpf_*_get of an accumulator whose arrays leave as they lie: the counters and the rows of f (three per quantity), arg and over in layout order
int accum_get(hpf_handle* h, Accum hpf_handle::*which, size_t count, int64_t* counts, std::initializer_list<double*> f,
              std::initializer_list<int32_t*> arg, std::initializer_list<uint32_t*> over) {
    if (!h) return HPF_E_ARG;
    const Accum& a = h->*which;
    if (!a.open) return HPF_E_STATE;
    int r = accum_counts(h, a, counts);
    size_t k = 0;
    for (double* dst : f) r = r ? r : accum_row(h, a.f, k++, count, dst);
    k = 0;
    for (int32_t* dst : arg) r = r ? r : accum_row(h, a.arg, k++, count, dst);
    k = 0;
    for (uint32_t* dst : over) r = r ? r : accum_row(h, a.over, k++, count, dst);
    return r;
}

// one k_distortion_add launch on the handle's stream (the open accumulator of h)
int distortion_launch(hpf_handle* h, const AccumList& list) {
    const int T = h->n * h->Hn + h->n;
    hipLaunchKernelGGL(k_distortion_add, dim3((unsigned)((T + 1 + TPB - 1) / TPB)), dim3(TPB), 0, h->stream, h->n, h->Hn, list, h->d_Vm, h->dist.limit,
                       h->dist_thd_limit, h->dist_hist_max, h->dist_inv_w, h->dist_bins, h->dist.f, h->dist.arg, h->dist.over, h->dist.cnt);
    return launch_status(h);
}

void start_free(hpf_handle* h) {
    h->start_mem.clear();
    h->start_set = false;
}

// the four start arrays of a handle that has none yet
int start_alloc(hpf_handle* h) {
    if (h->d_sVm) return HPF_OK;
    const size_t count = (size_t)h->n * h->Hn;
    int r;
    DevMem& mem = h->start_mem;
    if ((r = mem.alloc(&h->d_sVm, count)) || (r = mem.alloc(&h->d_sVa, count)) || (r = mem.alloc(&h->d_sU, count)) || (r = mem.alloc(&h->d_sE, count))) {
        start_free(h);
        return r;
    }
    return HPF_OK;
}

// ---- per-scenario source currents (hpf_sources.hpp) ------------------------------------------------------------------------------------------
void queue_sources_drop(hpf_handle* h) {
    h->qsrc_mem.clear();
    h->qsrc_n = 0;
}

void sources_free(hpf_handle* h) {
    queue_sources_drop(h);
    h->src_mem.clear();
    h->src_set = false;
}

// doubles of the caller's array per scenario
inline size_t sources_row(const hpf_handle* h, int form) { return (size_t)(h->n - h->m) * (form == SRC_CURRENTS ? 2 * (size_t)h->Hn : 2); }

// the argument rules of hpf_set_sources / hpf_queue_sources, on the host, before any HIP call
int sources_check(const hpf_handle* h, int n_scen, int form, const double* data, const int32_t* orders) {
    if (!h || !data || n_scen < 1) return HPF_E_ARG;
    if (form != SRC_CURRENTS && form != SRC_SCALE_SHIFT) return HPF_E_ARG;
    if (form == SRC_SCALE_SHIFT && !orders) return HPF_E_ARG;
    const size_t cnt = (size_t)n_scen * sources_row(h, form);
    for (size_t k = 0; k < cnt; ++k)
        if (!isfinite(data[k])) return HPF_E_ARG;
    return HPF_OK;
}

// the caller's array (and the orders of form 1) -> fresh device buffers of `mem` (empty; cleared on failure), on the handle's stream
int sources_upload(hpf_handle* h, DevMem& mem, int n_scen, int form, const double* data, const int32_t* orders, void** d_data, int** d_orders) {
    int r;
    const size_t cnt = (size_t)n_scen * sources_row(h, form);
    if ((r = mem.alloc((double**)d_data, cnt)) || (form == SRC_SCALE_SHIFT && (r = mem.alloc(d_orders, (size_t)h->Hn)))) {
        mem.clear();
        return r;
    }
    hipError_t e = hipMemcpyAsync(*d_data, data, sizeof(double) * cnt, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess && *d_orders) e = hipMemcpyAsync(*d_orders, orders, sizeof(int) * (size_t)h->Hn, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);            // (the caller's arrays may go away after the call)
    if (e != hipSuccess) {
        mem.clear();
        h->last_detail = (int)e;
        return HPF_E_HIP;
    }
    return HPF_OK;
}

// scenarios 0 .. S - 1 of the batch <- rows g0 .. g0 + S - 1 of a device array in input form `form`, device to device on the handle's stream
int sources_fill(hpf_handle* h, int S, int form, const void* d_data, const int* d_orders, int g0) {
    const int nnl = h->n - h->m;
    int r;
    if (!h->d_src && (r = h->src_mem.alloc(&h->d_src, (size_t)h->S_max * nnl * h->Hn))) return r;
    if (form == SRC_CURRENTS) {
        const size_t row = (size_t)nnl * h->Hn;
        HIPCHK(hipMemcpyAsync(h->d_src, (const cplx*)d_data + (size_t)g0 * row, sizeof(cplx) * row * (size_t)S, hipMemcpyDeviceToDevice, h->stream));
        return HPF_OK;
    }
    hipLaunchKernelGGL(k_source_expand, grid2(nnl * h->Hn, S), dim3(TPB), 0, h->stream, nnl, h->Hn, h->m, (const int*)nullptr, (const int*)nullptr,
                       g0, (const double*)d_data, d_orders, h->d_dev, h->d_IN, h->d_src);
    return launch_status(h);
}

void branch_free(hpf_handle* h) {
    accum_close(h->bstat);                               // (the statistics are per branch of this table)
    h->br_mem.clear();
    h->br_built = false;
}

// ---- branch table, branch flows, branch statistics (hpf_branch.hpp) ----------------------------------------------------------------------
// the table of a handle, built once by the first call that needs it: from / to / position in col of every stored pair (i, j), i < j, in CSR order
// (row-major, columns ascending), and the branch-major copy of the series admittances y = -Y
int branch_build(hpf_handle* h) {
    if (h->br_built) return HPF_OK;
    const int n = h->n, Hn = h->Hn, nnz = h->nnz;
    std::vector<int> rowptr((size_t)n + 1), col((size_t)nnz);
    std::vector<cplx> Y((size_t)nnz * Hn);
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(rowptr.data(), h->d_rowptr, sizeof(int) * rowptr.size(), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(col.data(), h->d_col, sizeof(int) * col.size(), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(Y.data(), h->d_Y, sizeof(cplx) * Y.size(), hipMemcpyDeviceToHost));     // entry-major [nnz][Hn]
    branch_table(n, rowptr.data(), col.data(), h->br_from, h->br_to, h->br_ypos);
    const int nb = (int)h->br_from.size();
    if (nb != h->nb) return HPF_E_STATE;                 // (hpf_create counted the same pattern)
    std::vector<cplx> yb((size_t)nb * Hn);
    for (int e = 0; e < nb; ++e)
        for (int q = 0; q < Hn; ++q) yb[(size_t)e * Hn + q] = cneg(Y[(size_t)h->br_ypos[e] * Hn + q]);
    const int tiles = (nb + BRANCH_TILE - 1) / BRANCH_TILE;
    int r;
    DevMem& mem = h->br_mem;
    if ((r = mem.upload(&h->d_br_from, h->br_from)) || (r = mem.upload(&h->d_br_to, h->br_to)) || (r = mem.upload(&h->d_br_y, yb)) ||
        (r = mem.alloc(&h->d_br_part, (size_t)h->S_max * tiles * Hn))) {
        branch_free(h);
        return r;
    }
    h->br_built = true;
    return HPF_OK;
}

// one k_branch_add launch on the handle's stream (the open accumulator of h)
int branch_add_launch(hpf_handle* h, const AccumList& list) {
    hipLaunchKernelGGL(k_branch_add, dim3((unsigned)((h->nb + 1 + BR_TPB - 1) / BR_TPB)), dim3(BR_TPB), 0, h->stream, h->nb, h->Hn, h->n, list, h->d_U,
                       h->d_br_from, h->d_br_to, h->d_br_y, h->bstat.limit, h->bstat.f, h->bstat.arg, h->bstat.over, h->bstat.cnt);
    return launch_status(h);
}

// one k_wave_peaks launch on the handle's stream: T samples (a valid T), the list, nbus buses per entry
void wave_peaks_launch(hpf_handle* h, int T, const AccumList& list, int nbus, const int* buslist, const int* orders, const double* ct, const double* st,
                       double* v, double* peak, int* kpeak, double* crest, double* slack) {
    if (list.L < 1 || nbus < 1) return;
    const dim3 grid((unsigned)((nbus + WV_BUSES - 1) / WV_BUSES), (unsigned)list.L);
    const size_t lds = 2 * sizeof(double) * (size_t)T;               // (at most 64 KiB: no attribute needed)
#define HPF_WAVE_LAUNCH(C)                                                                                                                       \
    hipLaunchKernelGGL((k_wave_peaks<C>), grid, dim3(WV_TPB), lds, h->stream, h->n, h->Hn, T, nbus, buslist, list, (const cplx*)h->d_U, orders, ct, \
                       st, v, peak, kpeak, crest, slack)
    switch (T / 64) {
        case 1: HPF_WAVE_LAUNCH(1); break;
        case 2: HPF_WAVE_LAUNCH(2); break;
        case 4: HPF_WAVE_LAUNCH(4); break;
        case 8: HPF_WAVE_LAUNCH(8); break;
        default: HPF_WAVE_LAUNCH(16); break;
    }
#undef HPF_WAVE_LAUNCH
}

// the open waveform accumulator of h takes a list: k_wave_peaks into the scratch, then k_wave_add
int wave_add_launch(hpf_handle* h, const AccumList& list) {
    wave_peaks_launch(h, h->ws_T, list, h->n, nullptr, h->d_ws_orders, h->d_ws_ct, h->d_ws_st, nullptr, h->d_ws_peak, nullptr, h->d_ws_crest, nullptr);
    hipLaunchKernelGGL(k_wave_add, dim3((unsigned)((h->n + 1 + BR_TPB - 1) / BR_TPB)), dim3(BR_TPB), 0, h->stream, h->n, list, h->d_ws_peak, h->d_ws_crest,
                       h->wstat.limit, h->ws_crest_limit, h->wstat.f, h->wstat.arg, h->wstat.over, h->wstat.cnt);
    return launch_status(h);
}

// every open accumulator of h takes the list (hpf_solve_queue, after a harvest round or a wave)
int accum_add_open(hpf_handle* h, const AccumList& list) {
    int r;
    if (h->dist.open && (r = distortion_launch(h, list))) return r;
    if (h->bstat.open && (r = branch_add_launch(h, list))) return r;
    if (h->wstat.open && (r = wave_add_launch(h, list))) return r;
    return HPF_OK;
}

// mode bits of hpf_stat.flags (include/hpf.h): begun at the handle's start state, rectangular update, per-scenario sources
inline int stat_mode_flags(const hpf_handle* h, bool from_start) { return (from_start ? 256 : 0) | (h->rect_update ? 512 : 0) | (h->src_set ? 1024 : 0); }

template <bool FUND>
int nr_loop(hpf_handle* h, double thresh, int max_iter, int* n_iter, double* err, double* err_hist) {
    if (!h->loads_set || !h->state_set || h->S < 1) return HPF_E_STATE;
    if (max_iter < 0) return HPF_E_ARG;
    h->solve_done = false;
    int r;
    const int S = h->S;
    const int cap = max_iter + 1;
    if (h->hist_cap < cap) {
        h->hist_cap = 0;
        if ((r = h->mem.alloc(&h->d_hist, (size_t)cap * h->S_max))) return r;       // (releases the smaller one first)
        h->hist_cap = cap;
    }
    {
        const size_t cnt = (size_t)h->hist_cap * S;
        hipLaunchKernelGGL(k_fill, dim3((unsigned)((cnt + TPB - 1) / TPB)), dim3(TPB), 0, h->stream, h->d_hist, cnt,
                           (double)NAN);
    }
    // BLOCK_TREE inverts the bus blocks with a STATIC pivot order (4x4 blocks on the matrix cores).  Every pivot block is watched
    // (inv4_cofactor_lane): a scenario in which one amplifies by more than piv_limit, or whose mismatch becomes non-finite, is
    // repeated from the state this call was entered with, with partial pivoting over the whole block (pivoted wave Gauss-Jordan
    // on the uncontracted tree).  hpf_stat.flags bit 3 / bit 4 report it.
    const bool can_repeat = !FUND && h->solver == HPF_SOLVER_BLOCK_TREE && h->has_ctree && h->gj_mode == 1 && h->auto_repivot &&
                            h->n_ties == 0;      // (the bordered step of a meshed network runs in the bus-image layout of the static-pivot kernels only)
    const size_t count = (size_t)h->n * h->Hn;
    if (!FUND) HIPCHK(hipMemsetAsync(h->d_pivflag, 0, sizeof(int) * S, h->stream));
    if (!FUND && h->resid_check && (r = reset_step_eta(h))) return r;
    if (can_repeat) {
        if (!h->d_Vm0) {
            DevMem& mem = h->repeat_mem;
            if ((r = mem.alloc(&h->d_Vm0, (size_t)h->S_max * count)) || (r = mem.alloc(&h->d_Va0, (size_t)h->S_max * count)) ||
                (r = mem.alloc(&h->d_mask, (size_t)h->S_max))) {
                mem.clear();
                return r;
            }
        }
        HIPCHK(hipMemcpyAsync(h->d_Vm0, h->d_Vm, sizeof(double) * S * count, hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->d_Va0, h->d_Va, sizeof(double) * S * count, hipMemcpyDeviceToDevice, h->stream));
    }
    // (trace: the first pass of a handle that may repeat is staged -- which rows belong to the caller is known after k_mark_repeat)
    const bool stage = can_repeat && h->trace_Vm != nullptr;
    if (stage) h->trace_stage.assign(2 * (size_t)S * h->trace_cap * count, 0.0);
    h->trace_staged = stage;
    r = nr_pass<FUND>(h, thresh, max_iter, nullptr);
    h->trace_staged = false;
    if (r) return r;
    if (can_repeat) {
        int nrep = 0;
        HIPCHK(hipMemsetAsync(h->d_nactive, 0, sizeof(int), h->stream));
        hipLaunchKernelGGL(k_mark_repeat, dim3((S + 63) / 64), dim3(64), 0, h->stream, S, h->d_err, h->d_pivflag, h->d_mask,
                           h->d_nactive, h->resid_check ? h->d_eta : (double*)nullptr, h->S_alloc);
        HIPCHK(hipMemcpyAsync(&nrep, h->d_nactive, sizeof(int), hipMemcpyDeviceToHost, h->stream));
        std::vector<int> rep_mask, niter1;
        if (stage) {
            rep_mask.resize(S);
            niter1.resize(S);
            HIPCHK(hipMemcpyAsync(rep_mask.data(), h->d_mask, sizeof(int) * S, hipMemcpyDeviceToHost, h->stream));
            HIPCHK(hipMemcpyAsync(niter1.data(), h->d_niter, sizeof(int) * S, hipMemcpyDeviceToHost, h->stream));
        }
        HIPCHK(hipStreamSynchronize(h->stream));
        h->trace_last = 0;
        if (nrep > 0) {
            const unsigned gx = (unsigned)(((count > (size_t)h->hist_cap ? count : (size_t)h->hist_cap) + TPB - 1) / TPB);
            hipLaunchKernelGGL(k_restore_masked, dim3(gx, (unsigned)S), dim3(TPB), 0, h->stream, (int)count, h->d_mask, h->d_Vm0,
                               h->d_Va0, h->d_Vm, h->d_Va, h->d_hist, h->hist_cap);
            h->gj_mode = 0;
            h->trace_only = rep_mask;
            r = nr_pass<FUND>(h, thresh, max_iter, h->d_mask);
            h->trace_only.clear();
            h->gj_mode = 1;
            if (r) {
                h->trace_stage = std::vector<double>();
                return r;
            }
        }
        if (stage) {
            trace_finish(h, rep_mask, niter1, h->trace_last);
            h->trace_stage = std::vector<double>();
        }
    }
    h->mismatch_valid = false;   // frozen scenarios leave stale rows in d_f: hpf_mismatch before hpf_iterate
    if (!FUND) h->prev_valid = h->keep_prev && h->d_Vmp;
    if (n_iter) HIPCHK(hipMemcpy(n_iter, h->d_niter, sizeof(int) * S, hipMemcpyDeviceToHost));
    if (err) HIPCHK(hipMemcpy(err, h->d_err, sizeof(double) * S, hipMemcpyDeviceToHost));
    if (err_hist) {
        const int cols = FUND ? max_iter : max_iter + 1;
        HIPCHK(hipMemcpy2D(err_hist, sizeof(double) * cols, h->d_hist, sizeof(double) * h->hist_cap,
                           sizeof(double) * cols, S, hipMemcpyDeviceToHost));
    }
    if (!FUND) {
        hipLaunchKernelGGL(k_stats, dim3(S), dim3(TPB), 0, h->stream, h->n, h->Hn, thresh, max_iter, h->d_Vm, h->d_err,
                           h->d_niter, h->d_pivflag, stat_mode_flags(h, h->from_start), h->d_stats);
        h->stats_valid = true;             // (also where the call goes on to return HPF_E_SINGULAR: its outputs are written)
        std::vector<int> pf(S);
        HIPCHK(hipMemcpyAsync(pf.data(), h->d_pivflag, sizeof(int) * S, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        for (int s = 0; s < S; ++s)
            if (pf[s] & 4) {               // the pivoted Gauss-Jordan met an exactly zero pivot: singular Jacobian block
                h->last_detail = s;
                return HPF_E_SINGULAR;
            }
        h->solve_done = true;
    }
    return HPF_OK;
}

// hpf_solve_queue on the fast path (radial BLOCK_TREE, static-pivot kernels): all scenarios' loads and power-flow seeds resident in
// HBM, the harmonic NR runs in chunks of iterations over the slot list; between chunks finished scenarios are harvested and their
// storages refilled (k_queue_*).  The host looks at the counters one chunk late (pinned double buffer + events, as in nr_pass).
int solve_queue_fast(hpf_handle* h, int n_total, const double* P, const double* Q, double thresh_f, int max_iter_f, double thresh,
                     int max_iter, hpf_stat* stats, double* Vm, double* Va) {
    int r = HPF_OK;
    const int n = h->n, Hn = h->Hn, S_max = h->S_max;
    const size_t count = (size_t)n * Hn;
    const bool info = h->sw.queue_info;
    const auto t_0 = std::chrono::steady_clock::now();
    auto ms_since = [&](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count(); };
    double *qP = nullptr, *qQ = nullptr, *sVm = nullptr, *sVa = nullptr, *qVm = nullptr, *qVa = nullptr;
    hpf_stat* qst = nullptr;
    int* qi = nullptr;                                   // slot_scen [S_max] | hlist | hg | newlist | next, base
    DevMem tmp(&h->last_detail);                         // the whole sweep's arrays: gone on every return path ...
    auto cleanup = [&](int code) {
        hipStreamSynchronize(h->stream);                 // ... once the stream is done with them
        tmp.clear();
        return code;
    };
    const bool warm = h->start_set;                      // every scenario begins at the handle's start state: no pf, no seed arrays
    if ((r = tmp.alloc(&qP, (size_t)n_total * n)) || (r = tmp.alloc(&qQ, (size_t)n_total * n)) ||
        (!warm && ((r = tmp.alloc(&sVm, (size_t)n_total * n)) || (r = tmp.alloc(&sVa, (size_t)n_total * n)))) ||
        (r = tmp.alloc(&qst, (size_t)n_total)) || (r = tmp.alloc(&qi, (size_t)4 * S_max + 2)))
        return cleanup(r);
    if (Vm && ((r = tmp.alloc(&qVm, (size_t)n_total * count)) || (r = tmp.alloc(&qVa, (size_t)n_total * count)))) return cleanup(r);
    int *slot_scen = qi, *hlist = qi + S_max, *hg = qi + 2 * S_max, *newlist = qi + 3 * S_max, *next = qi + 4 * S_max, *base = next + 1;
    if (hipMemcpyAsync(qP, P, sizeof(double) * (size_t)n_total * n, hipMemcpyHostToDevice, h->stream) != hipSuccess ||
        hipMemcpyAsync(qQ, Q, sizeof(double) * (size_t)n_total * n, hipMemcpyHostToDevice, h->stream) != hipSuccess)
        return cleanup(HPF_E_HIP);
    // ---- fundamental power flow (HG:244-275) of every scenario from the reference's start, in waves of S_max; only the fundamental
    //      entries are kept (the harmonic rows of the seed are the constants of HG:181-183).  With a start state set there is no pf
    //      phase: no scenario goes through these waves
    const int n_pf = warm ? 0 : n_total;
    for (int g0 = 0; g0 < n_pf; g0 += S_max) {
        const int S = n_pf - g0 < S_max ? n_pf - g0 : S_max;
        h->S = S;
        hipMemcpyAsync(h->d_P, qP + (size_t)g0 * n, sizeof(double) * (size_t)S * n, hipMemcpyDeviceToDevice, h->stream);
        hipMemcpyAsync(h->d_Q, qQ + (size_t)g0 * n, sizeof(double) * (size_t)S * n, hipMemcpyDeviceToDevice, h->stream);
        hipLaunchKernelGGL(k_init_voltages, grid2((int)count, S), dim3(TPB), 0, h->stream, Hn, (int)count, h->d_Vm, h->d_Va);
        h->loads_set = h->state_set = true;
        if ((r = nr_loop<true>(h, thresh_f, max_iter_f, nullptr, nullptr, nullptr))) return cleanup(r);
        hipLaunchKernelGGL(k_queue_keep_seed, grid2(n, S), dim3(TPB), 0, h->stream, n, Hn, g0, h->d_Vm, h->d_Va, sVm, sVa);
    }
    if (info) {
        hipStreamSynchronize(h->stream);
        fprintf(stderr, "hpf queue: %d scenarios, %d slots: uploads + pf of all scenarios %.2f ms\n", n_total, S_max, ms_since(t_0));
    }
    const auto t_1 = std::chrono::steady_clock::now();
    // ---- harmonic NR with refill -------------------------------------------------------------------------------------------------
    const int S_used = n_total < S_max ? n_total : S_max;
    h->S = S_used;
    h->mismatch_valid = false;
    h->prev_valid = false;
    {
        std::vector<int> init((size_t)4 * S_max + 2, -1);
        init[(size_t)4 * S_max] = 0;                    // next
        init[(size_t)4 * S_max + 1] = 0;                // base
        if (hipMemcpyAsync(qi, init.data(), sizeof(int) * init.size(), hipMemcpyHostToDevice, h->stream) != hipSuccess) return cleanup(HPF_E_HIP);
        if (hipStreamSynchronize(h->stream) != hipSuccess) return cleanup(HPF_E_HIP);      // (init is a local)
    }
    if (hipMemsetAsync(h->d_nactive, 0, sizeof(int), h->stream) != hipSuccess) return cleanup(HPF_E_HIP);
    if (hipMemsetAsync(h->d_pivflag, 0, sizeof(int) * S_max, h->stream) != hipSuccess) return cleanup(HPF_E_HIP);
    hipLaunchKernelGGL(k_set_int, dim3((unsigned)((S_max + TPB - 1) / TPB)), dim3(TPB), 0, h->stream, h->d_active, S_max, -1);   // (empty slot list)
    if ((r = ensure_poll_buffers(h))) return cleanup(r);
    const size_t q_lds = sizeof(int) * 2 * (size_t)S_max;
    // one round between two chunks: compact -> harvest / refill -> initial mismatch of the new scenarios -> counters to the host
    auto round = [&](int buf) -> int {
        hipLaunchKernelGGL(k_compact, dim3(1), dim3(1024), 0, h->stream, S_max, h->d_active, h->d_nactive);
        hipLaunchKernelGGL(k_queue_refill, dim3(1), dim3(1024), q_lds, h->stream, S_max, n_total, h->d_active, h->d_nactive, slot_scen, next,
                           hlist, hg, newlist, base);
        hipLaunchKernelGGL(k_queue_harvest, dim3((unsigned)S_max), dim3(TPB), 0, h->stream, n, Hn, thresh, max_iter, hlist, hg, h->d_Vm,
                           h->d_Va, h->d_err, h->d_niter, h->d_pivflag, stat_mode_flags(h, warm), qst, qVm, qVa);
        if (accum_add_open(h, AccumList{S_max, hlist, hg, h->dist_id_base, 1, qst})) return HPF_E_HIP;   // (before the storages are refilled)
        if (warm)
            hipLaunchKernelGGL(k_queue_init_start, grid2((int)count, S_max), dim3(TPB), 0, h->stream, n, Hn, newlist, slot_scen, qP, qQ, h->d_sVm,
                               h->d_sVa, h->d_sU, h->d_sE, h->d_P, h->d_Q, h->d_Vm, h->d_Va, h->d_U, h->d_E, h->d_niter, h->d_pivflag);
        else
            hipLaunchKernelGGL(k_queue_init, grid2((int)count, S_max), dim3(TPB), 0, h->stream, n, Hn, newlist, slot_scen, qP, qQ, sVm, sVa,
                               h->d_P, h->d_Q, h->d_Vm, h->d_Va, h->d_U, h->d_E, h->d_niter, h->d_pivflag);
        if (h->src_set) {                                // (hpf_queue_sources: the new scenarios' sources move in with their loads)
            const int nnl = n - h->m;
            if (h->qsrc_form == SRC_CURRENTS)
                hipLaunchKernelGGL(k_source_gather, grid2(nnl * Hn, S_max), dim3(TPB), 0, h->stream, nnl * Hn, newlist, slot_scen,
                                   (const cplx*)h->d_qsrc, h->d_src);
            else
                hipLaunchKernelGGL(k_source_expand, grid2(nnl * Hn, S_max), dim3(TPB), 0, h->stream, nnl, Hn, h->m, newlist, slot_scen, 0,
                                   (const double*)h->d_qsrc, h->d_qorders, h->d_dev, h->d_IN, h->d_src);
        }
        if (int rr = launch_mismatch<false>(h, LaunchCtx{h->stream, 0, S_max, newlist}, false)) return rr;   // (every storage: the list names the new ones)
        hipLaunchKernelGGL(k_queue_first, dim3((unsigned)S_max), dim3(64), 0, h->stream, S_max, thresh, max_iter, newlist, base,
                           h->d_errpart, h->errpart_stride, err_parts<false>(h), h->d_err, h->d_active);
        if (launch_status(h)) return HPF_E_HIP;
        return poll_post(h, buf, {h->d_nactive, next});
    };
    const IterSpec spec = {false, true, thresh, max_iter};       // (no error history, no previous state: nothing could read either after a sweep)
    const int chunk = h->queue_chunk > 0 ? h->queue_chunk : 4;
    int c = 0, n_ub = S_used;
    if ((r = round(0))) return cleanup(r);
    const long long max_rounds = ((long long)(n_total + S_used - 1) / S_used + 2) * ((max_iter + chunk - 1) / chunk + 2) + 8;
    for (long long rd = 0; rd < max_rounds; ++rd) {
        // queue the next chunk BEFORE looking at what the previous round left (the device never drains between chunks)
        if (n_ub > 0 && (r = enqueue_iterations<false>(h, n_ub, h->d_active, chunk, spec, GROUP_MAJOR))) return cleanup(r);
        if ((r = round((c + 1) & 1))) return cleanup(r);
        const int* left = poll_wait(h, c & 1);
        if (!left) return cleanup(HPF_E_HIP);
        const int cnt = left[0], nxt = left[1];
        ++c;
        if (cnt == 0 && nxt >= n_total) break;           // nothing was running and nothing was pending: every scenario is harvested
        n_ub = nxt < n_total ? S_used : cnt;             // pending scenarios: every storage may be running after the next refill
    }
    if (hipStreamSynchronize(h->stream) != hipSuccess) return cleanup(HPF_E_HIP);
    if (info) fprintf(stderr, "hpf queue: harmonic NR with refill %.2f ms (%d rounds of %d iterations)\n", ms_since(t_1), c, chunk);
    if (h->h_act[c & 1][0] != 0 || h->h_act[c & 1][1] < n_total) return cleanup(HPF_E_STATE);     // (round cap hit: cannot happen)
    if (stats && hipMemcpy(stats, qst, sizeof(hpf_stat) * (size_t)n_total, hipMemcpyDeviceToHost) != hipSuccess) return cleanup(HPF_E_HIP);
    if (Vm && (hipMemcpy(Vm, qVm, sizeof(double) * (size_t)n_total * count, hipMemcpyDeviceToHost) != hipSuccess ||
               hipMemcpy(Va, qVa, sizeof(double) * (size_t)n_total * count, hipMemcpyDeviceToHost) != hipSuccess))
        return cleanup(HPF_E_HIP);
    // the handle is left without a defined batch: loads and state have to be set again before the per-batch entry points
    h->loads_set = h->state_set = h->solve_done = h->from_start = h->stats_valid = false;
    h->S = 0;
    return cleanup(HPF_OK);
}

// everything of the handle that is no device block (those go with their owners, hpf_internal.hpp, when the handle is deleted)
void free_all(hpf_handle* h) {
    for (auto& sp : h->spans) {
        hipEventDestroy(sp.e0);
        hipEventDestroy(sp.e1);
    }
    for (int g = 0; g < 8; ++g) {
        if (h->gstream[g]) hipStreamDestroy(h->gstream[g]);
        if (h->join_ev[g]) hipEventDestroy(h->join_ev[g]);
    }
    if (h->fork_ev) hipEventDestroy(h->fork_ev);
    for (int i = 0; i < 2; ++i) {
        if (h->h_act[i]) hipHostFree(h->h_act[i]);
        if (h->poll_ev[i]) hipEventDestroy(h->poll_ev[i]);
    }
    if (h->blas) rocblas_destroy_handle(h->blas);
    if (h->own_stream) hipStreamDestroy(h->own_stream);
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------------------
extern "C" {

int hpf_version(void) { return 101; }

const char* hpf_strerror(int code) {
    switch (code) {
        case HPF_OK: return "success";
        case HPF_E_ARG: return "invalid argument";
        case HPF_E_STATE: return "call order violated (loads/state/mismatch not set)";
        case HPF_E_TOPOLOGY: return "BLOCK_TREE solver: network not connected from bus 0, pattern not symmetric, or too many loop-closing lines (border > 16 384 unknowns)";
        case HPF_E_NOMEM: return "out of device memory";
        case HPF_E_HIP: return "HIP runtime error";
        case HPF_E_ROCSOLVER: return "rocBLAS/rocSOLVER error";
        case HPF_E_SINGULAR: return "singular Jacobian (zero pivot)";
        default: return "unknown error";
    }
}

int hpf_last_error_detail(const hpf_handle* h) { return h ? h->last_detail : 0; }

int hpf_create(hpf_handle** out, const hpf_desc* d) { return hpf_create_opts(out, d, nullptr); }

int hpf_create_opts(hpf_handle** out, const hpf_desc* d, const char* options) {
    if (!out || !d) return HPF_E_ARG;
    *out = nullptr;
    if (d->n < 1 || d->Hn < 1 || d->m < 1 || d->m > d->n || d->c < 1 || d->c > d->m || d->nnz < d->n ||
        d->max_scenarios < 1 || !d->rowptr || !d->col || !d->Yval || !d->dev_of_bus)
        return HPF_E_ARG;
    if (d->m < d->n && (d->n_dev < 1 || !d->Y_N || !d->I_N)) return HPF_E_ARG;
    if (d->solver != HPF_SOLVER_DENSE && d->solver != HPF_SOLVER_BLOCK_TREE) return HPF_E_ARG;
    // (the per-entry kernels split a thread id t <= n Hn + 255 into (bus, harmonic) through a 32-bit reciprocal of Hn: exact for t Hn < 2^32;
    //  and the stacked index n Hn itself has to fit an int with room for the 2 N + 1 sizes derived from it)
    if (((long long)d->n * d->Hn + 256) * d->Hn >= (1ll << 32) || (long long)d->n * d->Hn >= (1ll << 29)) return HPF_E_ARG;
    // host-side validation of the pattern: sorted columns, diagonal present, indices in range
    std::vector<int> diag(d->n, -1), erow(d->nnz);
    int n_upper = 0;                                     // stored pairs (i, j), i < j: the branches (hpf_num_branches)
    if (d->rowptr[0] != 0 || d->rowptr[d->n] != d->nnz) return HPF_E_ARG;
    for (int i = 0; i < d->n; ++i) {
        if (d->rowptr[i + 1] < d->rowptr[i]) return HPF_E_ARG;
        for (int e = d->rowptr[i]; e < d->rowptr[i + 1]; ++e) {
            const int j = d->col[e];
            if (j < 0 || j >= d->n) return HPF_E_ARG;
            if (e > d->rowptr[i] && d->col[e - 1] >= j) return HPF_E_ARG;
            if (j == i) diag[i] = e;
            if (j > i) ++n_upper;
            erow[e] = i;
        }
        if (diag[i] < 0) return HPF_E_ARG;
        const int dv = d->dev_of_bus[i];
        if (i >= d->m ? (dv < 0 || dv >= d->n_dev) : dv != -1) return HPF_E_ARG;
    }
    hpf_handle* h = new (std::nothrow) hpf_handle();
    if (!h) return HPF_E_NOMEM;
    const auto t_create = std::chrono::steady_clock::now();
    int r = HPF_OK;
    auto fail = [&](int code) {
        free_all(h);
        delete h;
        return code;
    };
    h->n = d->n; h->m = d->m; h->c = d->c; h->Hn = d->Hn; h->nnz = d->nnz; h->n_dev = d->n_dev;
    h->coupled = d->coupled ? 1 : 0; h->solver = d->solver; h->device = d->device; h->S_max = d->max_scenarios;
    h->nb = n_upper;
    h->Nc = d->n * d->Hn - 1;
    h->N = 2 * h->Nc - (d->c - 1);
    h->Nf = 2 * d->n - 1 - d->c;
    h->sw = parse_switches(options, env_switches_opted_in());
    h->gj_mode = h->sw.gj_mode;
    h->n_groups = h->sw.n_groups;
    // (dense systems beyond N * N = 2^31 -- 1 000 buses x 26 harmonics is already N = 51 998 -- go through rocSOLVER's 64-bit entry
    //  points, dense_solve; memory, 8 N^2 bytes per scenario, is what bounds them: HPF_E_NOMEM from the allocation)
    if (hipSetDevice(d->device) != hipSuccess) return fail(HPF_E_HIP);
    if (hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking) != hipSuccess) return fail(HPF_E_HIP);
    h->stream = h->own_stream;
    for (int g = 0; g < 8; ++g) {
        if (g > 0 && hipStreamCreateWithFlags(&h->gstream[g], hipStreamNonBlocking) != hipSuccess) return fail(HPF_E_HIP);   // (group 0: group_stream)
        if (hipEventCreateWithFlags(&h->join_ev[g], hipEventDisableTiming) != hipSuccess) return fail(HPF_E_HIP);
    }
    if (hipEventCreateWithFlags(&h->fork_ev, hipEventDisableTiming) != hipSuccess) return fail(HPF_E_HIP);
    // (the rocBLAS handle is created on first use, ensure_blas: the radial block-tree path never needs it and its creation costs
    //  more than the whole set-up of a 10 000-bus model)
    h->S_alloc = h->S_max;
    if (d->solver == HPF_SOLVER_BLOCK_TREE) {
        // loop-closing lines of a meshed network: the bordered Newton step needs 1 + m virtual scenario slots behind the real ones
        if ((r = tree_find_ties(h, d))) return fail(r);
        if (h->n_ties > 0) h->gj_mode = 1;           // (HPF_GJ_MODE=0 does not apply: the bordered step needs the static-pivot kernels' layout)
        if (h->n_ties > 0) h->S_alloc = h->S_max + border_slots(h);
    }
    const size_t HnN = (size_t)d->Hn * d->n, S = (size_t)h->S_alloc;
    const size_t ynsz = (size_t)d->n_dev * d->Hn * (d->coupled ? d->Hn : 1);
    DevMem& mem = h->mem;
    if ((r = mem.upload(&h->d_rowptr, d->rowptr, (size_t)d->n + 1))) return fail(r);
    if ((r = mem.upload(&h->d_col, d->col, (size_t)d->nnz))) return fail(r);
    if ((r = mem.upload(&h->d_diag, diag.data(), (size_t)d->n))) return fail(r);
    if ((r = mem.upload(&h->d_erow, erow.data(), (size_t)d->nnz))) return fail(r);
    if ((r = mem.upload(&h->d_dev, d->dev_of_bus, (size_t)d->n))) return fail(r);
    {   // row records of the mismatch kernel (Model::rowrec)
        std::vector<int> rec((size_t)d->n * 8, 0);
        for (int i = 0; i < d->n; ++i) {
            const int e0 = d->rowptr[i], e1 = d->rowptr[i + 1];
            rec[(size_t)i * 8] = e0;
            rec[(size_t)i * 8 + 1] = e1;
            for (int u = 0; u < 3; ++u) rec[(size_t)i * 8 + 2 + u] = d->col[e0 + u < e1 ? e0 + u : e1 - 1];
        }
        if ((r = mem.upload(&h->d_rowrec, rec.data(), rec.size()))) return fail(r);
    }
    {   // device copy of the admittances: entry-major [nnz][Hn] (Model::yi)
        std::vector<cplx> yt((size_t)d->Hn * d->nnz);
        const cplx* src = (const cplx*)d->Yval;
        for (int q = 0; q < d->Hn; ++q)
            for (int e = 0; e < d->nnz; ++e) yt[(size_t)e * d->Hn + q] = src[(size_t)q * d->nnz + e];
        if ((r = mem.upload(&h->d_Y, yt.data(), yt.size()))) return fail(r);
    }
    if ((r = mem.upload(&h->d_YN, (const cplx*)d->Y_N, ynsz))) return fail(r);
    if (h->coupled) {                                     // transposed copy for the mismatch kernel (Model::YNt)
        std::vector<cplx> yt(ynsz);
        const cplx* src = (const cplx*)d->Y_N;
        for (int dv = 0; dv < d->n_dev; ++dv)
            for (int q = 0; q < d->Hn; ++q)
                for (int p2 = 0; p2 < d->Hn; ++p2)
                    yt[((size_t)dv * d->Hn + p2) * d->Hn + q] = src[((size_t)dv * d->Hn + q) * d->Hn + p2];
        if ((r = mem.upload(&h->d_YNt, yt.data(), ynsz))) return fail(r);
    }
    if ((r = mem.upload(&h->d_IN, (const cplx*)d->I_N, (size_t)d->n_dev * d->Hn))) return fail(r);
    if ((r = mem.alloc(&h->d_P, S * d->n))) return fail(r);
    if ((r = mem.alloc(&h->d_Q, S * d->n))) return fail(r);
    if ((r = mem.alloc(&h->d_Vm, S * HnN))) return fail(r);
    if ((r = mem.alloc(&h->d_Va, S * HnN))) return fail(r);
    if ((r = mem.alloc(&h->d_U, S * HnN))) return fail(r);
    if ((r = mem.alloc(&h->d_E, S * HnN))) return fail(r);
    if ((r = mem.alloc(&h->d_I0, S * (size_t)h->n))) return fail(r);
    if ((r = mem.alloc(&h->d_f, S * (size_t)(h->N > h->Nf ? h->N : h->Nf)))) return fail(r);
    if ((r = mem.alloc(&h->d_errbits, S))) return fail(r);
    h->errpart_stride = err_parts<false>(h) > err_parts<true>(h) ? err_parts<false>(h) : err_parts<true>(h);
    if ((r = mem.alloc(&h->d_errpart, S * (size_t)h->errpart_stride))) return fail(r);
    if (hipMemset(h->d_errpart, 0, sizeof(unsigned long long) * S * (size_t)h->errpart_stride) != hipSuccess) return fail(HPF_E_HIP);
    if ((r = mem.alloc(&h->d_err, S))) return fail(r);
    if ((r = mem.alloc(&h->d_niter, S))) return fail(r);
    if ((r = mem.alloc(&h->d_active, S))) return fail(r);
    if ((r = mem.alloc(&h->d_nactive, (size_t)1))) return fail(r);
    if ((r = mem.alloc(&h->d_pivflag, S))) return fail(r);
    if (hipMemset(h->d_pivflag, 0, sizeof(int) * S) != hipSuccess) return fail(HPF_E_HIP);
    if ((r = mem.alloc(&h->d_stats, S))) return fail(r);
    Model& M = h->M;
    M.n = d->n; M.m = d->m; M.c = d->c; M.Hn = d->Hn; M.nnz = d->nnz; M.n_dev = d->n_dev; M.coupled = h->coupled; M.bus_major = 1;
    M.rowptr = h->d_rowptr; M.col = h->d_col; M.diag = h->d_diag; M.Y = h->d_Y; M.dev = h->d_dev;
    M.YN = h->d_YN; M.IN = h->d_IN; M.YNt = h->d_YNt; M.rowrec = h->d_rowrec;
    if (d->solver == HPF_SOLVER_BLOCK_TREE) {
        const auto t_tree = std::chrono::steady_clock::now();
        if ((r = tree_build(h, d))) return fail(r);
        if ((r = tree_sel_build(h, d))) return fail(r);
        h->setup_ms[1] = h->tree.plan_ms + h->ctree.plan_ms;
        h->setup_ms[2] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_tree).count() - h->setup_ms[1];
        const auto t_al = std::chrono::steady_clock::now();
        if ((r = tree_alloc_scenarios(h))) return fail(r);
        h->setup_ms[3] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_al).count();
    }
    h->setup_ms[0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_create).count();
    *out = h;
    return HPF_OK;
}

int hpf_destroy(hpf_handle* h) {
    if (!h) return HPF_E_ARG;
    hipSetDevice(h->device);
    hipStreamSynchronize(h->stream);
    free_all(h);
    delete h;
    return HPF_OK;
}

int hpf_num_unknowns(const hpf_handle* h) { return h ? h->N : HPF_E_ARG; }
int hpf_num_unknowns_fund(const hpf_handle* h) { return h ? h->Nf : HPF_E_ARG; }
int hpf_num_scenarios(const hpf_handle* h) { return h ? ((h->loads_set || h->state_set) ? h->S : 0) : HPF_E_ARG; }
int hpf_max_scenarios(const hpf_handle* h) { return h ? h->S_max : HPF_E_ARG; }
int hpf_tree_levels(const hpf_handle* h) { return h ? active_tree(const_cast<hpf_handle*>(h)).n_levels : HPF_E_ARG; }
int hpf_tree_depths(const hpf_handle* h) { return h ? active_tree(const_cast<hpf_handle*>(h)).n_depths : HPF_E_ARG; }

int hpf_set_loads(hpf_handle* h, int n_scen, const double* P, const double* Q) {
    if (!h || !P || !Q || n_scen < 1 || n_scen > h->S_max) return HPF_E_ARG;
    if (h->state_set && n_scen != h->S) h->state_set = false;
    h->S = n_scen;
    HIPCHK(hipMemcpyAsync(h->d_P, P, sizeof(double) * (size_t)n_scen * h->n, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_Q, Q, sizeof(double) * (size_t)n_scen * h->n, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->loads_set = true;
    h->src_set = false;                                  // (sources belong to a batch's loads: new loads, the model's I_N again)
    h->mismatch_valid = false;
    h->prev_valid = false;
    h->solve_done = false;
    h->stats_valid = false;
    return HPF_OK;
}

int hpf_set_sources(hpf_handle* h, int n_scen, int form, const double* data, const int32_t* orders) {
    int r;
    if ((r = sources_check(h, n_scen, form, data, orders))) return r;
    if (!h->loads_set || h->S < 1) return HPF_E_STATE;
    if (n_scen != h->S) return HPF_E_ARG;
    if (h->n == h->m) return HPF_OK;                     // no nonlinear bus: nothing to set
    void* dd = nullptr;
    int* od = nullptr;
    DevMem tmp(&h->last_detail);
    if ((r = sources_upload(h, tmp, n_scen, form, data, orders, &dd, &od))) return r;
    r = sources_fill(h, n_scen, form, dd, od, 0);
    if (r == HPF_OK && hipStreamSynchronize(h->stream) != hipSuccess) r = HPF_E_HIP;
    if (r) {
        h->src_set = false;
        return r;
    }
    h->src_set = true;
    h->mismatch_valid = false;
    h->solve_done = false;
    return HPF_OK;
}

int hpf_get_sources(hpf_handle* h, double* I_src) {
    if (!h || !I_src) return HPF_E_ARG;
    if (!h->src_set || h->S < 1) return HPF_E_STATE;
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(I_src, h->d_src, sizeof(cplx) * (size_t)h->S * (h->n - h->m) * h->Hn, hipMemcpyDeviceToHost));
    return HPF_OK;
}

int hpf_clear_sources(hpf_handle* h) {
    if (!h) return HPF_E_ARG;
    if (!h->d_src && !h->d_qsrc) {
        h->src_set = false;
        return HPF_OK;
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    const bool had = h->src_set;                         // (storage alone -- kept by hpf_set_loads, or a registration -- is no source of the batch)
    sources_free(h);
    if (had) {
        h->mismatch_valid = false;
        h->solve_done = false;
    }
    return HPF_OK;
}

int hpf_queue_sources(hpf_handle* h, int n_total, int form, const double* data, const int32_t* orders) {
    int r;
    if ((r = sources_check(h, n_total, form, data, orders))) return r;
    if (h->n == h->m) return HPF_OK;
    queue_sources_drop(h);                               // (a registration that was never consumed is replaced)
    if ((r = sources_upload(h, h->qsrc_mem, n_total, form, data, orders, &h->d_qsrc, &h->d_qorders))) return r;
    h->qsrc_n = n_total;
    h->qsrc_form = form;
    return HPF_OK;
}

int hpf_set_state(hpf_handle* h, int n_scen, const double* Vm, const double* Va) {
    if (!h || n_scen < 1 || n_scen > h->S_max || (Vm == nullptr) != (Va == nullptr)) return HPF_E_ARG;
    if (h->loads_set && n_scen != h->S) return HPF_E_ARG;
    h->S = n_scen;
    const int count = h->n * h->Hn;
    if (Vm) {
        // ABI: stacked order q*n + i per scenario (HG:174-184); device: bus-major i*Hn + q
        std::vector<double> tm((size_t)n_scen * count), ta((size_t)n_scen * count);
        for (int sc = 0; sc < n_scen; ++sc)
            for (int q = 0; q < h->Hn; ++q)
                for (int i = 0; i < h->n; ++i) {
                    tm[(size_t)sc * count + (size_t)i * h->Hn + q] = Vm[(size_t)sc * count + (size_t)q * h->n + i];
                    ta[(size_t)sc * count + (size_t)i * h->Hn + q] = Va[(size_t)sc * count + (size_t)q * h->n + i];
                }
        // on the handle's stream: ordered behind whatever hpf_iterate left in flight (the group streams join h->stream)
        HIPCHK(hipMemcpyAsync(h->d_Vm, tm.data(), sizeof(double) * tm.size(), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->d_Va, ta.data(), sizeof(double) * ta.size(), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    } else {
        hipLaunchKernelGGL(k_init_voltages, grid2(count, n_scen), dim3(TPB), 0, h->stream, h->Hn, count, h->d_Vm, h->d_Va);
        if (launch_status(h)) return HPF_E_HIP;
    }
    if (h->resid_check && reset_step_eta(h)) return HPF_E_HIP;       // (a new state: no step taken yet)
    HIPCHK(hipStreamSynchronize(h->stream));
    h->from_start = false;
    h->state_set = true;
    h->mismatch_valid = false;
    h->prev_valid = false;
    h->solve_done = false;
    h->stats_valid = false;
    return HPF_OK;
}

int hpf_get_state(hpf_handle* h, double* Vm, double* Va) {
    if (!h || !Vm || !Va) return HPF_E_ARG;
    if (!h->state_set || h->S < 1) return HPF_E_STATE;
    const size_t count = (size_t)h->n * h->Hn, cnt = (size_t)h->S * count;
    std::vector<double> tm(cnt), ta(cnt);
    HIPCHK(hipMemcpyAsync(tm.data(), h->d_Vm, sizeof(double) * cnt, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(ta.data(), h->d_Va, sizeof(double) * cnt, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int sc = 0; sc < h->S; ++sc)                                   // device bus-major -> ABI stacked order
        for (int q = 0; q < h->Hn; ++q)
            for (int i = 0; i < h->n; ++i) {
                Vm[(size_t)sc * count + (size_t)q * h->n + i] = tm[(size_t)sc * count + (size_t)i * h->Hn + q];
                Va[(size_t)sc * count + (size_t)q * h->n + i] = ta[(size_t)sc * count + (size_t)i * h->Hn + q];
            }
    return HPF_OK;
}

int hpf_start_set(hpf_handle* h, const double* Vm0, const double* Va0) {
    if (!h || !Vm0 || !Va0) return HPF_E_ARG;
    const size_t count = (size_t)h->n * h->Hn;
    for (size_t k = 0; k < count; ++k)
        if (!isfinite(Vm0[k]) || !isfinite(Va0[k]) || Vm0[k] == 0.0) return HPF_E_ARG;      // (E = U / Vm)
    int r;
    double* tmp = nullptr;                               // the caller's arrays as they are (stacked); the kernel transposes
    DevMem tmp_mem(&h->last_detail);
    if ((r = start_alloc(h)) || (r = tmp_mem.alloc(&tmp, 2 * count))) return r;
    hipError_t e = hipMemcpyAsync(tmp, Vm0, sizeof(double) * count, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(tmp + count, Va0, sizeof(double) * count, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_start_set, dim3((unsigned)((count + TPB - 1) / TPB)), dim3(TPB), 0, h->stream, h->n, h->Hn, tmp, tmp + count, h->d_sVm,
                           h->d_sVa, h->d_sU, h->d_sE);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    tmp_mem.clear();
    if (e != hipSuccess) {
        h->last_detail = (int)e;
        start_free(h);
        return HPF_E_HIP;
    }
    h->start_set = true;
    return HPF_OK;
}

int hpf_start_capture(hpf_handle* h, int scen) {
    if (!h || scen < 0) return HPF_E_ARG;
    if (!h->state_set || h->S < 1) return HPF_E_STATE;
    if (scen >= h->S) return HPF_E_ARG;
    const int count = h->n * h->Hn;
    int r, bad = 0;
    if ((r = start_alloc(h))) return r;
    // (d_nactive: the solvers' counter word, free between two calls, takes the validity verdict)
    hipError_t e = hipMemsetAsync(h->d_nactive, 0, sizeof(int), h->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_start_capture, dim3((unsigned)((count + TPB - 1) / TPB)), dim3(TPB), 0, h->stream, count, scen, h->d_Vm, h->d_Va,
                           h->d_sVm, h->d_sVa, h->d_sU, h->d_sE, h->d_nactive);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&bad, h->d_nactive, sizeof(int), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess || bad) {                        // the buffers may be partly overwritten: no start state is left
        start_free(h);
        if (e == hipSuccess) return HPF_E_STATE;
        h->last_detail = (int)e;
        return HPF_E_HIP;
    }
    h->start_set = true;
    return HPF_OK;
}

int hpf_start_get(hpf_handle* h, double* Vm0, double* Va0) {
    if (!h || !Vm0 || !Va0) return HPF_E_ARG;
    if (!h->start_set) return HPF_E_STATE;
    const size_t count = (size_t)h->n * h->Hn;
    std::vector<double> tm(count), ta(count);
    HIPCHK(hipMemcpyAsync(tm.data(), h->d_sVm, sizeof(double) * count, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(ta.data(), h->d_sVa, sizeof(double) * count, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int q = 0; q < h->Hn; ++q)                                         // device bus-major -> ABI stacked order
        for (int i = 0; i < h->n; ++i) {
            Vm0[(size_t)q * h->n + i] = tm[(size_t)i * h->Hn + q];
            Va0[(size_t)q * h->n + i] = ta[(size_t)i * h->Hn + q];
        }
    return HPF_OK;
}

int hpf_start_clear(hpf_handle* h) {
    if (!h) return HPF_E_ARG;
    if (!h->d_sVm) return HPF_OK;
    HIPCHK(hipStreamSynchronize(h->stream));
    start_free(h);
    return HPF_OK;
}

int hpf_start_apply(hpf_handle* h, int n_scen) {
    if (!h || n_scen < 1 || n_scen > h->S_max) return HPF_E_ARG;
    if (!h->start_set) return HPF_E_STATE;
    if (h->loads_set && n_scen != h->S) return HPF_E_ARG;                   // (the rules of hpf_set_state)
    h->S = n_scen;
    const int count = h->n * h->Hn;
    hipLaunchKernelGGL(k_start_apply, grid2(count, n_scen), dim3(TPB), 0, h->stream, count, h->d_sVm, h->d_sVa, h->d_sU, h->d_sE, h->d_Vm, h->d_Va,
                       h->d_U, h->d_E);
    if (launch_status(h)) return HPF_E_HIP;
    if (h->resid_check && reset_step_eta(h)) return HPF_E_HIP;
    HIPCHK(hipStreamSynchronize(h->stream));
    h->from_start = true;
    h->state_set = true;
    h->mismatch_valid = false;
    h->prev_valid = false;
    h->solve_done = false;
    h->stats_valid = false;
    return HPF_OK;
}

static int mismatch_impl(hpf_handle* h, bool fund, double* f, double* err) {
    if (!h) return HPF_E_ARG;
    if (!h->loads_set || !h->state_set || h->S < 1) return HPF_E_STATE;
    int r;
    if ((r = fund ? launch_polar<true>(h) : launch_polar<false>(h))) return r;
    if ((r = fund ? launch_mismatch<true>(h, batch_ctx(h)) : launch_mismatch<false>(h, batch_ctx(h)))) return r;
    hipLaunchKernelGGL(k_err_reduce, dim3((unsigned)h->S), dim3(64), 0, h->stream, h->d_errpart, h->errpart_stride,
                       fund ? err_parts<true>(h) : err_parts<false>(h), h->d_errbits);
    HIPCHK(hipStreamSynchronize(h->stream));
    const int N = fund ? h->Nf : h->N;
    if (f) HIPCHK(hipMemcpy(f, h->d_f, sizeof(double) * (size_t)h->S * N, hipMemcpyDeviceToHost));
    if (err) HIPCHK(hipMemcpy(err, h->d_errbits, sizeof(double) * h->S, hipMemcpyDeviceToHost));
    h->mismatch_valid = !fund;
    return HPF_OK;
}

int hpf_mismatch(hpf_handle* h, double* f, double* err) { return mismatch_impl(h, false, f, err); }
int hpf_fund_mismatch(hpf_handle* h, double* f, double* err) { return mismatch_impl(h, true, f, err); }

static int jacobian_impl(hpf_handle* h, bool fund, int scen, double* J) {
    if (!h || !J || scen < 0) return HPF_E_ARG;
    if (!h->loads_set || !h->state_set || h->S < 1) return HPF_E_STATE;
    if (scen >= h->S) return HPF_E_ARG;
    int r;
    const int Nsys = fund ? h->Nf : h->N;
    if ((r = ensure_dense(h, Nsys))) return r;
    if ((r = fund ? launch_polar<true>(h) : launch_polar<false>(h))) return r;
    if ((r = fund ? launch_jacobian_dense<true>(h, batch_ctx(h)) : launch_jacobian_dense<false>(h, batch_ctx(h)))) return r;
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(J, h->d_J + (size_t)scen * h->J_elems_per_scen, sizeof(double) * (size_t)Nsys * Nsys,
                     hipMemcpyDeviceToHost));
    return HPF_OK;
}

int hpf_jacobian(hpf_handle* h, int scen, double* J) { return jacobian_impl(h, false, scen, J); }

// indptr of the CSR Jacobian (a property of the model): built on the device at the first request, kept for the handle's life
static int jcsr_pattern(hpf_handle* h) {
    if (h->d_jptr) return HPF_OK;
    int r;
    long long* tot = nullptr;
    DevMem tmp(&h->last_detail);
    auto fail = [&](int code) {          // (d_jptr stays null until the pattern stands: the next call builds it again)
        h->mem.release(&h->d_jptr);
        return code;
    };
    if ((r = h->mem.alloc(&h->d_jptr, (size_t)h->N + 1)) || (r = tmp.alloc(&tot, (size_t)1))) return fail(r);
    hipLaunchKernelGGL(k_jcsr_count, dim3((unsigned)((h->N + TPB - 1) / TPB)), dim3(TPB), 0, h->stream, h->M, h->N, h->Nc, h->d_jptr);
    hipLaunchKernelGGL(k_jcsr_scan, dim3(1), dim3(1024), 0, h->stream, h->N, h->d_jptr, tot);
    long long nnz = 0;
    hipError_t e = hipMemcpyAsync(&nnz, tot, sizeof(long long), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        h->last_detail = (int)e;
        return fail(HPF_E_HIP);
    }
    if (nnz >= 0x7fffffffll) return fail(HPF_E_ARG);     // 32-bit column indices / offsets, like scipy's default index type
    h->jnnz = nnz;
    return HPF_OK;
}

static int jacobian_csr_impl(hpf_handle* h, int scen, int32_t* indptr, int32_t* indices, double* data) {
    if (!h || !data || scen < 0) return HPF_E_ARG;
    if (!h->loads_set || !h->state_set || h->S < 1) return HPF_E_STATE;
    if (scen >= h->S) return HPF_E_ARG;
    int r;
    if ((r = jcsr_pattern(h))) return r;
    if (!h->d_jval && (r = h->mem.alloc(&h->d_jval, (size_t)h->jnnz))) return r;      // (each buffer under its own check: a failed second
    if (!h->d_jcol && (r = h->mem.alloc(&h->d_jcol, (size_t)h->jnnz))) return r;      //  allocation is retried by the next call)
    if ((r = launch_polar<false>(h))) return r;
    const size_t so = (size_t)scen * h->n * h->Hn;
    hipLaunchKernelGGL(k_jcsr_fill, dim3((unsigned)((h->N + TPB - 1) / TPB)), dim3(TPB), 0, h->stream, h->M, h->N, h->Nc, h->d_jptr,
                       h->d_U + so, h->d_E + so, indices ? h->d_jcol : (int*)nullptr, h->d_jval);
    if (launch_status(h)) return HPF_E_HIP;
    HIPCHK(hipStreamSynchronize(h->stream));
    if (indptr) HIPCHK(hipMemcpy(indptr, h->d_jptr, sizeof(int32_t) * ((size_t)h->N + 1), hipMemcpyDeviceToHost));
    if (indices) HIPCHK(hipMemcpy(indices, h->d_jcol, sizeof(int32_t) * (size_t)h->jnnz, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(data, h->d_jval, sizeof(double) * (size_t)h->jnnz, hipMemcpyDeviceToHost));
    return HPF_OK;
}

int hpf_jacobian_nnz(hpf_handle* h, int64_t* nnz) {
    if (!h || !nnz) return HPF_E_ARG;
    const int r = jcsr_pattern(h);
    if (r) return r;
    *nnz = (int64_t)h->jnnz;
    return HPF_OK;
}

int hpf_jacobian_csr(hpf_handle* h, int scen, int32_t* indptr, int32_t* indices, double* data) {
    return jacobian_csr_impl(h, scen, indptr, indices, data);
}

// run fn() with the voltages of option "keep_previous_state" in place of the current ones, then put the current state back
static int with_previous_state(hpf_handle* h, int scen, const std::function<int()>& fn) {
    if (!h || scen < 0) return HPF_E_ARG;
    if (!h->keep_prev || !h->d_Vmp || !h->loads_set || !h->state_set || h->S < 1 || !h->prev_valid) return HPF_E_STATE;     // (all on the host)
    if (scen >= h->S) return HPF_E_ARG;
    {   // the kept state exists for scenarios that took at least one Newton step in the last hpf_solve
        int ni = 0;
        HIPCHK(hipMemcpy(&ni, h->d_niter + scen, sizeof(int), hipMemcpyDeviceToHost));
        if (ni <= 0) return HPF_E_STATE;
    }
    const size_t cnt = (size_t)h->S * h->n * h->Hn;
    // (the swap buffers belong to the handle: no allocation / release per call -- a hipFree right after another handle returned tens of GB to
    //  the driver was seen to take 60 ms)
    int r;
    if (!h->d_swapVm && (r = h->mem.alloc(&h->d_swapVm, (size_t)h->S_alloc * h->n * h->Hn))) return r;
    if (!h->d_swapVa && (r = h->mem.alloc(&h->d_swapVa, (size_t)h->S_alloc * h->n * h->Hn))) return r;
    double *tm = h->d_swapVm, *ta = h->d_swapVa;
    hipMemcpyAsync(tm, h->d_Vm, sizeof(double) * cnt, hipMemcpyDeviceToDevice, h->stream);
    hipMemcpyAsync(ta, h->d_Va, sizeof(double) * cnt, hipMemcpyDeviceToDevice, h->stream);
    hipMemcpyAsync(h->d_Vm, h->d_Vmp, sizeof(double) * cnt, hipMemcpyDeviceToDevice, h->stream);
    hipMemcpyAsync(h->d_Va, h->d_Vap, sizeof(double) * cnt, hipMemcpyDeviceToDevice, h->stream);
    r = fn();
    hipMemcpyAsync(h->d_Vm, tm, sizeof(double) * cnt, hipMemcpyDeviceToDevice, h->stream);
    hipMemcpyAsync(h->d_Va, ta, sizeof(double) * cnt, hipMemcpyDeviceToDevice, h->stream);
    if (!r) r = launch_polar<false>(h);
    hipStreamSynchronize(h->stream);
    return r;
}

int hpf_jacobian_last(hpf_handle* h, int scen, double* J) {
    if (!J) return HPF_E_ARG;
    return with_previous_state(h, scen, [&]() { return jacobian_impl(h, false, scen, J); });
}

int hpf_jacobian_csr_last(hpf_handle* h, int scen, int32_t* indptr, int32_t* indices, double* data) {
    if (!data) return HPF_E_ARG;
    return with_previous_state(h, scen, [&]() { return jacobian_csr_impl(h, scen, indptr, indices, data); });
}
int hpf_fund_jacobian(hpf_handle* h, int scen, double* J) { return jacobian_impl(h, true, scen, J); }

int hpf_fund_pf(hpf_handle* h, double thresh, int max_iter, int* n_iter, double* err, double* err_hist) {
    if (!h) return HPF_E_ARG;
    return nr_loop<true>(h, thresh, max_iter, n_iter, err, err_hist);
}

int hpf_solve(hpf_handle* h, double thresh, int max_iter, int* n_iter, double* err, double* err_hist) {
    if (!h) return HPF_E_ARG;
    return nr_loop<false>(h, thresh, max_iter, n_iter, err, err_hist);
}

// hpf_solve_queue behind its argument checks.  With a registration of hpf_queue_sources every scenario is solved with its sources: the fast path
// moves them into a scenario's storage with its loads (k_source_gather / k_source_expand), the waves set them device to device after the loads
static int solve_queue_any(hpf_handle* h, int n_total, const double* P, const double* Q, double thresh_f, int max_iter_f, double thresh,
                           int max_iter, hpf_stat* stats, double* Vm, double* Va) {
    const bool with_src = h->qsrc_n > 0;
    h->src_set = false;
    if (with_src) {
        int r;
        if (!h->d_src && (r = h->src_mem.alloc(&h->d_src, (size_t)h->S_max * (h->n - h->m) * h->Hn))) return r;
    }
    const bool fast = h->solver == HPF_SOLVER_BLOCK_TREE && h->n_ties == 0 && h->has_ctree && h->gj_mode == 1 &&
                      bus_images(h) && h->S_max <= 4096 && !h->trace_Vm;      // (k_queue_refill keeps its storage table in LDS: 8 B per slot)
    if (fast) {
        h->src_set = with_src;
        return solve_queue_fast(h, n_total, P, Q, thresh_f, max_iter_f, thresh, max_iter, stats, Vm, Va);
    }
    // every other handle (dense solver, meshed network, pivoted mode): waves of up to S_max scenarios through the per-batch entry points
    const size_t cnt = (size_t)h->n * h->Hn;
    for (int g0 = 0; g0 < n_total; g0 += h->S_max) {
        const int S = n_total - g0 < h->S_max ? n_total - g0 : h->S_max;
        int r;
        if ((r = hpf_set_loads(h, S, P + (size_t)g0 * h->n, Q + (size_t)g0 * h->n))) return r;
        if (with_src) {
            if ((r = sources_fill(h, S, h->qsrc_form, h->d_qsrc, h->d_qorders, g0))) return r;
            h->src_set = true;
        }
        if (h->start_set) {                              // every scenario from the handle's start state, no pf
            if ((r = hpf_start_apply(h, S))) return r;
        } else {
            if ((r = hpf_set_state(h, S, nullptr, nullptr))) return r;
            if ((r = hpf_fund_pf(h, thresh_f, max_iter_f, nullptr, nullptr, nullptr))) return r;
        }
        if ((r = hpf_solve(h, thresh, max_iter, nullptr, nullptr, nullptr))) return r;
        if ((r = accum_add_open(h, AccumList{S, nullptr, nullptr, h->dist_id_base + g0, 1, h->d_stats}))) return r;
        if (stats && (r = hpf_get_stats(h, stats + g0))) return r;
        if (Vm && (r = hpf_get_state(h, Vm + (size_t)g0 * cnt, Va + (size_t)g0 * cnt))) return r;
    }
    h->loads_set = h->state_set = h->solve_done = h->from_start = h->stats_valid = false;   // (as on the queued path: the handle is left without a defined batch)
    h->S = 0;
    return HPF_OK;
}

int hpf_solve_queue(hpf_handle* h, int n_total, const double* P, const double* Q, double thresh_f, int max_iter_f, double thresh,
                    int max_iter, hpf_stat* stats, double* Vm, double* Va) {
    if (!h || !P || !Q || n_total < 1 || max_iter < 0 || max_iter_f < 0 || (Vm == nullptr) != (Va == nullptr)) return HPF_E_ARG;
    if (h->qsrc_n && h->qsrc_n != n_total) {             // sources registered for another sweep: refused, and the registration is gone
        queue_sources_drop(h);
        return HPF_E_ARG;
    }
    const int rq = solve_queue_any(h, n_total, P, Q, thresh_f, max_iter_f, thresh, max_iter, stats, Vm, Va);
    queue_sources_drop(h);                               // (consumed; the handle holds no batch, hence no sources either)
    h->src_set = false;
    return rq;
}

int hpf_iterate(hpf_handle* h, int iters) {
    if (!h || iters < 0) return HPF_E_ARG;
    if (!h->loads_set || !h->state_set || !h->mismatch_valid) return HPF_E_STATE;
    h->solve_done = false;
    // (replaying a captured hipGraph of several iterations was measured again in round 2, with 3 / 4 / 6 / 8 scenario groups at
    //  128 and 1 024 scenarios: 0..-6 % -- the step is not bound by the host's launch rate)
    return enqueue_iterations<false>(h, h->S, nullptr, iters, IterSpec{}, ITERATION_MAJOR);       // (every scenario, unconditionally: no stop rule)
}

int hpf_get_stats(hpf_handle* h, hpf_stat* stats) {
    if (!h || !stats) return HPF_E_ARG;
    if (!h->state_set || h->S < 1 || !h->stats_valid) return HPF_E_STATE;     // (no batch in the handle, e.g. after hpf_solve_queue, or no hpf_solve of it yet)
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(stats, h->d_stats, sizeof(hpf_stat) * h->S, hipMemcpyDeviceToHost));
    return HPF_OK;
}

int hpf_get_stats_dev(hpf_handle* h, void* stats_dev) {
    if (!h || !stats_dev) return HPF_E_ARG;
    if (!h->state_set || h->S < 1 || !h->stats_valid) return HPF_E_STATE;
    HIPCHK(hipMemcpyAsync(stats_dev, h->d_stats, sizeof(hpf_stat) * h->S, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return HPF_OK;
}

int hpf_get_step_residuals(hpf_handle* h, double* eta_last, double* eta_max) {
    if (!h) return HPF_E_ARG;
    if (!h->resid_check || !h->d_eta || !h->state_set || h->S < 1) return HPF_E_STATE;
    HIPCHK(hipStreamSynchronize(h->stream));
    if (eta_last) HIPCHK(hipMemcpy(eta_last, h->d_eta, sizeof(double) * h->S, hipMemcpyDeviceToHost));
    if (eta_max) {
        HIPCHK(hipMemcpy(eta_max, h->d_eta + h->S_alloc, sizeof(double) * h->S, hipMemcpyDeviceToHost));
        for (int s = 0; s < h->S; ++s)
            if (eta_max[s] == -1.0) eta_max[s] = NAN;        // no step yet
    }
    return HPF_OK;
}

int hpf_distortion_begin(hpf_handle* h, const double* limit, double thd_limit, double hist_max, int hist_bins) {
    if (!h || hist_bins < 1 || hist_bins > 256 || !(hist_max > 0.0) || isinf(hist_max) || thd_limit != thd_limit) return HPF_E_ARG;
    std::vector<double> lim;
    if (!accum_limits(limit, (size_t)h->Hn, lim)) return HPF_E_ARG;
    const size_t T = (size_t)h->n * h->Hn + h->n;
    int r;
    if ((r = accum_open(h, h->dist, 3 * T, T, T + (size_t)h->n * (hist_bins + 1), lim))) return r;   // (the histogram behind the over counters)
    h->dist_bins = hist_bins;
    h->dist_thd_limit = thd_limit;
    h->dist_hist_max = hist_max;
    h->dist_inv_w = (double)hist_bins / hist_max;
    return HPF_OK;
}

int hpf_distortion_add(hpf_handle* h, int first_id) { return accum_add(h, &hpf_handle::dist, distortion_launch, first_id); }

int hpf_distortion_get(hpf_handle* h, int64_t* counts, double* x_max, int32_t* x_arg, double* x_sum, double* x_sumsq, uint32_t* x_over,
                       double* thd_max, int32_t* thd_arg, double* thd_sum, double* thd_sumsq, uint32_t* thd_over, uint32_t* thd_hist) {
    if (!h) return HPF_E_ARG;
    const Accum& a = h->dist;
    if (!a.open) return HPF_E_STATE;
    const int n = h->n, Hn = h->Hn;
    const size_t E = (size_t)n * Hn, T = E + n;
    std::vector<double> f(a.nf);
    std::vector<int32_t> arg(a.narg);
    std::vector<uint32_t> u(a.nover);
    int r;
    if ((r = accum_counts(h, a, counts)) || (r = accum_row(h, a.f, 0, a.nf, f.data())) || (r = accum_row(h, a.arg, 0, a.narg, arg.data())) ||
        (r = accum_row(h, a.over, 0, a.nover, u.data())))
        return r;
    double* xf[3] = {x_max, x_sum, x_sumsq};
    double* tf[3] = {thd_max, thd_sum, thd_sumsq};
    for (int k = 0; k < 3; ++k) {
        if (tf[k]) memcpy(tf[k], f.data() + k * T + E, sizeof(double) * n);
        if (!xf[k]) continue;
        for (int q = 0; q < Hn; ++q)                         // device bus-major -> ABI stacked order
            for (int i = 0; i < n; ++i) xf[k][(size_t)q * n + i] = f[k * T + (size_t)i * Hn + q];
    }
    for (int q = 0; q < Hn; ++q)
        for (int i = 0; i < n; ++i) {
            if (x_arg) x_arg[(size_t)q * n + i] = arg[(size_t)i * Hn + q];
            if (x_over) x_over[(size_t)q * n + i] = u[(size_t)i * Hn + q];
        }
    if (thd_arg) memcpy(thd_arg, arg.data() + E, sizeof(int32_t) * n);
    if (thd_over) memcpy(thd_over, u.data() + E, sizeof(uint32_t) * n);
    if (thd_hist) memcpy(thd_hist, u.data() + T, sizeof(uint32_t) * (size_t)n * (h->dist_bins + 1));
    return HPF_OK;
}

int hpf_distortion_end(hpf_handle* h) { return accum_end(h, &hpf_handle::dist); }

int hpf_num_branches(const hpf_handle* h) { return h ? h->nb : HPF_E_ARG; }

int hpf_get_branches(hpf_handle* h, int32_t* from, int32_t* to, int32_t* ypos) {
    if (!h) return HPF_E_ARG;
    int r;
    if ((r = branch_build(h))) return r;
    if (from) memcpy(from, h->br_from.data(), sizeof(int32_t) * (size_t)h->nb);
    if (to) memcpy(to, h->br_to.data(), sizeof(int32_t) * (size_t)h->nb);
    if (ypos) memcpy(ypos, h->br_ypos.data(), sizeof(int32_t) * (size_t)h->nb);
    return HPF_OK;
}

int hpf_branch_flows(hpf_handle* h, double* I, double* irms, double* thd_i, double* loss, double* loss_harm, double* loss_h) {
    if (!h) return HPF_E_ARG;
    if (!h->state_set || h->S < 1) return HPF_E_STATE;
    const size_t lds = (size_t)BRANCH_TILE * h->Hn * (sizeof(cplx) + 2 * sizeof(double));
    if (lds > 160 * 1024) return HPF_E_ARG;              // (Hn > 160)
    int r;
    if ((r = branch_build(h))) return r;
    const int S = h->S, nb = h->nb, Hn = h->Hn, tiles = (nb + BRANCH_TILE - 1) / BRANCH_TILE;
    const size_t count = (size_t)h->n * Hn;
    cplx* dI = nullptr;
    double* dv[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};      // irms, thd_i, loss, loss_harm, loss_h
    double* host[5] = {irms, thd_i, loss, loss_harm, loss_h};
    DevMem tmp(&h->last_detail);
    auto cleanup = [&](int code) {
        hipStreamSynchronize(h->stream);
        tmp.clear();
        return code;
    };
    if (I && (r = tmp.alloc(&dI, (size_t)S * Hn * nb))) return cleanup(r);
    for (int k = 0; k < 5; ++k)
        if (host[k] && (r = tmp.alloc(&dv[k], (size_t)S * (k == 4 ? Hn : nb)))) return cleanup(r);
    hipLaunchKernelGGL(k_branch_refresh_u, grid2((int)count, S), dim3(TPB), 0, h->stream, (int)count, h->d_Vm, h->d_Va, h->d_U);
    if (nb > 0) {
        if (lds > 64 * 1024 &&
            hipFuncSetAttribute(reinterpret_cast<const void*>(&k_branch_flows), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
            return cleanup(HPF_E_HIP);
        hipLaunchKernelGGL(k_branch_flows, dim3((unsigned)tiles, (unsigned)S), dim3(TPB), lds, h->stream, nb, Hn, h->n, tiles, h->d_br_from,
                           h->d_br_to, h->d_br_y, h->d_U, dI, dv[0], dv[1], dv[2], dv[3], loss_h ? h->d_br_part : (double*)nullptr);
    }
    if (loss_h)
        hipLaunchKernelGGL(k_branch_loss_h, grid2(Hn, S), dim3(TPB), 0, h->stream, Hn, nb > 0 ? tiles : 0, h->d_br_part, dv[4]);
    if (launch_status(h)) return cleanup(HPF_E_HIP);
    if (hipStreamSynchronize(h->stream) != hipSuccess) return cleanup(HPF_E_HIP);
    if (I && hipMemcpy(I, dI, sizeof(cplx) * (size_t)S * Hn * nb, hipMemcpyDeviceToHost) != hipSuccess) return cleanup(HPF_E_HIP);
    for (int k = 0; k < 5; ++k)
        if (host[k] && hipMemcpy(host[k], dv[k], sizeof(double) * (size_t)S * (k == 4 ? Hn : nb), hipMemcpyDeviceToHost) != hipSuccess)
            return cleanup(HPF_E_HIP);
    return cleanup(HPF_OK);
}

int hpf_branch_stats_begin(hpf_handle* h, const double* rating) {
    if (!h) return HPF_E_ARG;
    const size_t nb = (size_t)h->nb;
    std::vector<double> lim;
    if (!accum_limits(rating, nb, lim)) return HPF_E_ARG;
    int r;
    if ((r = branch_build(h))) return r;
    return accum_open(h, h->bstat, 9 * nb, 3 * nb, nb, lim);
}

int hpf_branch_stats_add(hpf_handle* h, int first_id) { return accum_add(h, &hpf_handle::bstat, branch_add_launch, first_id); }

int hpf_branch_stats_get(hpf_handle* h, int64_t* counts, double* irms_max, int32_t* irms_arg, double* irms_sum, double* irms_sumsq,
                         uint32_t* irms_over, double* loss_max, int32_t* loss_arg, double* loss_sum, double* loss_sumsq, double* lossh_max,
                         int32_t* lossh_arg, double* lossh_sum, double* lossh_sumsq) {
    return accum_get(h, &hpf_handle::bstat, h ? (size_t)h->nb : 0, counts,
                     {irms_max, irms_sum, irms_sumsq, loss_max, loss_sum, loss_sumsq, lossh_max, lossh_sum, lossh_sumsq}, {irms_arg, loss_arg, lossh_arg},
                     {irms_over});
}

int hpf_branch_stats_end(hpf_handle* h) { return accum_end(h, &hpf_handle::bstat); }

// ---- voltage waveforms (hpf_waveform.hpp) ------------------------------------------------------------------------------------------------
int hpf_waveform_table(int T, double* ct, double* st) {
    if (!wave_T_ok(T) || !ct || !st) return HPF_E_ARG;
    wave_table(T, ct, st);
    return HPF_OK;
}

// T and the Hn orders of a waveform call, checked on the host
static bool wave_args_ok(const hpf_handle* h, const int32_t* orders, int T) {
    if (!orders || !wave_T_ok(T)) return false;
    for (int q = 0; q < h->Hn; ++q)
        if (!wave_order_ok(orders[q])) return false;
    return true;
}

int hpf_waveform(hpf_handle* h, const int32_t* orders, int T, int n_sel, const int32_t* sel, double* v, double* peak, int32_t* kpeak, double* crest,
                 double* slack) {
    if (!h) return HPF_E_ARG;
    if (!wave_args_ok(h, orders, T) || n_sel < 0 || (n_sel > 0 && !sel)) return HPF_E_ARG;
    for (int k = 0; k < n_sel; ++k)
        if (sel[k] < 0 || sel[k] >= h->n) return HPF_E_ARG;
    if (!h->state_set || h->S < 1) return HPF_E_STATE;
    const int S = h->S, n = h->n, Hn = h->Hn;
    const size_t count = (size_t)n * Hn, sn = (size_t)S * n;
    std::vector<double> tab(2 * (size_t)T);
    wave_table(T, tab.data(), tab.data() + T);
    double *d_tab = nullptr, *d_v = nullptr, *d_f[3] = {nullptr, nullptr, nullptr};          // peak, crest, slack
    int *d_orders = nullptr, *d_sel = nullptr, *d_k = nullptr;
    double* host[3] = {peak, crest, slack};
    const bool per_bus = peak || kpeak || crest || slack, samples = v && n_sel > 0;
    DevMem tmp(&h->last_detail);
    auto cleanup = [&](int code) {
        hipStreamSynchronize(h->stream);
        tmp.clear();
        return code;
    };
    int r;
    if ((r = tmp.upload(&d_tab, tab)) || (r = tmp.upload(&d_orders, (const int*)orders, (size_t)Hn))) return cleanup(r);
    for (int k = 0; k < 3; ++k)
        if (host[k] && (r = tmp.alloc(&d_f[k], sn))) return cleanup(r);
    if (kpeak && (r = tmp.alloc(&d_k, sn))) return cleanup(r);
    if (samples && ((r = tmp.upload(&d_sel, (const int*)sel, (size_t)n_sel)) || (r = tmp.alloc(&d_v, (size_t)S * n_sel * T)))) return cleanup(r);
    hipLaunchKernelGGL(k_branch_refresh_u, grid2((int)count, S), dim3(TPB), 0, h->stream, (int)count, h->d_Vm, h->d_Va, h->d_U);
    // every bus for the per-bus outputs; the selected buses (in the caller's order, repeats allowed) once more for their samples
    const AccumList every{S, nullptr, nullptr, 0, 0, nullptr};         // (the S scenarios of the batch, whatever their records say)
    if (per_bus)
        wave_peaks_launch(h, T, every, n, nullptr, d_orders, d_tab, d_tab + T, nullptr, d_f[0], d_k, d_f[1], d_f[2]);
    if (samples)
        wave_peaks_launch(h, T, every, n_sel, d_sel, d_orders, d_tab, d_tab + T, d_v, nullptr, nullptr, nullptr, nullptr);
    if (launch_status(h)) return cleanup(HPF_E_HIP);
    if (hipStreamSynchronize(h->stream) != hipSuccess) return cleanup(HPF_E_HIP);
    for (int k = 0; k < 3; ++k)
        if (host[k] && hipMemcpy(host[k], d_f[k], sizeof(double) * sn, hipMemcpyDeviceToHost) != hipSuccess) return cleanup(HPF_E_HIP);
    if (kpeak && hipMemcpy(kpeak, d_k, sizeof(int32_t) * sn, hipMemcpyDeviceToHost) != hipSuccess) return cleanup(HPF_E_HIP);
    if (samples && hipMemcpy(v, d_v, sizeof(double) * (size_t)S * n_sel * T, hipMemcpyDeviceToHost) != hipSuccess) return cleanup(HPF_E_HIP);
    return cleanup(HPF_OK);
}

int hpf_waveform_stats_begin(hpf_handle* h, const int32_t* orders, int T, const double* peak_limit, double crest_limit) {
    if (!h) return HPF_E_ARG;
    if (!wave_args_ok(h, orders, T) || crest_limit != crest_limit) return HPF_E_ARG;
    const size_t n = (size_t)h->n;
    std::vector<double> lim;
    if (!accum_limits(peak_limit, n, lim)) return HPF_E_ARG;
    std::vector<double> ct((size_t)T), st((size_t)T);
    wave_table(T, ct.data(), st.data());
    int r;
    if ((r = accum_open(h, h->wstat, 6 * n, 2 * n, 2 * n, lim))) return r;                 // (an open one is reset: T may differ)
    DevMem& mem = h->wstat.mem;
    if ((r = mem.upload(&h->d_ws_ct, ct)) || (r = mem.upload(&h->d_ws_st, st)) || (r = mem.upload(&h->d_ws_orders, (const int*)orders, (size_t)h->Hn)) ||
        (r = mem.alloc(&h->d_ws_peak, (size_t)h->S_max * n)) || (r = mem.alloc(&h->d_ws_crest, (size_t)h->S_max * n))) {
        accum_close(h->wstat);
        return r;
    }
    h->ws_T = T;
    h->ws_crest_limit = crest_limit;
    return HPF_OK;
}

int hpf_waveform_stats_add(hpf_handle* h, int first_id) { return accum_add(h, &hpf_handle::wstat, wave_add_launch, first_id); }

int hpf_waveform_stats_get(hpf_handle* h, int64_t* counts, double* peak_max, int32_t* peak_arg, double* peak_sum, double* peak_sumsq,
                           uint32_t* peak_over, double* crest_max, int32_t* crest_arg, double* crest_sum, double* crest_sumsq,
                           uint32_t* crest_over) {
    return accum_get(h, &hpf_handle::wstat, h ? (size_t)h->n : 0, counts, {peak_max, peak_sum, peak_sumsq, crest_max, crest_sum, crest_sumsq},
                     {peak_arg, crest_arg}, {peak_over, crest_over});
}

int hpf_waveform_stats_end(hpf_handle* h) { return accum_end(h, &hpf_handle::wstat); }

int hpf_debug_stamps(hpf_handle* h, long long* out, int count) {
    if (!h || !out || !h->d_dbg || count > h->S_max * h->n * 8) return HPF_E_ARG;
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(out, h->d_dbg, sizeof(long long) * count, hipMemcpyDeviceToHost));
    return HPF_OK;
}

int hpf_debug_device_memory(int64_t* blocks, int64_t* bytes) {
    if (blocks) *blocks = devmem_live().blocks.load();
    if (bytes) *bytes = devmem_live().bytes.load();
    return HPF_OK;
}

int hpf_set_option(hpf_handle* h, const char* name, int value) {
    if (!h || !name) return HPF_E_ARG;
    if (!strcmp(name, "scenario_groups")) {         // independent scenario pipelines on separate streams (1..8)
        if (value < 1 || value > 8) return HPF_E_ARG;
        h->n_groups = value;
        return HPF_OK;
    }
    if (!strcmp(name, "block_pivoting")) {          // 1: partial pivoting (wave Gauss-Jordan), 0: static 4x4 blocks on MFMA
        if (value && h->n_ties > 0) return HPF_E_STATE;    // meshed network: the bordered Newton step exists for the static-pivot kernels only
        if (h->gj_mode != (value ? 0 : 1)) h->mismatch_valid = false;     // (static-pivot steps read the bus-major image d_fb, pivoted ones d_f:
        h->gj_mode = value ? 0 : 1;                                       //  a mismatch taken in the other mode left only one of them current)
        return HPF_OK;
    }
    if (!strcmp(name, "pivot_growth_limit_log10")) { // static pivot order: amplification limit of a 4x4 pivot block, 10^value
        if (value < 0 || value > 300) return HPF_E_ARG;
        h->piv_limit = pow(10.0, (double)value);
        return HPF_OK;
    }
    if (!strcmp(name, "keep_previous_state")) {     // hpf_solve keeps, per scenario, the state its last Newton step started from
        if (value && !h->d_Vmp) {
            int rr;
            const size_t cnt = (size_t)h->S_alloc * h->n * h->Hn;
            if ((rr = h->prev_mem.alloc(&h->d_Vmp, cnt)) || (rr = h->prev_mem.alloc(&h->d_Vap, cnt))) {
                h->prev_mem.clear();
                return rr;
            }
        }
        h->keep_prev = value ? 1 : 0;                // (only with both buffers in place)
        return HPF_OK;
    }
    if (!strcmp(name, "border_pivoting")) {         // meshed BLOCK_TREE handles: 1 = the border system always through the pivoted LU
        h->border_pivoting = value ? 1 : 0;
        return HPF_OK;
    }
    if (!strcmp(name, "queue_chunk")) {             // hpf_solve_queue: Newton iterations between two harvest / refill rounds
        if (value < 1 || value > 16) return HPF_E_ARG;
        h->queue_chunk = value;
        return HPF_OK;
    }
    if (!strcmp(name, "step_residual_check")) {     // 1: every harmonic Newton step's backward error on the device (k_step_residual), flags bits 6 / 7
        if (value != 0 && value != 1) return HPF_E_ARG;
        if (value && !h->d_eta) {
            int rr;
            if ((rr = h->resid_mem.alloc(&h->d_respart, (size_t)h->S_alloc * 4 * h->errpart_stride)) ||
                (rr = h->resid_mem.alloc(&h->d_eta, 2 * (size_t)h->S_alloc))) {
                h->resid_mem.clear();
                return rr;
            }
        }
        if (value && !h->resid_check) {
            int rr;
            HIPCHK(hipStreamSynchronize(h->stream));
            if ((rr = reset_step_eta(h))) return rr;
        }
        h->resid_check = value;
        return HPF_OK;
    }
    if (!strcmp(name, "rectangular_update")) {      // 1: the harmonic Newton steps are applied to U = Vm e^(j Va) (k_update_rect), flags bit 9
        if (value != 0 && value != 1) return HPF_E_ARG;
        h->rect_update = value;
        return HPF_OK;
    }
    if (!strcmp(name, "step_residual_limit_log10")) {   // a step is flagged when its eta exceeds 10^value (-16..0, default -10)
        if (value < -16 || value > 0) return HPF_E_ARG;
        h->resid_limit = pow(10.0, (double)value);
        return HPF_OK;
    }
    if (!strcmp(name, "distortion_id_base")) {      // hpf_solve_queue with the distortion or the branch accumulator open: scenario g of a call gets id value + g
        if (value < 0) return HPF_E_ARG;
        h->dist_id_base = value;
        return HPF_OK;
    }
    if (!strcmp(name, "auto_repivot")) {            // 0: flagged scenarios are only reported (flags bit 3), not repeated
        h->auto_repivot = value ? 1 : 0;
        return HPF_OK;
    }
    return HPF_E_ARG;
}

int hpf_set_trace(hpf_handle* h, double* Vm_traj, double* Va_traj, int cap) {
    if (!h || (Vm_traj == nullptr) != (Va_traj == nullptr) || (Vm_traj && cap < 1)) return HPF_E_ARG;
    h->trace_Vm = Vm_traj;
    h->trace_Va = Va_traj;
    h->trace_cap = Vm_traj ? cap : 0;
    return HPF_OK;
}

int hpf_set_stream(hpf_handle* h, void* s) {
    if (!h) return HPF_E_ARG;
    HIPCHK(hipStreamSynchronize(h->stream));
    h->stream = s ? (hipStream_t)s : h->own_stream;
    return HPF_OK;
}

int hpf_sync(hpf_handle* h) {
    if (!h) return HPF_E_ARG;
    HIPCHK(hipStreamSynchronize(h->stream));
    return HPF_OK;
}

int hpf_timing_enable(hpf_handle* h, int on) {
    if (!h) return HPF_E_ARG;
    if (on && !h->d_tstamp && h->solver == HPF_SOLVER_BLOCK_TREE) {
        std::vector<unsigned long long> init(2 * (size_t)hpf_handle::TS_CAP);
        for (size_t i = 0; i < init.size(); i += 2) {
            init[i] = ~0ull;
            init[i + 1] = 0ull;
        }
        int rr = h->mem.upload(&h->d_tstamp, init);
        if (rr) return rr;
    }
    int r = resolve_spans(h);
    h->timing = on == 2 ? 2 : (on != 0 ? 1 : 0);
    return r;
}

int hpf_timing_get(hpf_handle* h, int which, double* ms, int64_t* launches) {
    if (!h || which < 0 || which >= T_COUNT) return HPF_E_ARG;
    int r = resolve_spans(h);
    if (r) return r;
    if (ms) *ms = h->t_ms[which];
    if (launches) *launches = h->t_n[which];
    return HPF_OK;
}

int hpf_timing_reset(hpf_handle* h) {
    if (!h) return HPF_E_ARG;
    int r = resolve_spans(h);
    for (int i = 0; i < T_COUNT; ++i) {
        h->t_ms[i] = 0;
        h->t_n[i] = 0;
    }
    return r;
}

// update_harmonic_state_vec (HG:476-479) as a standalone call: dx = J^-1 f for a caller-supplied dense column-major J
// (rocSOLVER getrf / getrs, partial pivoting).  No handle: the reference function is stateless too.  N * N >= 2^31 (N > 46 340): rocSOLVER's
// 64-bit entry points, exactly as dense_solve does for a handle; a system whose 8 N^2 bytes do not fit the device's free memory is refused with
// HPF_E_NOMEM before anything is allocated (the sparse form of the same call, hpf_sparse_solve, has no such bound).
int hpf_dense_solve(int device, int N, const double* J_colmajor, const double* f, double* dx) {
    if (N < 1 || !J_colmajor || !f || !dx) return HPF_E_ARG;
    if (hipSetDevice(device) != hipSuccess) return HPF_E_HIP;
    const size_t elems = (size_t)N * N;
    const bool wide = elems >= ((size_t)1 << 31);
    {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return HPF_E_HIP;
        // J + rocSOLVER's workspace (a few panels) + pivots: leave 5 % + 64 MiB of headroom
        const double need = 8.0 * (double)elems * 1.05 + 64.0 * 1048576.0;
        if (need > (double)free_b) return HPF_E_NOMEM;
    }
    rocblas_handle blas = nullptr;
    double *dJ = nullptr, *df = nullptr;
    int64_t *dip = nullptr, *dinfo = nullptr;            // (sized for the 64-bit path; the 32-bit one uses the front half)
    int64_t info64 = 0;
    int info32 = 0, rc = HPF_OK;
    if (rocblas_create_handle(&blas) != rocblas_status_success) return HPF_E_ROCSOLVER;
    DevMem tmp;
    if (!(rc = tmp.alloc(&dJ, elems)) && !(rc = tmp.alloc(&df, (size_t)N)) && !(rc = tmp.alloc(&dip, (size_t)N))) rc = tmp.alloc(&dinfo, (size_t)1);
    if (!rc && (hipMemcpy(dJ, J_colmajor, sizeof(double) * elems, hipMemcpyHostToDevice) != hipSuccess ||
                hipMemcpy(df, f, sizeof(double) * N, hipMemcpyHostToDevice) != hipSuccess))
        rc = HPF_E_HIP;
    if (!rc) {
        rocblas_status st;
        if (wide) {
            st = rocsolver_dgetrf_64(blas, N, N, dJ, N, dip, dinfo);
            if (st == rocblas_status_success) st = rocsolver_dgetrs_64(blas, rocblas_operation_none, N, 1, dJ, N, dip, df, N);
        } else {
            st = rocsolver_dgetrf(blas, N, N, dJ, N, reinterpret_cast<int*>(dip), reinterpret_cast<int*>(dinfo));
            if (st == rocblas_status_success)
                st = rocsolver_dgetrs(blas, rocblas_operation_none, N, 1, dJ, N, reinterpret_cast<int*>(dip), df, N);
        }
        if (st == rocblas_status_memory_error)
            rc = HPF_E_NOMEM;
        else if (st != rocblas_status_success)
            rc = HPF_E_ROCSOLVER;
    }
    if (!rc && (hipMemcpy(wide ? (void*)&info64 : (void*)&info32, dinfo, wide ? sizeof(int64_t) : sizeof(int), hipMemcpyDeviceToHost) != hipSuccess ||
                hipMemcpy(dx, df, sizeof(double) * N, hipMemcpyDeviceToHost) != hipSuccess))
        rc = HPF_E_HIP;
    if (!rc && (wide ? info64 != 0 : info32 != 0)) rc = HPF_E_SINGULAR;
    tmp.clear();
    rocblas_destroy_handle(blas);
    return rc;
}

double hpf_solve_flops(const hpf_handle* h) {
    if (!h) return 0.0;
    if (h->solver == HPF_SOLVER_BLOCK_TREE) return active_tree(const_cast<hpf_handle*>(h)).flops_factor;
    const double N = h->N;
    return (2.0 / 3.0) * N * N * N + 2.0 * N * N;
}

double hpf_solve_bytes(const hpf_handle* h) {
    if (!h) return 0.0;
    if (h->solver == HPF_SOLVER_BLOCK_TREE) return active_tree(const_cast<hpf_handle*>(h)).bytes_factor;
    const double N = h->N;
    return 8.0 * (2.0 * N * N + 2.0 * N);           // Jacobian written by the assembly, read and written back by getrf
}

int hpf_kernel_model(const hpf_handle* h, int which, double* bytes, double* flops, int* launches) {
    if (!h) return HPF_E_ARG;
    double by = 0.0, fl = 0.0;
    int ln = 0;
    if (which == T_RESID) {
        // k_step_residual + k_step_eta, one scenario and step.  Bytes: Y, the pattern, U, E, the step, P and Q once (the neighbours' gathers and
        // the mismatch's second walk of the row hit the L2; Y_N is shared by all scenarios).  Flops per stored admittance entry and harmonic: 8
        // (the mismatch's product and sum) + 12 (two complex products of the entry) + 24 (eight fma into r and a, four sums into w); per cross
        // term of a coupled nonlinear bus 12 + 2 + 24, and 8 for its share of the Norton injection.
        const double Hn = h->Hn, nl = h->coupled ? (double)(h->n - h->m) : 0.0;
        by = 16.0 * Hn * h->nnz + 4.0 * (h->nnz + 9.0 * h->n) + 16.0 * Hn * h->n * 3.0 + 16.0 * h->n;
        fl = 44.0 * Hn * h->nnz + nl * Hn * ((Hn - 1.0) * 38.0 + Hn * 8.0);
        ln = 2;
    } else if (h->solver == HPF_SOLVER_BLOCK_TREE) {
        const Tree& T = active_tree(const_cast<hpf_handle*>(h));
        if (which == T_GJ && tree_levels_fused(const_cast<hpf_handle*>(h))) {      // k_level: every dense bus, one launch per level
            by = T.bytes_factor; fl = T.flops_factor; ln = T.n_levels;
        } else if (which == T_GJ) {
            by = T.bytes_gj; fl = T.flops_gj; ln = T.n_gj_launches;
        } else if (which == T_SOLVE) {
            by = T.bytes_factor; fl = T.flops_factor; ln = T.n_levels;
        } else if (which == T_BACK) {
            by = T.bytes_back; fl = T.flops_per_solve - T.flops_factor; ln = T.n_depths;
        } else {
            return HPF_E_ARG;
        }
    } else if (which == T_SOLVE) {
        by = hpf_solve_bytes(h); fl = hpf_solve_flops(h); ln = 1;
    } else {
        return HPF_E_ARG;
    }
    if (bytes) *bytes = by;
    if (flops) *flops = fl;
    if (launches) *launches = ln;
    return HPF_OK;
}

int hpf_tree_census(const hpf_handle* h, int* counts, int n_counts) {
    if (!h || !counts || n_counts < 0) return HPF_E_ARG;
    if (h->solver != HPF_SOLVER_BLOCK_TREE) return HPF_E_STATE;
    const Tree& T = active_tree(const_cast<hpf_handle*>(h));
    int w[CENSUS_WORDS] = {};
    for (int i = 0; i < 8; ++i) w[i] = T.census[i];
    w[CENSUS_TIES] = h->n_ties;
    w[CENSUS_FUSED_LEVELS] = tree_levels_fused(const_cast<hpf_handle*>(h)) ? 1 : 0;
    w[CENSUS_COMPRESS_STEPS] = T.n_comp;
    w[CENSUS_BORDER_REPIVOTS] = h->border_repivots;
    w[CENSUS_BORDER_UNKNOWNS] = h->m_border;
    w[CENSUS_ROOT_PATH_BUSES] = h->mesh_sel ? h->sel_nP : 0;
    w[CENSUS_BORDERED_FORM] = h->mesh_sel ? (h->border_gj ? 2 : 1) : 0;
    w[CENSUS_BACK_WALKS] = (int)h->n_back_walks;
    w[CENSUS_BACK_TAILS] = (int)h->n_back_tails;
    w[CENSUS_BATCH_TILE] = h->last_batch_tile;
    w[CENSUS_LEAF_BATCH_TILE] = h->last_leaf_tile;
    for (int i = 0; i < n_counts; ++i) counts[i] = i < CENSUS_WORDS ? w[i] : 0;
    return HPF_OK;
}

int hpf_setup_times(const hpf_handle* h, double* ms, int n_ms) {
    if (!h || !ms || n_ms < 0) return HPF_E_ARG;
    for (int i = 0; i < n_ms; ++i) ms[i] = i < 4 ? h->setup_ms[i] : 0.0;
    return HPF_OK;
}

int hpf_scenario_groups(const hpf_handle* h, int live) {
    if (!h || live < 0) return HPF_E_ARG;
    return group_count(h->solver == HPF_SOLVER_BLOCK_TREE && h->n_ties == 0, h->n_groups, live);
}

int hpf_tree_plan(const hpf_desc* d, const char* path) {
    if (!d || !path || d->n < 1 || !d->rowptr || !d->col || !d->Yval || !d->dev_of_bus) return HPF_E_ARG;
    if (d->nnz < d->n + 2 * (d->n - 1) || ((d->nnz - d->n) & 1)) return HPF_E_TOPOLOGY;           // (a connected symmetric pattern has at least the tree's entries)
    if (d->max_scenarios < 1) return HPF_E_ARG;
    remove(path);                                                           // (a stale file of an earlier run must not pass for this one)
    return tree_plan_dump(d, path);
}

double hpf_back_bytes(const hpf_handle* h) {
    if (!h || h->solver != HPF_SOLVER_BLOCK_TREE) return 0.0;
    return active_tree(const_cast<hpf_handle*>(h)).bytes_back;
}

}  // extern "C"
