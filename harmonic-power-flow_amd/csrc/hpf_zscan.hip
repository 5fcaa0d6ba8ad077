// hpf_impedance_scan: driving-point and transfer impedances over a grid of harmonic orders (hpf_zscan.hpp has the arithmetic and the planner;
// include/hpf.h the contract).  Every kernel maps a thread to (item, frequency point) with the frequency fastest: block b of a launch over m items
// serves item b / fb, points (b % fb) * ZS_TPB + threadIdx.x, fb = ceil(Fc / ZS_TPB) -- a one-dimensional grid, so that the widest depth of a large
// star still fits; the host keeps n * fb <= 2^30.  hpf_penetration (below, hpf_penetration.hpp) and hpf_resonance_modes (last, hpf_resonance.hpp)
// need the same Y(h): ZsFactor is the one host driver of the factor of a chunk (the scan's kernels) and of y = Y^-1 x (the penetration's walks);
// the three entry points keep their own checks, chunk lengths, buffers and outputs.
#include <algorithm>
#include <utility>

#include "hpf_internal.hpp"
#include "hpf_penetration.hpp"
#include "hpf_resonance.hpp"
#include "hpf_zscan.hpp"

using namespace hpf;

namespace {

constexpr int ZS_TPB = 256;

__device__ __forceinline__ bool zs_item(int m, int Fc, int& item, int& f) {
    const int fb = (Fc + ZS_TPB - 1) / ZS_TPB;
    item = (int)(blockIdx.x / (unsigned)fb);
    f = (int)(blockIdx.x % (unsigned)fb) * ZS_TPB + (int)threadIdx.x;
    return item < m && f < Fc;
}

// upward walk, the m buses `nodes` of one depth: w, t [n][Fc]; hh [Fc] the chunk's orders; yx [n][Fc] or NULL
__global__ __launch_bounds__(ZS_TPB) void k_zscan_up(ZscanView V, const int* __restrict__ nodes, int m, int Fc, const double* __restrict__ hh,
                                                     const cplx* __restrict__ yx, cplx* __restrict__ w, cplx* __restrict__ t) {
    int bi, f;
    if (!zs_item(m, Fc, bi, f)) return;
    const int i = nodes[bi];
    const size_t o = (size_t)i * Fc + f;
    cplx wi, ti;
    zscan_up(V, i, hh[f], yx != nullptr, yx ? yx[o] : cplx{0.0, 0.0}, t, (size_t)Fc, (size_t)f, wi, ti);
    w[o] = wi;
    t[o] = ti;
}

// downward walk of one depth: Zd [n][Fc]
__global__ __launch_bounds__(ZS_TPB) void k_zscan_down(ZscanView V, const int* __restrict__ nodes, int m, int Fc, const cplx* __restrict__ w,
                                                       const cplx* __restrict__ t, cplx* __restrict__ Zd) {
    int bi, f;
    if (!zs_item(m, Fc, bi, f)) return;
    const int i = nodes[bi], p = V.parent[i];
    const size_t o = (size_t)i * Fc + f;
    Zd[o] = p < 0 ? w[o] : zscan_down(w[o], t[o], Zd[(size_t)p * Fc + f]);
}

// columns: the walk up from bus colbus[s] of each of the ncol columns; cols [ncol][n][Fc]
__global__ __launch_bounds__(ZS_TPB) void k_zscan_col_walk(ZscanView V, const int* __restrict__ colbus, int ncol, int Fc, const cplx* __restrict__ t,
                                                           const cplx* __restrict__ Zd, cplx* __restrict__ cols) {
    int s, f;
    if (!zs_item(ncol, Fc, s, f)) return;
    zscan_col_walk(V.parent, colbus[s], t, Zd, cols + (size_t)s * V.n * Fc, (size_t)Fc, (size_t)f);
}

// columns: the buses of one depth that no walk wrote (path [ncol][n]: 1 on the column bus and its ancestors), column blockIdx.y
__global__ __launch_bounds__(ZS_TPB) void k_zscan_col_fill(ZscanView V, const int* __restrict__ nodes, int m, int Fc,
                                                           const unsigned char* __restrict__ path, const cplx* __restrict__ t,
                                                           cplx* __restrict__ cols) {
    int bi, f;
    if (!zs_item(m, Fc, bi, f)) return;
    const int i = nodes[bi], s = blockIdx.y;
    if (path[(size_t)s * V.n + i]) return;
    cplx* col = cols + (size_t)s * V.n * Fc;
    col[(size_t)i * Fc + f] = zscan_col_fill(t[(size_t)i * Fc + f], col[(size_t)V.parent[i] * Fc + f]);
}

// ties: W^-1 of every point; tc = the 2 k tie columns
__global__ __launch_bounds__(ZS_TPB) void k_zscan_tie_winv(int k, const int* __restrict__ ta, const int* __restrict__ tb, const double* __restrict__ tR,
                                                           const double* __restrict__ tX, int n, int Fc, const double* __restrict__ hh,
                                                           const cplx* __restrict__ tc, cplx* __restrict__ Winv) {
    int z, f;
    if (!zs_item(1, Fc, z, f)) return;
    zscan_tie_winv(k, ta, tb, tR, tX, hh[f], tc, (size_t)n, (size_t)Fc, (size_t)f, Winv);
}

// ties: the correction of the diagonal (colbus NULL: row blockIdx.y = 0, target Zd) or of the selected columns (column blockIdx.y of `target`)
__global__ __launch_bounds__(ZS_TPB) void k_zscan_tie_fix(int k, int n, int Fc, const cplx* __restrict__ tc, const cplx* __restrict__ Winv,
                                                          const int* __restrict__ colbus, cplx* __restrict__ target) {
    int i, f;
    if (!zs_item(n, Fc, i, f)) return;
    const int s = blockIdx.y, j = colbus ? colbus[s] : i;
    cplx* z = target + ((size_t)s * n + i) * Fc + f;
    *z = csub(*z, zscan_tie_form(k, tc, Winv, (size_t)n, (size_t)Fc, (size_t)f, i, j));
}

// peaks: one wavefront per bus reduces the chunk's Fc points (grid index f0 + f) and folds the result into the bus's running peak (pkey, pf) --
// chunks arrive in ascending order on one stream, lane 0 is the only writer of its bus.  bad[i] |= a non-finite Z_ii.  No atomics.
__global__ __launch_bounds__(ZS_TPB) void k_zscan_peaks(int n, int Fc, int f0, const cplx* __restrict__ Zd, unsigned long long* __restrict__ pkey,
                                                        int* __restrict__ pf, int* __restrict__ bad) {
    const int i = blockIdx.x * (ZS_TPB / 64) + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= n) return;                                  // (a whole wavefront)
    uint64_t key = 0;
    int fbest = ZSCAN_NO_F, nonfinite = 0;
    for (int f = lane; f < Fc; f += 64) {
        const cplx z = Zd[(size_t)i * Fc + f];
        nonfinite |= !zscan_finite(z);
        wave_peak_combine(key, fbest, wave_key(zscan_abs(z)), f0 + f);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long key2 = __shfl_xor((unsigned long long)key, off, 64);
        const int f2 = __shfl_xor(fbest, off, 64);
        nonfinite |= __shfl_xor(nonfinite, off, 64);
        wave_peak_combine(key, fbest, (uint64_t)key2, f2);
    }
    if (lane != 0) return;
    uint64_t k0 = pkey[i];
    int fp = pf[i];
    wave_peak_combine(k0, fp, key, fbest);
    pkey[i] = k0;
    pf[i] = fp;
    if (nonfinite) bad[i] = 1;
}

__global__ void k_zscan_peaks_init(int n, unsigned long long* __restrict__ pkey, int* __restrict__ pf, int* __restrict__ bad) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    pkey[i] = 0ull;
    pf[i] = ZSCAN_NO_F;
    bad[i] = 0;
}

// out [C][R] <- in [R][C] (complex): 32 x 32 tiles through LDS, so that loads and stores both run along rows; tile b of a one-dimensional grid
constexpr int ZS_TILE = 32;
__global__ __launch_bounds__(ZS_TILE * 8) void k_zscan_transpose(const cplx* __restrict__ in, long long R, long long C, cplx* __restrict__ out) {
    __shared__ cplx tile[ZS_TILE][ZS_TILE + 1];
    const long long tc = (C + ZS_TILE - 1) / ZS_TILE;
    const long long r0 = (long long)(blockIdx.x / (unsigned long long)tc) * ZS_TILE, c0 = (long long)(blockIdx.x % (unsigned long long)tc) * ZS_TILE;
    const int tx = threadIdx.x & (ZS_TILE - 1), ty = threadIdx.x / ZS_TILE;
    for (int y = ty; y < ZS_TILE; y += 8)
        if (r0 + y < R && c0 + tx < C) tile[y][tx] = in[(size_t)(r0 + y) * C + (c0 + tx)];
    __syncthreads();
    for (int y = ty; y < ZS_TILE; y += 8)
        if (c0 + y < C && r0 + tx < R) out[(size_t)(c0 + y) * R + (r0 + tx)] = tile[tx][y];
}

bool finite_all(const double* a, size_t count) {
    for (size_t k = 0; k < count; ++k)
        if (!(fabs(a[k]) <= 1.79769313486231570815e308)) return false;
    return true;
}

// the host checks of hpf_impedance_scan (before any HIP call)
bool zscan_args_ok(const hpf_zscan_net* net, int F, const double* h, const double* y_extra, int n_sel, const int32_t* sel, int chunk, double* Zt) {
    if (!net || !h) return false;
    const int n = net->n, nb = net->nb;
    if (n < 1 || n > ZSCAN_MAX_N || nb < 0 || F < 1 || F > ZSCAN_MAX_F || chunk < 0) return false;
    if (!net->gsh || !net->bsh || !net->xsh || (nb > 0 && (!net->from || !net->to || !net->R || !net->X))) return false;
    if (n_sel < 0 || n_sel > ZSCAN_MAX_SEL || (n_sel > 0 && (!sel || !Zt))) return false;
    for (int k = 0; k < n_sel; ++k)
        if (sel[k] < 0 || sel[k] >= n) return false;
    std::vector<std::pair<int, int>> pairs((size_t)nb);
    for (int e = 0; e < nb; ++e) {
        if (net->from[e] < 0 || net->to[e] >= n || net->from[e] >= net->to[e]) return false;
        pairs[e] = {net->from[e], net->to[e]};
    }
    std::sort(pairs.begin(), pairs.end());
    if (std::adjacent_find(pairs.begin(), pairs.end()) != pairs.end()) return false;
    if (!finite_all(net->R, nb) || !finite_all(net->X, nb) || !finite_all(net->gsh, n) || !finite_all(net->bsh, n) || !finite_all(net->xsh, n) ||
        !finite_all(h, F) || (y_extra && !finite_all(y_extra, (size_t)2 * F * n)))
        return false;
    for (int e = 0; e < nb; ++e)
        if (net->R[e] == 0.0 && net->X[e] == 0.0) return false;
    for (int f = 0; f < F; ++f)
        if (!(h[f] > 0.0)) return false;
    return true;
}

unsigned zs_grid(long long items, int Fc) { return (unsigned)(items * ((Fc + ZS_TPB - 1) / ZS_TPB)); }

// the one-dimensional grid of a kernel that takes 32 x 32 tiles of an [a][b] matrix
unsigned zs_tiles(long long a, long long b) { return (unsigned)(((a + ZS_TILE - 1) / ZS_TILE) * ((b + ZS_TILE - 1) / ZS_TILE)); }

void zs_transpose(hipStream_t st, const cplx* in, long long R, long long C, cplx* out) {
    hipLaunchKernelGGL(k_zscan_transpose, dim3(zs_tiles(R, C)), dim3(ZS_TILE * 8), 0, st, in, R, C, out);
}

// a launch over n buses may have (2^30) / n blocks of ZS_TPB points: an automatic chunk length is clipped to that, a forced one has to fit (false)
bool zs_clip_chunk(int n, int chunk, int& Fc) {
    const long long fb_max = (1ll << 30) / n;
    if ((Fc + ZS_TPB - 1) / ZS_TPB <= fb_max) return true;
    if (chunk > 0) return false;
    Fc = (int)fb_max * ZS_TPB;
    return true;
}

// the end of a call, on every path after hipSetDevice: the per-call workspace is gone before the code goes back
int zs_done(DevMem& ws, int code) {
    hipDeviceSynchronize();
    ws.clear();
    return code;
}

// Y(h) of one call: the plan, the ties, the model and the factor of one chunk of frequency points on the device (w, t, Zd where wanted, the columns
// of the selected buses and of the ties, W^-1), and the solve with it.  The blocks belong to the caller's DevMem, which records the ADDRESS of every
// pointer below: the object is neither copied nor moved, and it is declared before the DevMem local that nulls its pointers.
struct ZsFactor {
    ZscanPlan P;
    ZscanTies T;
    ZscanView V{};
    const hpf_zscan_net* net = nullptr;
    const double* h = nullptr;
    int n = 0, F = 0;
    bool diag = false;                                   // the downward walk runs: Zd is wanted, or the tie columns read it
    int *d_parent = nullptr, *d_pbranch = nullptr, *d_child_ptr = nullptr, *d_child = nullptr, *d_inc_ptr = nullptr, *d_inc = nullptr;
    int *d_nodes = nullptr, *d_colbus = nullptr, *d_ta = nullptr, *d_tb = nullptr;
    double *d_R = nullptr, *d_X = nullptr, *d_gsh = nullptr, *d_bsh = nullptr, *d_xsh = nullptr, *d_h = nullptr, *d_tR = nullptr, *d_tX = nullptr;
    unsigned char* d_path = nullptr;
    cplx *d_w = nullptr, *d_t = nullptr, *d_Zd = nullptr, *d_yx = nullptr, *d_cols = nullptr, *d_Winv = nullptr;

    ZsFactor() = default;
    ZsFactor(const ZsFactor&) = delete;
    ZsFactor& operator=(const ZsFactor&) = delete;

    // the host part, before any HIP call (the arguments passed zscan_args_ok): HPF_OK or HPF_E_TOPOLOGY
    int plan(const hpf_zscan_net* net_, int F_, const double* h_, int n_sel = 0, const int32_t* sel = nullptr) {
        net = net_, h = h_, n = net_->n, F = F_;
        const int r = zscan_plan(n, net->nb, net->from, net->to, P);
        if (r == HPF_OK) T = zscan_ties(P, net->from, net->to, net->R, net->X, n_sel, sel);
        return r;
    }

    // plan, model and orders up, the arrays of a chunk of Fc points allocated; on a failure the caller clears ws
    int upload(DevMem& ws, int Fc, bool has_x, bool want_diag) {
        const size_t nF = (size_t)n * Fc, nb = (size_t)net->nb;
        const int k = T.k;
        int r;
        diag = want_diag || k;
        if ((r = ws.upload(&d_parent, P.parent)) || (r = ws.upload(&d_pbranch, P.pbranch)) || (r = ws.upload(&d_child_ptr, P.child_ptr)) ||
            (r = ws.upload(&d_child, P.child)) || (r = ws.upload(&d_inc_ptr, P.inc_ptr)) || (r = ws.upload(&d_inc, P.inc)) ||
            (r = ws.upload(&d_nodes, P.dep_nodes)) || (r = ws.upload(&d_R, net->R, nb)) || (r = ws.upload(&d_X, net->X, nb)) ||
            (r = ws.upload(&d_gsh, net->gsh, (size_t)n)) || (r = ws.upload(&d_bsh, net->bsh, (size_t)n)) ||
            (r = ws.upload(&d_xsh, net->xsh, (size_t)n)) || (r = ws.upload(&d_h, h, (size_t)F)) || (r = ws.alloc(&d_w, nF)) ||
            (r = ws.alloc(&d_t, nF)))
            return r;
        if (diag && (r = ws.alloc(&d_Zd, nF))) return r;
        if (has_x && (r = ws.alloc(&d_yx, nF))) return r;
        if (T.ncol && ((r = ws.upload(&d_colbus, T.colbus)) || (r = ws.upload(&d_path, T.path)) || (r = ws.alloc(&d_cols, (size_t)T.ncol * nF))))
            return r;
        if (k && ((r = ws.upload(&d_ta, T.ta)) || (r = ws.upload(&d_tb, T.tb)) || (r = ws.upload(&d_tR, T.tR)) || (r = ws.upload(&d_tX, T.tX)) ||
                  (r = ws.alloc(&d_Winv, (size_t)k * k * Fc))))
            return r;
        V = ZscanView{n, d_parent, d_pbranch, d_child_ptr, d_child, d_inc_ptr, d_inc, d_R, d_X, d_gsh, d_bsh, d_xsh};
        return HPF_OK;
    }

    // launch(the buses of the depth, their number) for every depth but the first `skip` ones of the order: the root first, or the deepest depth first
    template <class L>
    void depths(bool root_first, int skip, L launch) const {
        for (int q = skip; q < P.n_depths; ++q) {
            const int d = root_first ? q : P.n_depths - 1 - q;
            launch(d_nodes + P.dep_ptr[d], P.dep_ptr[d + 1] - P.dep_ptr[d]);
        }
    }

    // the tie columns of a chunk of fc points: behind the selected ones
    const cplx* tie_cols(int fc) const { return d_cols + (size_t)T.n_sel * n * fc; }

    // the factor of the fc points from f0 on; y_extra (the caller's, or NULL) passes through `stage` [fc][n].  HPF_OK or HPF_E_HIP (the copy)
    int factor(hipStream_t st, int f0, int fc, const double* y_extra, cplx* stage) {
        const int k = T.k, ncol = T.ncol;
        const double* hh = d_h + f0;
        const dim3 tpb(ZS_TPB);
        if (y_extra) {
            if (hipMemcpy(stage, y_extra + (size_t)2 * f0 * n, sizeof(cplx) * (size_t)fc * n, hipMemcpyHostToDevice) != hipSuccess) return HPF_E_HIP;
            zs_transpose(st, stage, fc, n, d_yx);
        }
        depths(false, 0, [&](const int* nodes, int m) {
            hipLaunchKernelGGL(k_zscan_up, dim3(zs_grid(m, fc)), tpb, 0, st, V, nodes, m, fc, hh, d_yx, d_w, d_t);
        });
        if (diag)
            depths(true, 0, [&](const int* nodes, int m) {
                hipLaunchKernelGGL(k_zscan_down, dim3(zs_grid(m, fc)), tpb, 0, st, V, nodes, m, fc, d_w, d_t, d_Zd);
            });
        if (ncol) {
            hipLaunchKernelGGL(k_zscan_col_walk, dim3(zs_grid(ncol, fc)), tpb, 0, st, V, d_colbus, ncol, fc, d_t, d_Zd, d_cols);
            depths(true, 1, [&](const int* nodes, int m) {
                hipLaunchKernelGGL(k_zscan_col_fill, dim3(zs_grid(m, fc), ncol), tpb, 0, st, V, nodes, m, fc, d_path, d_t, d_cols);
            });
        }
        if (k) hipLaunchKernelGGL(k_zscan_tie_winv, dim3(zs_grid(1, fc)), tpb, 0, st, k, d_ta, d_tb, d_tR, d_tX, n, fc, hh, tie_cols(fc), d_Winv);
        return HPF_OK;
    }

    // r [n][fc sc] <- Y^-1 r in place, with the factor of the chunk; coef [k][fc sc] (defined behind the penetration's kernels)
    void solve(hipStream_t st, int fc, int sc, cplx* r, cplx* coef) const;
};

}  // namespace

extern "C" int hpf_impedance_scan(int device, const hpf_zscan_net* net, int F, const double* h, const double* y_extra, int n_sel, const int32_t* sel,
                                  int chunk, double* Z, double* Zt, double* zpeak, int32_t* fpeak) {
    if (!zscan_args_ok(net, F, h, y_extra, n_sel, sel, chunk, Zt)) return HPF_E_ARG;
    ZsFactor Y;
    int r = Y.plan(net, F, h, n_sel, sel);
    if (r != HPF_OK) return r;
    const int n = net->n, k = Y.T.k;
    const size_t stage_rows = zscan_stage_rows(n, n_sel, y_extra != nullptr, Z != nullptr);
    int Fc = zscan_chunk(F, chunk, zscan_per_f(n, k, n_sel, y_extra != nullptr, Z != nullptr));
    if (!zs_clip_chunk(n, chunk, Fc)) return HPF_E_ARG;

    if (hipSetDevice(device) != hipSuccess) return HPF_E_HIP;
    int detail = 0;
    int *d_pf = nullptr, *d_bad = nullptr;
    unsigned long long* d_pkey = nullptr;
    cplx* d_stage = nullptr;
    DevMem ws(&detail);                                  // per-call workspace (declared after the pointers it nulls): gone on every return path
    if ((r = Y.upload(ws, Fc, y_extra != nullptr, true)) || (r = ws.alloc(&d_pkey, (size_t)n)) || (r = ws.alloc(&d_pf, (size_t)n)) ||
        (r = ws.alloc(&d_bad, (size_t)n)))
        return zs_done(ws, r);
    if (stage_rows && (r = ws.alloc(&d_stage, stage_rows * Fc))) return zs_done(ws, r);

    const hipStream_t st = nullptr;
    hipLaunchKernelGGL(k_zscan_peaks_init, dim3((n + 255) / 256), dim3(256), 0, st, n, d_pkey, d_pf, d_bad);
    for (int f0 = 0; f0 < F; f0 += Fc) {
        const int fc = std::min(Fc, F - f0);             // (the arrays of a short last chunk are [bus][fc])
        if ((r = Y.factor(st, f0, fc, y_extra, d_stage))) return zs_done(ws, r);
        if (k) {                                         // the ties' correction of the diagonal and of the selected columns
            const cplx* tc = Y.tie_cols(fc);
            hipLaunchKernelGGL(k_zscan_tie_fix, dim3(zs_grid(n, fc), 1), dim3(ZS_TPB), 0, st, k, n, fc, tc, Y.d_Winv, (const int*)nullptr, Y.d_Zd);
            if (n_sel)
                hipLaunchKernelGGL(k_zscan_tie_fix, dim3(zs_grid(n, fc), n_sel), dim3(ZS_TPB), 0, st, k, n, fc, tc, Y.d_Winv, Y.d_colbus, Y.d_cols);
        }
        hipLaunchKernelGGL(k_zscan_peaks, dim3((n + ZS_TPB / 64 - 1) / (ZS_TPB / 64)), dim3(ZS_TPB), 0, st, n, fc, f0, Y.d_Zd, d_pkey, d_pf, d_bad);
        if (Z) {
            zs_transpose(st, Y.d_Zd, n, fc, d_stage);
            if (hipMemcpy(Z + (size_t)2 * f0 * n, d_stage, sizeof(cplx) * (size_t)fc * n, hipMemcpyDeviceToHost) != hipSuccess)
                return zs_done(ws, HPF_E_HIP);
        }
        if (n_sel) {
            zs_transpose(st, Y.d_cols, (long long)n_sel * n, fc, d_stage);
            if (hipMemcpy(Zt + (size_t)2 * f0 * n_sel * n, d_stage, sizeof(cplx) * (size_t)fc * n_sel * n, hipMemcpyDeviceToHost) != hipSuccess)
                return zs_done(ws, HPF_E_HIP);
        }
        if (hipGetLastError() != hipSuccess) return zs_done(ws, HPF_E_HIP);
    }
    std::vector<unsigned long long> pkey((size_t)n);
    std::vector<int> pf((size_t)n), bad((size_t)n);
    if (hipMemcpy(pkey.data(), d_pkey, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(pf.data(), d_pf, sizeof(int) * n, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(bad.data(), d_bad, sizeof(int) * n, hipMemcpyDeviceToHost) != hipSuccess)
        return zs_done(ws, HPF_E_HIP);
    bool singular = false;
    for (int i = 0; i < n; ++i) {
        if (zpeak) zpeak[i] = wave_key_value(pkey[i]);
        if (fpeak) fpeak[i] = pf[i];
        singular |= bad[i] != 0;
    }
    return zs_done(ws, singular ? HPF_E_SINGULAR : HPF_OK);
}

// ---- hpf_penetration ---------------------------------------------------------------------------------------------------------------------------
// V(h) = Y(h)^-1 I(h) for S scenarios (hpf_penetration.hpp has the arithmetic; include/hpf.h the contract).  The factor of a chunk of fc frequency
// points (w, t, the tie columns, W^-1) is ZsFactor::factor, the two walks and the tie correction ZsFactor::solve; the right-hand sides of a chunk of sc scenarios live in place as
// r [n][J], j = f sc + s, J = fc sc.  The walks map a thread to (bus of the depth, j) with j fastest (zs_item over J): a wavefront reads 64
// consecutive values of r and, with sc >= 64, one w_i / t_i.
namespace {

// r [inj[q]][f sc + s] <- in [s][f][q] (the caller's currents of the chunk, [sc][fc][n_inj]): 32 x 32 tiles over (s, q) of one point f through LDS,
// so that the loads run along q and the stores along s; tile b of a one-dimensional grid
__global__ __launch_bounds__(ZS_TILE * 8) void k_pen_scatter(const cplx* __restrict__ in, const int* __restrict__ inj, int n_inj, int fc, int sc,
                                                             cplx* __restrict__ r) {
    __shared__ cplx tile[ZS_TILE][ZS_TILE + 1];
    const long long tq = (n_inj + ZS_TILE - 1) / ZS_TILE, ts = (sc + ZS_TILE - 1) / ZS_TILE, b = blockIdx.x;
    const int f = (int)(b / (ts * tq)), s0 = (int)(b % (ts * tq) / tq) * ZS_TILE, q0 = (int)(b % tq) * ZS_TILE;
    const int tx = threadIdx.x & (ZS_TILE - 1), ty = threadIdx.x / ZS_TILE;
    const size_t J = (size_t)fc * sc;
    for (int y = ty; y < ZS_TILE; y += 8)
        if (s0 + y < sc && q0 + tx < n_inj) tile[y][tx] = in[((size_t)(s0 + y) * fc + f) * n_inj + (q0 + tx)];
    __syncthreads();
    for (int y = ty; y < ZS_TILE; y += 8)
        if (q0 + y < n_inj && s0 + tx < sc) r[(size_t)inj[q0 + y] * J + (size_t)f * sc + (s0 + tx)] = tile[tx][y];
}

// upward walk of the right-hand sides, the m buses `nodes` of one depth: r_i gathers t_c r_c of its children (t_c stays in registers while applied)
__global__ __launch_bounds__(ZS_TPB) void k_pen_up(ZscanView V, const int* __restrict__ nodes, int m, int fc, int sc, const cplx* __restrict__ t,
                                                   cplx* r) {
    int bi, j;
    if (!zs_item(m, fc * sc, bi, j)) return;
    const int i = nodes[bi];
    if (V.child_ptr[i] == V.child_ptr[i + 1]) return;    // a leaf: r_i = b_i
    const size_t J = (size_t)fc * sc;
    r[(size_t)i * J + j] = pen_up(V.child_ptr, V.child, i, t, r, (size_t)fc, J, (size_t)(j / sc), (size_t)j);
}

// downward walk of one depth: V overwrites r
__global__ __launch_bounds__(ZS_TPB) void k_pen_down(ZscanView V, const int* __restrict__ nodes, int m, int fc, int sc, const cplx* __restrict__ w,
                                                     const cplx* __restrict__ t, cplx* r) {
    int bi, j;
    if (!zs_item(m, fc * sc, bi, j)) return;
    const int i = nodes[bi], p = V.parent[i];
    const size_t J = (size_t)fc * sc, o = (size_t)i * J + j, fo = (size_t)i * fc + j / sc;
    r[o] = p < 0 ? pen_down_root(w[fo], r[o]) : pen_down(w[fo], r[o], t[fo], r[(size_t)p * J + j]);
}

// ties: the k coefficients c_l of every j -> coef [k][J]
__global__ __launch_bounds__(ZS_TPB) void k_pen_tie_coef(int k, const int* __restrict__ ta, const int* __restrict__ tb, int fc, int sc,
                                                         const cplx* __restrict__ Winv, const cplx* __restrict__ r, cplx* __restrict__ coef) {
    int z, j;
    if (!zs_item(1, fc * sc, z, j)) return;
    pen_tie_coef(k, ta, tb, Winv, r, (size_t)fc, (size_t)fc * sc, (size_t)(j / sc), (size_t)j, coef);
}

// ties: V'_i = V_i - sum_l u_l[i] c_l
__global__ __launch_bounds__(ZS_TPB) void k_pen_tie_fix(int k, int n, int fc, int sc, const cplx* __restrict__ tc, const cplx* __restrict__ coef,
                                                        cplx* __restrict__ r) {
    int i, j;
    if (!zs_item(n, fc * sc, i, j)) return;
    const size_t J = (size_t)fc * sc, o = (size_t)i * J + j;
    r[o] = pen_tie_fix(k, tc, coef, (size_t)n, (size_t)fc, J, (size_t)(j / sc), (size_t)j, i, r[o]);
}

// statistics: a row-wise SEQUENTIAL fold of a [rows][cols] matrix, one lane per row, one wavefront per block.  The wavefront loads 64 rows x 32
// columns at a time along the rows (two 512-byte segments per load instruction), leaves the derived value in LDS, and every lane then folds its own
// row in ascending column order (pen_stat_add) -- the order the sums over the scenarios are defined in.
//   RSS = false: the matrix is r viewed as [n fc][sc] (row p = i fc + f), value = |V|; the running statistics of row p are those of (f0 + f, i),
//                carried from scenario chunk to scenario chunk (c_start = s0; fresh at s0 = 0).  *bad = 1 for a non-finite V.
//   RSS = true:  the matrix is the finished sums of squares [n][S], value = sqrt, written back in place (the rss of (i, s)); the statistics of row i.
constexpr int PEN_FOLD_COLS = 32;
template <bool RSS>
__global__ __launch_bounds__(64) void k_pen_fold(long long rows, int cols, int c_start, int n, int fc, int f0, const cplx* __restrict__ r,
                                                 double* __restrict__ sq, unsigned long long* __restrict__ key, int* __restrict__ arg,
                                                 double* __restrict__ sum, double* __restrict__ sumsq, int* __restrict__ bad) {
    __shared__ double tile[64][PEN_FOLD_COLS + 1];
    const int lane = threadIdx.x, tx = lane & (PEN_FOLD_COLS - 1);
    const long long p0 = (long long)blockIdx.x * 64, p = p0 + lane;
    size_t g = 0;
    PenStat st = pen_stat_start();
    if (p < rows) {
        g = RSS ? (size_t)p : (size_t)(f0 + (int)(p % fc)) * n + (size_t)(p / fc);
        if (c_start != 0) st = {key[g], arg[g], sum[g], sumsq[g]};
    }
    int nonfinite = 0;
    for (int c0 = 0; c0 < cols; c0 += PEN_FOLD_COLS) {
        for (int y = lane / PEN_FOLD_COLS; y < 64; y += 64 / PEN_FOLD_COLS)
            if (p0 + y < rows && c0 + tx < cols) {
                const size_t o = (size_t)(p0 + y) * cols + (c0 + tx);
                if (RSS) {
                    const double a = sqrt(sq[o]);
                    sq[o] = a;
                    tile[y][tx] = a;
                } else {
                    const cplx v = r[o];
                    nonfinite |= !zscan_finite(v);
                    tile[y][tx] = zscan_abs(v);
                }
            }
        __syncthreads();
        if (p < rows) {
            const int cn = cols - c0 < PEN_FOLD_COLS ? cols - c0 : PEN_FOLD_COLS;
            for (int c = 0; c < cn; ++c) pen_stat_add(st, tile[lane][c], c_start + c0 + c);
        }
        __syncthreads();
    }
    if (p < rows) {
        key[g] = st.key;
        arg[g] = st.arg;
        sum[g] = st.sum;
        sumsq[g] = st.sumsq;
    }
    if (!RSS && nonfinite) *bad = 1;                     // (every writer stores the same value)
}

// rss: the running sum of squares of (bus, scenario) takes the chunk's fc points in ascending order; sq [n][S] (fresh at f0 = 0)
__global__ __launch_bounds__(ZS_TPB) void k_pen_fold_sq(int n, int fc, int sc, int f0, int s0, int S, const cplx* __restrict__ r,
                                                        double* __restrict__ sq) {
    int i, s;
    if (!zs_item(n, sc, i, s)) return;
    const size_t J = (size_t)fc * sc, o = (size_t)i * S + s0 + s;
    double acc = f0 == 0 ? 0.0 : sq[o];
    for (int f = 0; f < fc; ++f) acc = acc + pen_sq(r[(size_t)i * J + (size_t)f * sc + s]);
    sq[o] = acc;
}

// out [s][f][i] <- r [i][f sc + s] (the chunk's V in the caller's order, [sc][fc][n]): 32 x 32 tiles over (i, s) of one point f through LDS
__global__ __launch_bounds__(ZS_TILE * 8) void k_pen_copy_out(const cplx* __restrict__ r, int n, int fc, int sc, cplx* __restrict__ out) {
    __shared__ cplx tile[ZS_TILE][ZS_TILE + 1];
    const long long ts = (sc + ZS_TILE - 1) / ZS_TILE, ti = (n + ZS_TILE - 1) / ZS_TILE, b = blockIdx.x;
    const int f = (int)(b / (ti * ts)), i0 = (int)(b % (ti * ts) / ts) * ZS_TILE, s0 = (int)(b % ts) * ZS_TILE;
    const int tx = threadIdx.x & (ZS_TILE - 1), ty = threadIdx.x / ZS_TILE;
    const size_t J = (size_t)fc * sc;
    for (int y = ty; y < ZS_TILE; y += 8)
        if (i0 + y < n && s0 + tx < sc) tile[y][tx] = r[(size_t)(i0 + y) * J + (size_t)f * sc + (s0 + tx)];
    __syncthreads();
    for (int y = ty; y < ZS_TILE; y += 8)
        if (s0 + y < sc && i0 + tx < n) out[((size_t)(s0 + y) * fc + f) * n + (i0 + tx)] = tile[tx][y];
}

// the host checks of hpf_penetration beyond the scan's (before any HIP call)
bool pen_args_ok(int n, int F, int S, int n_inj, const int32_t* inj, const double* I, int chunk_f, int chunk_s) {
    if (S < 1 || S > PEN_MAX_S || n_inj < 1 || n_inj > n || !inj || !I || chunk_f < 0 || chunk_s < 0 || (long long)S * n > PEN_MAX_SN) return false;
    std::vector<char> seen((size_t)n, 0);
    for (int q = 0; q < n_inj; ++q) {
        if (inj[q] < 0 || inj[q] >= n || seen[inj[q]]) return false;
        seen[inj[q]] = 1;
    }
    return finite_all(I, (size_t)2 * S * F * n_inj);
}

void ZsFactor::solve(hipStream_t st, int fc, int sc, cplx* r, cplx* coef) const {
    const int k = T.k, J = fc * sc;
    const dim3 tpb(ZS_TPB);
    depths(false, 1, [&](const int* nodes, int m) {      // (the deepest depth holds leaves only)
        hipLaunchKernelGGL(k_pen_up, dim3(zs_grid(m, J)), tpb, 0, st, V, nodes, m, fc, sc, d_t, r);
    });
    depths(true, 0, [&](const int* nodes, int m) {
        hipLaunchKernelGGL(k_pen_down, dim3(zs_grid(m, J)), tpb, 0, st, V, nodes, m, fc, sc, d_w, d_t, r);
    });
    if (k) {
        hipLaunchKernelGGL(k_pen_tie_coef, dim3(zs_grid(1, J)), tpb, 0, st, k, d_ta, d_tb, fc, sc, d_Winv, r, coef);
        hipLaunchKernelGGL(k_pen_tie_fix, dim3(zs_grid(n, J)), tpb, 0, st, k, n, fc, sc, tie_cols(fc), coef, r);
    }
}

}  // namespace

extern "C" int hpf_penetration(int device, const hpf_zscan_net* net, int F, const double* h, const double* y_extra, int S, int n_inj,
                               const int32_t* inj, const double* I, int chunk_f, int chunk_s, double* V, double* rss, double* vmax, int32_t* varg,
                               double* vsum, double* vsumsq, double* rss_max, int32_t* rss_arg, double* rss_sum, double* rss_sumsq) {
    if (!zscan_args_ok(net, F, h, y_extra, 0, nullptr, 0, nullptr) || !pen_args_ok(net->n, F, S, n_inj, inj, I, chunk_f, chunk_s)) return HPF_E_ARG;
    ZsFactor Y;
    int r = Y.plan(net, F, h);
    if (r != HPF_OK) return r;
    const int n = net->n, k = Y.T.k;
    const bool want_rss = rss || rss_max || rss_arg || rss_sum || rss_sumsq;
    const size_t stage_rows = pen_stage_rows(n, n_inj, V != nullptr);
    int Fc, Sc;
    pen_chunks(F, S, chunk_f, chunk_s, pen_per_f(n, k, y_extra != nullptr), pen_per_j(n, k, n_inj, V != nullptr), Fc, Sc);
    if ((long long)n * Fc * Sc > PEN_MAX_NJ) return HPF_E_ARG;   // (forced lengths only: the automatic ones stay inside the budget)

    if (hipSetDevice(device) != hipSuccess) return HPF_E_HIP;
    int detail = 0;
    int *d_inj = nullptr, *d_varg = nullptr, *d_rarg = nullptr, *d_bad = nullptr;
    double *d_vsum = nullptr, *d_vsumsq = nullptr, *d_sq = nullptr, *d_rsum = nullptr, *d_rsumsq = nullptr;
    unsigned long long *d_vkey = nullptr, *d_rkey = nullptr;
    cplx *d_yst = nullptr, *d_r = nullptr, *d_stage = nullptr, *d_coef = nullptr;
    DevMem ws(&detail);                                  // per-call workspace (declared after the pointers it nulls): gone on every return path
    const size_t nF = (size_t)n * Fc, Jmax = (size_t)Fc * Sc, Fn = (size_t)F * n;
    const std::vector<int> injv(inj, inj + n_inj);
    if ((r = Y.upload(ws, Fc, y_extra != nullptr, false)) || (r = ws.upload(&d_inj, injv)) || (r = ws.alloc(&d_r, n * Jmax)) ||
        (r = ws.alloc(&d_stage, stage_rows * Jmax)) || (r = ws.alloc(&d_vkey, Fn)) || (r = ws.alloc(&d_varg, Fn)) || (r = ws.alloc(&d_vsum, Fn)) ||
        (r = ws.alloc(&d_vsumsq, Fn)) || (r = ws.alloc(&d_bad, (size_t)1)))
        return zs_done(ws, r);
    if (y_extra && (r = ws.alloc(&d_yst, nF))) return zs_done(ws, r);
    if (want_rss && ((r = ws.alloc(&d_sq, (size_t)n * S)) || (r = ws.alloc(&d_rkey, (size_t)n)) || (r = ws.alloc(&d_rarg, (size_t)n)) ||
                     (r = ws.alloc(&d_rsum, (size_t)n)) || (r = ws.alloc(&d_rsumsq, (size_t)n))))
        return zs_done(ws, r);
    if (k && (r = ws.alloc(&d_coef, (size_t)k * Jmax))) return zs_done(ws, r);

    const hipStream_t st = nullptr;
    if (hipMemsetAsync(d_bad, 0, sizeof(int), st) != hipSuccess) return zs_done(ws, HPF_E_HIP);
    for (int f0 = 0; f0 < F; f0 += Fc) {
        const int fc = std::min(Fc, F - f0);             // (the arrays of a short last chunk are [bus][fc])
        if ((r = Y.factor(st, f0, fc, y_extra, d_yst))) return zs_done(ws, r);
        for (int s0 = 0; s0 < S; s0 += Sc) {
            const int sc = std::min(Sc, S - s0);
            const int J = fc * sc;
            // I [s0 ..][f0 ..][:] -> stage [sc][fc][n_inj] -> r
            if (hipMemcpy2D(d_stage, sizeof(cplx) * (size_t)fc * n_inj, I + (size_t)2 * ((size_t)s0 * F + f0) * n_inj, sizeof(cplx) * (size_t)F * n_inj,
                            sizeof(cplx) * (size_t)fc * n_inj, (size_t)sc, hipMemcpyHostToDevice) != hipSuccess)
                return zs_done(ws, HPF_E_HIP);
            if (n_inj < n && hipMemsetAsync(d_r, 0, sizeof(cplx) * (size_t)n * J, st) != hipSuccess) return zs_done(ws, HPF_E_HIP);
            hipLaunchKernelGGL(k_pen_scatter, dim3((unsigned)fc * zs_tiles(sc, n_inj)), dim3(ZS_TILE * 8), 0, st, d_stage, d_inj, n_inj, fc, sc, d_r);
            Y.solve(st, fc, sc, d_r, d_coef);
            const long long rows = (long long)n * fc;
            hipLaunchKernelGGL(k_pen_fold<false>, dim3((unsigned)((rows + 63) / 64)), dim3(64), 0, st, rows, sc, s0, n, fc, f0, d_r, (double*)nullptr,
                               d_vkey, d_varg, d_vsum, d_vsumsq, d_bad);
            if (want_rss) hipLaunchKernelGGL(k_pen_fold_sq, dim3(zs_grid(n, sc)), dim3(ZS_TPB), 0, st, n, fc, sc, f0, s0, S, d_r, d_sq);
            if (V) {
                hipLaunchKernelGGL(k_pen_copy_out, dim3((unsigned)fc * zs_tiles(n, sc)), dim3(ZS_TILE * 8), 0, st, d_r, n, fc, sc, d_stage);
                if (hipMemcpy2D(V + (size_t)2 * ((size_t)s0 * F + f0) * n, sizeof(cplx) * (size_t)F * n, d_stage, sizeof(cplx) * (size_t)fc * n,
                                sizeof(cplx) * (size_t)fc * n, (size_t)sc, hipMemcpyDeviceToHost) != hipSuccess)
                    return zs_done(ws, HPF_E_HIP);
            }
            if (hipGetLastError() != hipSuccess) return zs_done(ws, HPF_E_HIP);
        }
    }
    if (want_rss)
        hipLaunchKernelGGL(k_pen_fold<true>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, (long long)n, S, 0, n, 1, 0, (const cplx*)nullptr, d_sq,
                           d_rkey, d_rarg, d_rsum, d_rsumsq, d_bad);
    auto fetch = [&](void* dst, const void* src, size_t bytes) { return !dst || hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) == hipSuccess; };
    auto fetch_max = [&](double* dst, const unsigned long long* src, size_t count) {
        if (!dst) return true;
        std::vector<unsigned long long> key(count);
        if (hipMemcpy(key.data(), src, sizeof(unsigned long long) * count, hipMemcpyDeviceToHost) != hipSuccess) return false;
        for (size_t q = 0; q < count; ++q) dst[q] = wave_key_value(key[q]);
        return true;
    };
    int bad = 0;
    if (hipMemcpy(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess || !fetch_max(vmax, d_vkey, Fn) ||
        !fetch(varg, d_varg, sizeof(int) * Fn) || !fetch(vsum, d_vsum, sizeof(double) * Fn) || !fetch(vsumsq, d_vsumsq, sizeof(double) * Fn))
        return zs_done(ws, HPF_E_HIP);
    if (want_rss) {
        if (!fetch_max(rss_max, d_rkey, (size_t)n) || !fetch(rss_arg, d_rarg, sizeof(int) * n) || !fetch(rss_sum, d_rsum, sizeof(double) * n) ||
            !fetch(rss_sumsq, d_rsumsq, sizeof(double) * n))
            return zs_done(ws, HPF_E_HIP);
        if (rss) {                                       // [n][S] on the device (the scenario fastest) -> the caller's [S][n]
            std::vector<double> a((size_t)n * S);
            if (hipMemcpy(a.data(), d_sq, sizeof(double) * a.size(), hipMemcpyDeviceToHost) != hipSuccess) return zs_done(ws, HPF_E_HIP);
            for (int i = 0; i < n; ++i)
                for (int s = 0; s < S; ++s) rss[(size_t)s * n + i] = a[(size_t)i * S + s];
        }
    }
    return zs_done(ws, bad ? HPF_E_SINGULAR : HPF_OK);
}

// ---- hpf_resonance_modes -----------------------------------------------------------------------------------------------------------------------
// The critical mode of Y(h) per frequency point by inverse iteration (hpf_resonance.hpp has the arithmetic; include/hpf.h the contract).  The factor
// of a chunk is ZsFactor::factor, y = Y^-1 x is ZsFactor::solve with sc = 1 (r = y [n][fc], in place); the kernels below are the
// loop around them.  x, y and pf are [bus][fc], the partial keys and sums [tile][fc], the per-point values [fc]: a wavefront reads 64 consecutive
// values everywhere.  No atomics: every reduction over the buses is a partial per tile of RMA_TILE buses and then one thread per point over the tiles.
namespace {

// x = y = the start vector
__global__ __launch_bounds__(ZS_TPB) void k_rma_start(int n, int fc, cplx* __restrict__ x, cplx* __restrict__ y) {
    int i, f;
    if (!zs_item(n, fc, i, f)) return;
    const size_t o = (size_t)i * fc + f;
    x[o] = y[o] = rma_start(i, n);
}

// the pivot of every point.  STAGE 0: the partial key of (tile, point) -> pkey, parg [tiles][fc]; STAGE 1: over the tiles -> piv [fc], yp [fc] = y_p
template <int STAGE>
__global__ __launch_bounds__(ZS_TPB) void k_rma_pivot(int n, int fc, const cplx* __restrict__ y, unsigned long long* __restrict__ pkey,
                                                      int* __restrict__ parg, int* __restrict__ piv, cplx* __restrict__ yp) {
    int T, f;
    if (!zs_item(STAGE == 0 ? rma_tiles(n) : 1, fc, T, f)) return;
    uint64_t key;
    int arg;
    if (STAGE == 0) {
        rma_tile_peak(y, n, (size_t)fc, (size_t)f, T, key, arg);
        pkey[(size_t)T * fc + f] = key;
        parg[(size_t)T * fc + f] = arg;
    } else {
        rma_peak_fold((const uint64_t*)pkey, parg, rma_tiles(n), (size_t)fc, (size_t)f, key, arg);
        piv[f] = arg;
        yp[f] = y[(size_t)arg * fc + f];
    }
}

// x = y = y / y_p (yp [fc] is the pivot kernel's copy: y_p itself is overwritten here)
__global__ __launch_bounds__(ZS_TPB) void k_rma_scale(int n, int fc, const cplx* __restrict__ yp, cplx* __restrict__ x, cplx* __restrict__ y) {
    int i, f;
    if (!zs_item(n, fc, i, f)) return;
    const size_t o = (size_t)i * fc + f;
    x[o] = y[o] = rma_scale(y[o], yp[f]);
}

// the three bilinear sums.  STAGE 0: the tile sums -> part [3][tiles][fc]; STAGE 1: the ordered fold over the tiles -> sums [3][fc]
template <int STAGE>
__global__ __launch_bounds__(ZS_TPB) void k_rma_sums(int n, int fc, const cplx* __restrict__ x, const cplx* __restrict__ y, cplx* __restrict__ part,
                                                     cplx* __restrict__ sums) {
    int T, f;
    const int tiles = rma_tiles(n);
    if (!zs_item(STAGE == 0 ? tiles : 1, fc, T, f)) return;
    const size_t q = (size_t)tiles * fc;
    if (STAGE == 0) {
        cplx a, b, g;
        rma_tile_sums(x, y, n, (size_t)fc, (size_t)f, T, a, b, g);
        part[(size_t)T * fc + f] = a;
        part[q + (size_t)T * fc + f] = b;
        part[2 * q + (size_t)T * fc + f] = g;
    } else {
        for (int s = 0; s < 3; ++s) sums[(size_t)s * fc + f] = rma_sum_fold(part + s * q, tiles, (size_t)fc, (size_t)f);
    }
}

// the eigenpair, the participation factors and the residual.
//   STAGE 0 (one thread per point): lambda, zm and 1 / g from the sums -> lam, zr [fc] (.re = zm), ginv [fc]
//   STAGE 1 (per tile and point):   pf_i of the tile's buses -> pf [n][fc] (when wanted), the partial key of the largest defect -> pkey, parg;
//                                   *bad = 1 for a non-finite pf
//   STAGE 2 (per point):            res from the largest defect -> zr (.im = res); *bad = 1 for a non-finite lambda, zm or res
template <int STAGE>
__global__ __launch_bounds__(ZS_TPB) void k_rma_finish(int n, int fc, const cplx* __restrict__ x, const cplx* __restrict__ y,
                                                       const cplx* __restrict__ sums, const cplx* __restrict__ yp, cplx* __restrict__ lam,
                                                       cplx* __restrict__ zr, cplx* __restrict__ ginv, cplx* __restrict__ pf,
                                                       unsigned long long* __restrict__ pkey, int* __restrict__ parg, int* __restrict__ bad) {
    int T, f;
    const int tiles = rma_tiles(n);
    if (!zs_item(STAGE == 1 ? tiles : 1, fc, T, f)) return;
    if (STAGE == 0) {
        cplx l, gi;
        double zm;
        rma_eig(sums[f], sums[(size_t)fc + f], sums[(size_t)2 * fc + f], l, zm, gi);
        lam[f] = l;
        ginv[f] = gi;
        zr[f] = {zm, 0.0};
    } else if (STAGE == 1) {
        const cplx l = lam[f], gi = ginv[f];
        uint64_t key = 0;
        int arg = RMA_NO_BUS, nonfinite = 0;
        const int i1 = (T + 1) * RMA_TILE < n ? (T + 1) * RMA_TILE : n;
        for (int i = T * RMA_TILE; i < i1; ++i) {
            const size_t o = (size_t)i * fc + f;
            const cplx yi = y[o], p = rma_pf(yi, gi);
            nonfinite |= !zscan_finite(p);
            if (pf) pf[o] = p;
            wave_peak_combine(key, arg, wave_key(rma_defect(x[o], l, yi)), i);
        }
        pkey[(size_t)T * fc + f] = key;
        parg[(size_t)T * fc + f] = arg;
        if (nonfinite) *bad = 1;                         // (every writer stores the same value)
    } else {
        uint64_t key;
        int arg;
        rma_peak_fold((const uint64_t*)pkey, parg, tiles, (size_t)fc, (size_t)f, key, arg);
        const cplx l = lam[f];
        const double zm = zr[f].re, res = rma_res(key, l, yp[f]);
        zr[f].im = res;
        if (!zscan_finite(l) || !rma_finite(zm) || !rma_finite(res)) *bad = 1;
    }
}

}  // namespace

extern "C" int hpf_resonance_modes(int device, const hpf_zscan_net* net, int F, const double* h, const double* y_extra, int iters, int chunk,
                                   double* lam, double* zm, double* res, int32_t* top, double* pf) {
    if (!zscan_args_ok(net, F, h, y_extra, 0, nullptr, chunk, nullptr) || iters < 1 || iters > RMA_MAX_ITERS) return HPF_E_ARG;
    ZsFactor Y;
    int r = Y.plan(net, F, h);
    if (r != HPF_OK) return r;
    const int n = net->n, k = Y.T.k, tiles = rma_tiles(n);
    int Fc = zscan_chunk(F, chunk, rma_per_f(n, k, y_extra != nullptr, pf != nullptr));
    if (!zs_clip_chunk(n, chunk, Fc)) return HPF_E_ARG;

    if (hipSetDevice(device) != hipSuccess) return HPF_E_HIP;
    int detail = 0;
    int *d_parg = nullptr, *d_piv = nullptr, *d_bad = nullptr;
    unsigned long long* d_pkey = nullptr;
    cplx *d_coef = nullptr, *d_stage = nullptr, *d_x = nullptr, *d_y = nullptr, *d_pf = nullptr, *d_part = nullptr, *d_sums = nullptr;
    cplx *d_yp = nullptr, *d_lam = nullptr, *d_zr = nullptr, *d_ginv = nullptr;
    DevMem ws(&detail);                                  // per-call workspace (declared after the pointers it nulls): gone on every return path
    const size_t nF = (size_t)n * Fc, tF = (size_t)tiles * Fc;
    if ((r = Y.upload(ws, Fc, y_extra != nullptr, false)) || (r = ws.alloc(&d_x, nF)) || (r = ws.alloc(&d_y, nF)) || (r = ws.alloc(&d_pkey, tF)) ||
        (r = ws.alloc(&d_parg, tF)) || (r = ws.alloc(&d_part, 3 * tF)) || (r = ws.alloc(&d_sums, (size_t)3 * Fc)) ||
        (r = ws.alloc(&d_piv, (size_t)Fc)) || (r = ws.alloc(&d_yp, (size_t)Fc)) || (r = ws.alloc(&d_lam, (size_t)Fc)) ||
        (r = ws.alloc(&d_zr, (size_t)Fc)) || (r = ws.alloc(&d_ginv, (size_t)Fc)) || (r = ws.alloc(&d_bad, (size_t)1)))
        return zs_done(ws, r);
    if (pf && (r = ws.alloc(&d_pf, nF))) return zs_done(ws, r);
    if ((y_extra || pf) && (r = ws.alloc(&d_stage, nF))) return zs_done(ws, r);
    if (k && (r = ws.alloc(&d_coef, (size_t)k * Fc))) return zs_done(ws, r);

    const hipStream_t st = nullptr;
    std::vector<cplx> hl((size_t)Fc), hz((size_t)Fc);
    if (hipMemsetAsync(d_bad, 0, sizeof(int), st) != hipSuccess) return zs_done(ws, HPF_E_HIP);
    for (int f0 = 0; f0 < F; f0 += Fc) {
        const int fc = std::min(Fc, F - f0);             // (the arrays of a short last chunk are [bus][fc])
        const dim3 g_n(zs_grid(n, fc)), g_t(zs_grid(tiles, fc)), g_1(zs_grid(1, fc)), tpb(ZS_TPB);
        if ((r = Y.factor(st, f0, fc, y_extra, d_stage))) return zs_done(ws, r);
        // inverse iteration: y = Y^-1 x with one scenario (in place), the pivot, the scaling
        hipLaunchKernelGGL(k_rma_start, g_n, tpb, 0, st, n, fc, d_x, d_y);
        for (int it = 1; it <= iters; ++it) {
            Y.solve(st, fc, 1, d_y, d_coef);
            hipLaunchKernelGGL(k_rma_pivot<0>, g_t, tpb, 0, st, n, fc, d_y, d_pkey, d_parg, d_piv, d_yp);
            hipLaunchKernelGGL(k_rma_pivot<1>, g_1, tpb, 0, st, n, fc, d_y, d_pkey, d_parg, d_piv, d_yp);
            if (it < iters) hipLaunchKernelGGL(k_rma_scale, g_n, tpb, 0, st, n, fc, d_yp, d_x, d_y);
        }
        hipLaunchKernelGGL(k_rma_sums<0>, g_t, tpb, 0, st, n, fc, d_x, d_y, d_part, d_sums);
        hipLaunchKernelGGL(k_rma_sums<1>, g_1, tpb, 0, st, n, fc, d_x, d_y, d_part, d_sums);
        hipLaunchKernelGGL(k_rma_finish<0>, g_1, tpb, 0, st, n, fc, d_x, d_y, d_sums, d_yp, d_lam, d_zr, d_ginv, d_pf, d_pkey, d_parg, d_bad);
        hipLaunchKernelGGL(k_rma_finish<1>, g_t, tpb, 0, st, n, fc, d_x, d_y, d_sums, d_yp, d_lam, d_zr, d_ginv, d_pf, d_pkey, d_parg, d_bad);
        hipLaunchKernelGGL(k_rma_finish<2>, g_1, tpb, 0, st, n, fc, d_x, d_y, d_sums, d_yp, d_lam, d_zr, d_ginv, d_pf, d_pkey, d_parg, d_bad);
        if (pf) {
            zs_transpose(st, d_pf, n, fc, d_stage);
            if (hipMemcpy(pf + (size_t)2 * f0 * n, d_stage, sizeof(cplx) * (size_t)fc * n, hipMemcpyDeviceToHost) != hipSuccess) return zs_done(ws, HPF_E_HIP);
        }
        if (hipMemcpy(hl.data(), d_lam, sizeof(cplx) * fc, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(hz.data(), d_zr, sizeof(cplx) * fc, hipMemcpyDeviceToHost) != hipSuccess ||
            (top && hipMemcpy(top + f0, d_piv, sizeof(int) * fc, hipMemcpyDeviceToHost) != hipSuccess))
            return zs_done(ws, HPF_E_HIP);
        for (int f = 0; f < fc; ++f) {
            if (lam) lam[2 * (size_t)(f0 + f)] = hl[f].re, lam[2 * (size_t)(f0 + f) + 1] = hl[f].im;
            if (zm) zm[f0 + f] = hz[f].re;
            if (res) res[f0 + f] = hz[f].im;
        }
        if (hipGetLastError() != hipSuccess) return zs_done(ws, HPF_E_HIP);
    }
    int bad = 0;
    if (hipMemcpy(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return zs_done(ws, HPF_E_HIP);
    return zs_done(ws, bad ? HPF_E_SINGULAR : HPF_OK);
}
