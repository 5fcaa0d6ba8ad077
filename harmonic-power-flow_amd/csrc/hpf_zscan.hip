// hpf_impedance_scan: driving-point and transfer impedances over a grid of harmonic orders (hpf_zscan.hpp has the arithmetic and the planner;
// include/hpf.h the contract).  Every kernel maps a thread to (item, frequency point) with the frequency fastest: block b of a launch over m items
// serves item b / fb, points (b % fb) * ZS_TPB + threadIdx.x, fb = ceil(Fc / ZS_TPB) -- a one-dimensional grid, so that the widest depth of a large
// star still fits; the host keeps n * fb <= 2^30.
#include <algorithm>
#include <utility>

#include "hpf_internal.hpp"
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

}  // namespace

extern "C" int hpf_impedance_scan(int device, const hpf_zscan_net* net, int F, const double* h, const double* y_extra, int n_sel, const int32_t* sel,
                                  int chunk, double* Z, double* Zt, double* zpeak, int32_t* fpeak) {
    if (!zscan_args_ok(net, F, h, y_extra, n_sel, sel, chunk, Zt)) return HPF_E_ARG;
    const int n = net->n, nb = net->nb;
    ZscanPlan P;
    int r = zscan_plan(n, nb, net->from, net->to, P);
    if (r != HPF_OK) return r;
    const int k = (int)P.tie.size(), ncol = n_sel + 2 * k;
    // columns: the selected buses first (they leave as Zt), then col(a_l), col(b_l) of every tie
    std::vector<int> colbus(sel, sel + n_sel), ta(k), tb(k);
    std::vector<double> tR(k), tX(k);
    for (int l = 0; l < k; ++l) {
        ta[l] = net->from[P.tie[l]], tb[l] = net->to[P.tie[l]];
        tR[l] = net->R[P.tie[l]], tX[l] = net->X[P.tie[l]];
        colbus.push_back(ta[l]);
        colbus.push_back(tb[l]);
    }
    std::vector<unsigned char> path((size_t)ncol * n, 0);
    for (int s = 0; s < ncol; ++s) zscan_mark_path(P, colbus[s], path.data() + (size_t)s * n);
    // scratch per frequency point, in complex values: w, t, Zd | y_extra | columns | W^-1 | staging of the transposed copies
    const size_t stage_rows = std::max<size_t>((Z || y_extra) ? n : 0, (size_t)n_sel * n);
    const size_t per_f = (size_t)3 * n + (y_extra ? n : 0) + (size_t)ncol * n + (size_t)k * k + stage_rows;
    int Fc = zscan_chunk(F, chunk, per_f);
    const long long fb_max = (1ll << 30) / n;            // blocks of ZS_TPB points a launch over n buses may have
    if ((Fc + ZS_TPB - 1) / ZS_TPB > fb_max) {
        if (chunk > 0) return HPF_E_ARG;
        Fc = (int)fb_max * ZS_TPB;
    }

    if (hipSetDevice(device) != hipSuccess) return HPF_E_HIP;
    int detail = 0;
    int *d_parent = nullptr, *d_pbranch = nullptr, *d_child_ptr = nullptr, *d_child = nullptr, *d_inc_ptr = nullptr, *d_inc = nullptr;
    int *d_nodes = nullptr, *d_colbus = nullptr, *d_ta = nullptr, *d_tb = nullptr, *d_pf = nullptr, *d_bad = nullptr;
    double *d_R = nullptr, *d_X = nullptr, *d_gsh = nullptr, *d_bsh = nullptr, *d_xsh = nullptr, *d_h = nullptr, *d_tR = nullptr, *d_tX = nullptr;
    unsigned char* d_path = nullptr;
    unsigned long long* d_pkey = nullptr;
    cplx *d_w = nullptr, *d_t = nullptr, *d_Zd = nullptr, *d_yx = nullptr, *d_cols = nullptr, *d_Winv = nullptr, *d_stage = nullptr;
    DevMem ws(&detail);                                  // per-call workspace (declared after the pointers it nulls): gone on every return path
    auto done = [&](int code) {
        hipDeviceSynchronize();
        ws.clear();
        return code;
    };
    const size_t nF = (size_t)n * Fc;
    if ((r = ws.upload(&d_parent, P.parent)) || (r = ws.upload(&d_pbranch, P.pbranch)) || (r = ws.upload(&d_child_ptr, P.child_ptr)) ||
        (r = ws.upload(&d_child, P.child)) || (r = ws.upload(&d_inc_ptr, P.inc_ptr)) || (r = ws.upload(&d_inc, P.inc)) ||
        (r = ws.upload(&d_nodes, P.dep_nodes)) || (r = ws.upload(&d_R, net->R, (size_t)nb)) || (r = ws.upload(&d_X, net->X, (size_t)nb)) ||
        (r = ws.upload(&d_gsh, net->gsh, (size_t)n)) || (r = ws.upload(&d_bsh, net->bsh, (size_t)n)) ||
        (r = ws.upload(&d_xsh, net->xsh, (size_t)n)) || (r = ws.upload(&d_h, h, (size_t)F)) || (r = ws.alloc(&d_pkey, (size_t)n)) ||
        (r = ws.alloc(&d_pf, (size_t)n)) || (r = ws.alloc(&d_bad, (size_t)n)) || (r = ws.alloc(&d_w, nF)) || (r = ws.alloc(&d_t, nF)) ||
        (r = ws.alloc(&d_Zd, nF)))
        return done(r);
    if (y_extra && (r = ws.alloc(&d_yx, nF))) return done(r);
    if (stage_rows && (r = ws.alloc(&d_stage, stage_rows * Fc))) return done(r);
    if (ncol && ((r = ws.upload(&d_colbus, colbus)) || (r = ws.upload(&d_path, path)) || (r = ws.alloc(&d_cols, (size_t)ncol * nF)))) return done(r);
    if (k && ((r = ws.upload(&d_ta, ta)) || (r = ws.upload(&d_tb, tb)) || (r = ws.upload(&d_tR, tR)) || (r = ws.upload(&d_tX, tX)) ||
              (r = ws.alloc(&d_Winv, (size_t)k * k * Fc))))
        return done(r);

    const ZscanView V{n, d_parent, d_pbranch, d_child_ptr, d_child, d_inc_ptr, d_inc, d_R, d_X, d_gsh, d_bsh, d_xsh};
    const hipStream_t st = nullptr;
    auto transpose = [&](const cplx* in, long long R, long long C, cplx* out) {
        const long long tiles = ((R + ZS_TILE - 1) / ZS_TILE) * ((C + ZS_TILE - 1) / ZS_TILE);
        hipLaunchKernelGGL(k_zscan_transpose, dim3((unsigned)tiles), dim3(ZS_TILE * 8), 0, st, in, R, C, out);
    };
    hipLaunchKernelGGL(k_zscan_peaks_init, dim3((n + 255) / 256), dim3(256), 0, st, n, d_pkey, d_pf, d_bad);
    for (int f0 = 0; f0 < F; f0 += Fc) {
        const int fc = std::min(Fc, F - f0);             // (the arrays of a short last chunk are [bus][fc])
        const double* hh = d_h + f0;
        if (y_extra) {
            if (hipMemcpy(d_stage, y_extra + (size_t)2 * f0 * n, sizeof(cplx) * (size_t)fc * n, hipMemcpyHostToDevice) != hipSuccess)
                return done(HPF_E_HIP);
            transpose(d_stage, fc, n, d_yx);
        }
        for (int d = P.n_depths - 1; d >= 0; --d) {
            const int m = P.dep_ptr[d + 1] - P.dep_ptr[d];
            hipLaunchKernelGGL(k_zscan_up, dim3(zs_grid(m, fc)), dim3(ZS_TPB), 0, st, V, d_nodes + P.dep_ptr[d], m, fc, hh, d_yx, d_w, d_t);
        }
        for (int d = 0; d < P.n_depths; ++d) {
            const int m = P.dep_ptr[d + 1] - P.dep_ptr[d];
            hipLaunchKernelGGL(k_zscan_down, dim3(zs_grid(m, fc)), dim3(ZS_TPB), 0, st, V, d_nodes + P.dep_ptr[d], m, fc, d_w, d_t, d_Zd);
        }
        if (ncol) {
            hipLaunchKernelGGL(k_zscan_col_walk, dim3(zs_grid(ncol, fc)), dim3(ZS_TPB), 0, st, V, d_colbus, ncol, fc, d_t, d_Zd, d_cols);
            for (int d = 1; d < P.n_depths; ++d) {
                const int m = P.dep_ptr[d + 1] - P.dep_ptr[d];
                hipLaunchKernelGGL(k_zscan_col_fill, dim3(zs_grid(m, fc), ncol), dim3(ZS_TPB), 0, st, V, d_nodes + P.dep_ptr[d], m, fc, d_path, d_t,
                                   d_cols);
            }
        }
        if (k) {
            const cplx* tc = d_cols + (size_t)n_sel * n * fc;
            hipLaunchKernelGGL(k_zscan_tie_winv, dim3(zs_grid(1, fc)), dim3(ZS_TPB), 0, st, k, d_ta, d_tb, d_tR, d_tX, n, fc, hh, tc, d_Winv);
            hipLaunchKernelGGL(k_zscan_tie_fix, dim3(zs_grid(n, fc), 1), dim3(ZS_TPB), 0, st, k, n, fc, tc, d_Winv, (const int*)nullptr, d_Zd);
            if (n_sel)
                hipLaunchKernelGGL(k_zscan_tie_fix, dim3(zs_grid(n, fc), n_sel), dim3(ZS_TPB), 0, st, k, n, fc, tc, d_Winv, d_colbus, d_cols);
        }
        hipLaunchKernelGGL(k_zscan_peaks, dim3((n + ZS_TPB / 64 - 1) / (ZS_TPB / 64)), dim3(ZS_TPB), 0, st, n, fc, f0, d_Zd, d_pkey, d_pf, d_bad);
        if (Z) {
            transpose(d_Zd, n, fc, d_stage);
            if (hipMemcpy(Z + (size_t)2 * f0 * n, d_stage, sizeof(cplx) * (size_t)fc * n, hipMemcpyDeviceToHost) != hipSuccess) return done(HPF_E_HIP);
        }
        if (n_sel) {
            transpose(d_cols, (long long)n_sel * n, fc, d_stage);
            if (hipMemcpy(Zt + (size_t)2 * f0 * n_sel * n, d_stage, sizeof(cplx) * (size_t)fc * n_sel * n, hipMemcpyDeviceToHost) != hipSuccess)
                return done(HPF_E_HIP);
        }
        if (hipGetLastError() != hipSuccess) return done(HPF_E_HIP);
    }
    std::vector<unsigned long long> pkey((size_t)n);
    std::vector<int> pf((size_t)n), bad((size_t)n);
    if (hipMemcpy(pkey.data(), d_pkey, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(pf.data(), d_pf, sizeof(int) * n, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(bad.data(), d_bad, sizeof(int) * n, hipMemcpyDeviceToHost) != hipSuccess)
        return done(HPF_E_HIP);
    bool singular = false;
    for (int i = 0; i < n; ++i) {
        if (zpeak) zpeak[i] = wave_key_value(pkey[i]);
        if (fpeak) fpeak[i] = pf[i];
        singular |= bad[i] != 0;
    }
    return done(singular ? HPF_E_SINGULAR : HPF_OK);
}
