// TEST INFRASTRUCTURE: executes the functions of csrc/hpf_sources.hpp (what k_source_expand runs per thread) and the harmonic mismatch row with a
// source pointer (csrc/hpf_assembly.hpp: what k_mismatch<false, true> forms) serially on the host, so that `-m "not gpu"` tests can check them
// against the NumPy restatement (sweep.source_currents) and against a per-bus-device model.  It is NOT part of libhpf.so and never on the
// product path.
#include "hpf_sources.hpp"
using namespace hpf;

extern "C" {

// form 1 end to end (the host's libm sin / cos): out[t] = source_expand(a[t], phi[t], order[t], in[t])
void emul_source_expand(int count, const double* a, const double* phi, const int* order, const cplx* in, cplx* out) {
    for (int t = 0; t < count; ++t) out[t] = source_expand(a[t], phi[t], order[t], in[t]);
}

// ... with the caller's (cos, sin) values
void emul_source_from_cs(int count, const double* a, const double* c, const double* s, const cplx* in, cplx* out) {
    for (int t = 0; t < count; ++t) out[t] = source_from_cs(a[t], c[t], s[t], in[t]);
}

// harmonic mismatch (stacked layout of the host model) of one scenario; src: [n - m][Hn] source currents of the nonlinear buses, or NULL
void emul_mismatch_sources(int n, int m, int c, int Hn, int nnz, int n_dev, int coupled, const int* rowptr, const int* col, const int* diag,
                           const double* Y, const int* dev, const double* YN, const double* IN, const double* U, const double* P, const double* Q,
                           const cplx* src, double* f) {
    Model M;
    M.n = n; M.m = m; M.c = c; M.Hn = Hn; M.nnz = nnz; M.n_dev = n_dev; M.coupled = coupled;
    M.rowptr = rowptr; M.col = col; M.diag = diag; M.Y = (const cplx*)Y; M.dev = dev;
    M.YN = (const cplx*)YN; M.IN = (const cplx*)IN;
    const int Nc = n * Hn - 1;
    for (int k = 1; k < n * Hn; ++k) {
        const int q = k / n, i = k - q * n;
        const cplx* sp = (src && i >= m) ? src + (size_t)(i - m) * Hn : nullptr;
        store_mismatch(f, Nc, c, k, mismatch_row_qi<false>(M, (const cplx*)U, P, Q, q, i, nullptr, sp));
    }
}
}
