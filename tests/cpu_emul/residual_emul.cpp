// TEST INFRASTRUCTURE: executes the residual row function of csrc/hpf_assembly.hpp (step_residual_row: what k_step_residual runs per
// thread) serially on the host, so that `-m "not gpu"` tests can check it against f - J dx with the J of emul_jacobian_csr.
// It is NOT part of libhpf.so and never on the product path.
#include "hpf_assembly.hpp"
using namespace hpf;

extern "C" {

// U, E [Hn*n] complex in stacked order; the step either stacked (form 0: dx [N]) or as a bus-major image (form 1: dx [n][Bst], entry
// 2p + (theta | V) of bus j).  Outputs in the reference's real row layout (store_mismatch): r, a = |J| |dx|, w = row sums of |J|, f.
void emul_step_residual(int n, int m, int c, int Hn, int nnz, int n_dev, int coupled, const int* rowptr, const int* col, const int* diag,
                        const double* Y, const int* dev, const double* YN, const double* IN, const double* U, const double* E,
                        const double* P, const double* Q, const double* dx, int form, int Bst, double* r, double* a, double* w, double* f) {
    Model M;
    M.n = n; M.m = m; M.c = c; M.Hn = Hn; M.nnz = nnz; M.n_dev = n_dev; M.coupled = coupled;
    M.rowptr = rowptr; M.col = col; M.diag = diag; M.Y = (const cplx*)Y; M.dev = dev;
    M.YN = (const cplx*)YN; M.IN = (const cplx*)IN;
    const int Nc = n * Hn - 1;
    const StepStacked ds{dx, Nc, c};
    const StepBusMajor db{dx, Bst};
    for (int k = 1; k < n * Hn; ++k) {
        const int q = k / n, i = k - q * n;
        const cplx fk = mismatch_row_qi<false>(M, (const cplx*)U, P, Q, q, i);
        const StepRow s = form ? step_residual_row(M, (const cplx*)U, (const cplx*)E, q, i, fk, db)
                               : step_residual_row(M, (const cplx*)U, (const cplx*)E, q, i, fk, ds);
        store_mismatch(r, Nc, c, k, s.r);
        store_mismatch(a, Nc, c, k, s.a);
        store_mismatch(w, Nc, c, k, s.w);
        store_mismatch(f, Nc, c, k, fk);
    }
}
}
