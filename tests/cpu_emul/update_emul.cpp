// TEST INFRASTRUCTURE: executes the functions of csrc/hpf_update.hpp (what k_update / k_update_rect run per thread) serially on the host, so that
// `-m "not gpu"` tests can check them against the NumPy restatement (tests/update_ref.py).  It is NOT part of libhpf.so and never on the
// product path.
#include "hpf_update.hpp"
using namespace hpf;

extern "C" {

// count entries with stacked indices k, states (vm, va), the U, E the handle would hold for them, steps (dth, dv); rect != 0: update_rect, else
// update_polar.  Out: the new state, the target U' (NaN where the entry takes the polar update) and the U, E the kernel would store.
void emul_update(int count, int c, int rect, const int* k, const double* vm, const double* va, const cplx* u, const cplx* e, const double* dth,
                 const double* dv, double* vm_out, double* va_out, cplx* target, cplx* U_out, cplx* E_out) {
    for (int t = 0; t < count; ++t) {
        double m = vm[t], a = va[t];
        const bool through_u = rect && k[t] >= c;
        target[t] = through_u ? update_rect_target(m, u[t], e[t], dth[t], dv[t]) : cplx{NAN, NAN};
        if (rect)
            update_rect(m, a, u[t], e[t], k[t], c, dth[t], dv[t]);
        else
            update_polar(m, a, k[t], c, dth[t], dv[t]);
        vm_out[t] = m;
        va_out[t] = a;
        if (through_u)
            update_rect_polar(m, a, U_out[t], E_out[t]);
        else
            polar<false>(m, a, U_out[t], E_out[t]);
    }
}
}
