// State update of the harmonic Newton loop (k_update / k_update_rect, hpf_lib.hip): the per-entry arithmetic that applies one Newton step
// dx = (dtheta, dV) to the state (Vm, Va) of entry (bus i, harmonic position q), stacked index k = q*n + i.  The kernels run these functions one
// thread per entry; the host emulation (tests/cpu_emul/update_emul.cpp) runs the same functions serially.
//   polar (the reference, HG:478,484-485):  va' = va - dtheta (k >= 1),  vm' = vm - dV (k >= c).
//   rectangular (option "rectangular_update"): the polar step IS, through the tangent map, the rectangular Newton step
//     dU = E (dV + j vm dtheta), E = e^(j va); entries whose magnitude is a state variable (k >= c) take it where it is exact,
//     U' = U - dU, vm' = |U'|, va' = arg U'; the others (slack, PV fundamentals) keep the polar update.
// Every product and sum is rounded on its own: compiled with -ffp-contract=off like the rest of the library.
#pragma once
#include <math.h>
#include <stdint.h>

#include "hpf_assembly.hpp"

#if defined(__HIPCC__)
#define HPF_UPD_HD __host__ __device__ __forceinline__
#else
#define HPF_UPD_HD inline
#endif

namespace hpf {

// the reference's update: dtheta exists for k >= 1, dV for k >= c (whatever the arguments hold below those bounds is not read into the state)
HPF_UPD_HD void update_polar(double& vm, double& va, int k, int c, double dth, double dv) {
    if (k >= 1) va = va - dth;
    if (k >= c) vm = vm - dv;
}

// U' = U - E (dV + j vm dtheta) from the entry's state and the U, E formed from it (polar<false>); vm may be negative: E = U / vm carries the
// sign, and the tangent formula holds for signed states
HPF_UPD_HD cplx update_rect_target(double vm, cplx u, cplx e, double dth, double dv) {
    const double b = vm * dth;
    const cplx dU = {e.re * dv - e.im * b, e.re * b + e.im * dv};
    return {u.re - dU.re, u.im - dU.im};
}

// (vm', va') of a target U': never a negative magnitude; U' = 0 (either sign of zero) -> vm' = 0, va' = 0
HPF_UPD_HD void update_rect_state(cplx t, double& vm, double& va) {
    vm = sqrt(t.re * t.re + t.im * t.im);
    va = vm == 0.0 ? 0.0 : atan2(t.im, t.re);
}

// the rectangular update of one entry: k < c polar, else through U'
HPF_UPD_HD void update_rect(double& vm, double& va, cplx u, cplx e, int k, int c, double dth, double dv) {
    if (k < c) {
        update_polar(vm, va, k, c, dth, dv);
        return;
    }
    update_rect_state(update_rect_target(vm, u, e, dth, dv), vm, va);
}

// U, E of the updated entry: polar<false>(vm', va') as after every update and hpf_set_state (U, E stay a function of (Vm, Va) bit for bit) --
// except at vm' = 0, where E = U / vm does not exist: E = e^(j va') = 1, its limit, keeps the next Jacobian finite
HPF_UPD_HD void update_rect_polar(double vm, double va, cplx& U, cplx& E) {
    if (vm == 0.0) {
        U = {0.0, 0.0};
        E = {1.0, 0.0};
        return;
    }
    polar<false>(vm, va, U, E);
}

}  // namespace hpf
