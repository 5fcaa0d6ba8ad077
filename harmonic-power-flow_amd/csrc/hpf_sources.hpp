// Per-scenario Norton source currents (hpf_set_sources / hpf_queue_sources, include/hpf.h "Source currents"): the arithmetic of input form 1.
//
// The harmonic mismatch of a nonlinear bus i is I_net + (I_N - Y_N U) (HG:313-323, 347-354).  Y_N enters the Jacobian and every per-model image of
// the block tree; I_N enters the right-hand side alone.  A scenario with sources replaces I_N[dev(i)][q] by I_src[s][i - m][q] in exactly that
// place (norton_injection / norton_injection_lds, hpf_assembly.hpp / hpf_lib.hip) and nothing else changes.
//
// Form 0 ("currents"): I_src is the caller's, used as given.
// Form 1 ("scale and shift"): per (scenario, nonlinear bus) two doubles (a, phi) -- a units of the device in service, their waveform shifted in
// time by phi (radians at the fundamental), so that harmonic order h rotates by h phi:
//     I_src[q] = (a e^(j h_q phi)) I_N[dev(i)][q],      h_q = the harmonic ORDER of position q (1, 3, 5, ...; passed with the data)
// Rounding, fixed here and the same on the device and in the host emulation (tests/cpu_emul/sources_emul.cpp) -- every product and sum is rounded
// on its own, nothing is contracted (-ffp-contract=off):
//     ang    = (double)h_q * phi
//     (s, c) = sincos(ang)
//     w      = (a * c, a * s)
//     I      = cmul_unf(w, in) = (w.re * in.re - w.im * in.im,  w.re * in.im + w.im * in.re)
// With sin / cos within 1 ulp, each component of I is within 6 * 2^-52 * |a| * |in| of the exact product (two function values, one rounding
// each for a c and a s, two products, one sum).  sources_from_cs takes (c, s) from the caller: what a test needs to compare two implementations
// bit for bit without comparing their sin / cos.
#pragma once
#include "hpf_assembly.hpp"

namespace hpf {

enum { SRC_CURRENTS = 0, SRC_SCALE_SHIFT = 1 };

HPF_HD cplx source_from_cs(double a, double c, double s, cplx in) {
    const cplx w = {a * c, a * s};
    return cmul_unf(w, in);
}

HPF_HD cplx source_expand(double a, double phi, int order, cplx in) {
    const double ang = (double)order * phi;
    double s, c;
#if defined(__HIP_DEVICE_COMPILE__)
    sincos(ang, &s, &c);
#else
    s = sin(ang);
    c = cos(ang);
#endif
    return source_from_cs(a, c, s, in);
}

}  // namespace hpf
