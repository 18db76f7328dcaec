// loop_math.h -- what the walk kernels of carrier.hip and constellation.hip share (internal, device code): the float
// twins of the loop's double constants, gri_control_loop's step, and the two sine/cosine pairs of the NCO.
#pragma once
#include <hip/hip_runtime.h>

#include "carrier.h"
#include "control_loop.h"

namespace grhip {

namespace {

// `in > M_PI` and `d_phase > M_TWOPI` compare a float with a double constant.  float(pi) and float(2 pi) lie above the
// double constants and their predecessors below, so for a float f:  f > pi_d  <=>  f >= float(pi), and likewise for
// 2 pi and for the negated pair.  The conversion to double then happens only where the subtraction runs.
constexpr float PI_UP = (float)CL_PI, TWOPI_UP = (float)CL_TWOPI;
static_assert((double)PI_UP > CL_PI && (double)TWOPI_UP > CL_TWOPI, "the float constants round up");
static_assert(__builtin_bit_cast(unsigned, PI_UP) == 0x40490fdbu && (double)__builtin_bit_cast(float, 0x40490fdau) < CL_PI &&
              __builtin_bit_cast(unsigned, TWOPI_UP) == 0x40c90fdbu && (double)__builtin_bit_cast(float, 0x40c90fdau) < CL_TWOPI,
              "no float between the double constant and its float");

// advance_loop, phase_wrap, frequency_limit (gri_control_loop.cc:56-80)
__device__ __forceinline__ void loop_step(float &phase, float &freq, float error, const CarrierParams &p)
{
    freq = __fadd_rn(freq, __fmul_rn(p.beta, error));                                    // :59
    phase = __fadd_rn(__fadd_rn(phase, freq), __fmul_rn(p.alpha, error));                // :60
    while (phase >= TWOPI_UP) phase = __double2float_rn(__dsub_rn((double)phase, CL_TWOPI));     // :67-68
    while (phase <= -TWOPI_UP) phase = __double2float_rn(__dadd_rn((double)phase, CL_TWOPI));    // :69-70
    if (freq > p.max_freq) freq = p.max_freq;                                            // :76-79
    else if (freq < p.min_freq) freq = p.min_freq;
}

// (float)sin((double)x), (float)cos((double)x)
__device__ __forceinline__ void sincos_rounded(float x, float &s, float &c)
{
    s = __double2float_rn(sin((double)x));
    c = __double2float_rn(cos((double)x));
}

// float sine and cosine for |x| <= 2 pi (the loop's phase), absolute error below 2e-7: k = rint(x 2/pi), r = x - k pi/2
// with pi/2 in two floats and fused steps, then the degree-7 and degree-8 minimax polynomials on [-pi/4, pi/4] and a
// swap by quadrant.  A NaN gives NaNs (k converts to 0).
__device__ __forceinline__ void sincos_fast(float x, float &s, float &c)
{
    const float k = __builtin_rintf(__fmul_rn(x, 0.636619772f));
    float r = __builtin_fmaf(k, -1.57079637f, x);
    r = __builtin_fmaf(k, 4.37113883e-8f, r);
    const float z = __fmul_rn(r, r);
    float ps = __builtin_fmaf(z, -1.9515295891e-4f, 8.3321608736e-3f);
    ps = __builtin_fmaf(z, ps, -1.6666654611e-1f);
    ps = __builtin_fmaf(__fmul_rn(z, r), ps, r);
    float pc = __builtin_fmaf(z, 2.443315711809948e-5f, -1.388731625493765e-3f);
    pc = __builtin_fmaf(z, pc, 4.166664568298827e-2f);
    pc = __builtin_fmaf(__fmul_rn(z, z), pc, __builtin_fmaf(z, -0.5f, 1.0f));
    const int q = (int)k;
    const float a = (q & 1) ? pc : ps, b = (q & 1) ? ps : pc;
    s = (q & 2) ? -a : a;
    c = ((q + 1) & 2) ? -b : b;
}

}  // namespace

}  // namespace grhip
