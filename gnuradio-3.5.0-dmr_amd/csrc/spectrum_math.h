// spectrum_math.h -- the two element-wise formulas of the spectrum-estimate blocks (internal, device code), shared by
// spectrum.hip and the power / dB store path of the register FFT kernels so that both have one definition.
//
// Written with the round-to-nearest intrinsics: nothing here can be contracted to an FMA whatever the flags.
#pragma once
#include <hip/hip_runtime.h>

namespace grhip {

// re * re + im * im: two rounded products, one rounded add (general/gr_complex_to_xxx.cc:198)
__device__ __forceinline__ float mag_squared_val(float re, float im)
{
    return __fadd_rn(__fmul_rn(re, re), __fmul_rn(im, im));
}

// |z| as (float)sqrt((double)re * re + (double)im * im): two rounded double products, one rounded add, a correctly
// rounded double square root and one narrowing (general/gr_complex_to_xxx.cc, the std::abs loop; include/grhip.h says
// what ties this form to hypotf).  The sum of two float squares cannot overflow a double.  As hypotf: an infinite part
// gives +inf whatever the other part is
__device__ __forceinline__ float mag_val(float re, float im)
{
    const double r = (double)re, i = (double)im;
    const float m = __double2float_rn(__dsqrt_rn(__dadd_rn(__dmul_rn(r, r), __dmul_rn(i, i))));
    return (isinf(re) || isinf(im)) ? __builtin_inff() : m;
}

// n * log10f(max(x, 1e-18f)) + k (general/gr_nlog10_ff.cc:60-61)
__device__ __forceinline__ float nlog10_val(float x, float n, float k)
{
    const float m = x < 1e-18f ? 1e-18f : x;            // std::max(in, 1e-18f): a NaN input stays NaN
    return __fadd_rn(__fmul_rn(n, log10f(m)), k);
}

}  // namespace grhip
