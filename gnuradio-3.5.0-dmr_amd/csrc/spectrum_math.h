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

// n * log10f(max(x, 1e-18f)) + k (general/gr_nlog10_ff.cc:60-61)
__device__ __forceinline__ float nlog10_val(float x, float n, float k)
{
    const float m = x < 1e-18f ? 1e-18f : x;            // std::max(in, 1e-18f): a NaN input stays NaN
    return __fadd_rn(__fmul_rn(n, log10f(m)), k);
}

}  // namespace grhip
