// fir_arith.h -- device arithmetic shared by the per-lane FIR kernels (csrc/arb_resampler.hip, csrc/frac_interp.hip,
// csrc/resampler.hip) and the input staging of csrc/frac_interp.hip.  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

namespace grhip {

__device__ inline float2 zero_of(float2) { return make_float2(0.f, 0.f); }
__device__ inline float zero_of(float) { return 0.f; }

// acc + h*x unfused, in the reference's operand order (float * gr_complex is (h*re, h*im); the complex product is
// (ac - bd, ad + bc)); the Makefile's -ffp-contract=off keeps the multiply and the add apart
__device__ inline float mac_unfused(float acc, float h, float x) { return acc + h * x; }
__device__ inline float2 mac_unfused(float2 acc, float h, float2 x) { return make_float2(acc.x + h * x.x, acc.y + h * x.y); }
__device__ inline float2 mac_unfused(float2 acc, float2 h, float2 x)
{
    const float ac = h.x * x.x, bd = h.y * x.y, ad = h.x * x.y, bc = h.y * x.x;
    return make_float2(acc.x + (ac - bd), acc.y + (ad + bc));
}
__device__ inline float mac_fma(float acc, float h, float x) { return __builtin_fmaf(h, x, acc); }
__device__ inline float2 mac_fma(float2 acc, float h, float2 x)
{
    return make_float2(__builtin_fmaf(h, x.x, acc.x), __builtin_fmaf(h, x.y, acc.y));
}
__device__ inline float2 mac_fma(float2 acc, float2 h, float2 x)
{
    return make_float2(__builtin_fmaf(h.x, x.x, __builtin_fmaf(-h.y, x.y, acc.x)),
                       __builtin_fmaf(h.x, x.y, __builtin_fmaf(h.y, x.x, acc.y)));
}
__device__ inline float2 add(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ inline float add(float a, float b) { return a + b; }

// Stages the logical items [p0, p0 + span) of `in` into xs[0 .. span) with a workgroup of THREADS lanes, eight loads
// in flight per lane.  Positions outside the n_phys physical items (p < 0: the zeros in front; p >= n_phys) read as 0.
template <class T, int THREADS>
__device__ inline void stage_span(T *xs, const T *in, long long p0, int span, long long n_phys)
{
    for (int ub = threadIdx.x; ub < span; ub += THREADS * 8) {
        T v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int u = ub + THREADS * i;
            const long long p = p0 + u;
            v[i] = zero_of(T());
            if (u < span && p >= 0 && p < n_phys) v[i] = in[p];
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int u = ub + THREADS * i;
            if (u < span) xs[u] = v[i];
        }
    }
}

}  // namespace grhip
