// carrier.hip -- the carrier loops built on gri_control_loop (general/gri_control_loop.cc:56-80): gr_pll_freqdet_cf,
// gr_pll_refout_cc, gr_pll_carriertracking_cc (general/gr_pll_*.cc) and digital_costas_loop_cc
// (gr-digital/lib/digital_costas_loop_cc.cc).
//
// Every block is a serial recurrence over the samples: error from the sample and the phase, advance_loop, phase_wrap,
// frequency_limit.  One wavefront per stream, the form of agc_walk_kernel (agc.hip): a window of CARRIER_WIN samples
// goes coalesced into LDS with the next window's loads in flight, every lane walks the recurrence out of LDS (all lanes
// read the same address: a broadcast), lane l keeps the state in front of sample l of each group of 64 and forms that
// sample's outputs itself, so the stores are coalesced.  Every float operation is rounded once in the reference's order
// and types.
//
// pll_walk_kernel<KIND>: the state depends on a sample only through gr_fast_atan2f(im, re), so the lanes turn their
//           samples into that angle on the way into LDS and the walk reads one float per sample.  Sine and cosine of
//           the phase are output only: each lane forms its own.  carriertracking's lock signal is a second serial pass
//           per group over c_n = re cos + im sin, which the lanes form in parallel.
// costas_walk_kernel<ORDER, FREQ_OUT, FASTNCO>: the NCO is inside the loop (out = in * expj(-phase), the detector works
//           on out), so sine and cosine sit on the serial chain: the float-rounded double ones (FASTNCO = false), or a
//           float polynomial after a quadrant reduction that stays off the double pipe.
//
// Termination (every bit pattern of the samples; the host refuses the parameters this rests on, control_loop.h): the
// only loops whose trip count depends on data are phase_wrap's.  alpha and beta are finite, within [0, 1] and [0, 4];
// max_freq and min_freq are finite and at most 1024 in magnitude; the stored phase is within [-2 pi, 2 pi] or NaN and
// the stored frequency is max_freq, min_freq, a value between them, or NaN.  The error is NaN or bounded: for the PLLs
// the angle is NaN or within [-pi, pi] (q + s * base with base <= 1.6), so mod_2pi's result is within 2 pi + 1e-6; for
// Costas gr_branchless_clip gives NaN or a value in [-1, 1] (an infinite sum gives inf - inf).  So after advance_loop
// the phase is NaN, which fails both comparisons, or below 2 pi + 1024 + 4 * 7 + 7 in magnitude: at most 170 trips.
// No index depends on a sample except the arctangent table's, which fast_atan2f clamps to 0 .. 255.
#include <cmath>

#include "carrier.h"
#include "control_loop.h"
#include "device_math.h"
#include "loop_math.h"

namespace grhip {

namespace {

// gr_pll_freqdet_cf.cc:50-59 (and its two siblings): in -+ M_TWOPI in double, narrowed
__device__ __forceinline__ float mod_2pi(float in)
{
    if (in >= PI_UP) return __double2float_rn(__dsub_rn((double)in, CL_TWOPI));
    if (in <= -PI_UP) return __double2float_rn(__dadd_rn((double)in, CL_TWOPI));
    return in;
}

// ---- the three PLLs ----------------------------------------------------------------------------------------------
template <int KIND>
__global__ void __launch_bounds__(64)
pll_walk_kernel(const float2 *__restrict__ in, void *__restrict__ out, long long n, CarrierState *__restrict__ state,
                CarrierParams p, const float *__restrict__ atan_tab)
{
    constexpr bool CT = KIND == PLL_CARRIERTRACKING;
    __shared__ float s_t[CARRIER_WIN];                          // gr_fast_atan2f(im, re) of the window's samples
    __shared__ float2 s_x[CT ? CARRIER_WIN : 1];                // the samples themselves (carriertracking mixes them)
    __shared__ float s_c[CT ? 64 : 1];                          // a group's re cos + im sin
    __shared__ float s_tab[260];
    const int s = blockIdx.x, lane = threadIdx.x;
    const float2 *__restrict__ x = in + (long long)s * n;
    for (int t = lane; t < 257; t += 64) s_tab[t] = atan_tab[t];
    float phase = state[s].phase, freq = state[s].freq, lock = state[s].locksig;
    const double lock_keep = __dsub_rn(1.0, (double)p.alpha);   // gr_pll_carriertracking_cc.cc:113 `(1.0 - d_alpha)`
    float2 v[CARRIER_WIN / 64];
#pragma unroll
    for (int q = 0; q < CARRIER_WIN / 64; ++q) {
        const long long i = lane + 64 * q;
        v[q] = i < n ? x[i] : make_float2(0.f, 0.f);
    }
    __syncthreads();
    for (long long base = 0; base < n; base += CARRIER_WIN) {
        const int m = (int)(n - base < CARRIER_WIN ? n - base : CARRIER_WIN);
#pragma unroll
        for (int q = 0; q < CARRIER_WIN / 64; ++q) {
            s_t[lane + 64 * q] = fast_atan2f<true>(v[q].y, v[q].x, (const float *)s_tab);      // gr_pll_freqdet_cf.cc:65
            if (CT) s_x[lane + 64 * q] = v[q];
        }
        __syncthreads();
        // the next window's loads, in flight while this one is walked
#pragma unroll
        for (int q = 0; q < CARRIER_WIN / 64; ++q) {
            const long long i = base + CARRIER_WIN + lane + 64 * q;
            v[q] = i < n ? x[i] : make_float2(0.f, 0.f);
        }
        for (int g0 = 0; g0 < m; g0 += 64) {
            const int cnt = m - g0 < 64 ? m - g0 : 64;
            float kp = phase, kf = freq;                        // the state in front of this lane's sample
            if (cnt == 64) {
#pragma unroll 8
                for (int j = 0; j < 64; ++j) {
                    kp = lane == j ? phase : kp;
                    kf = lane == j ? freq : kf;
                    loop_step(phase, freq, mod_2pi(__fsub_rn(s_t[g0 + j], phase)), p);    // gr_pll_freqdet_cf.cc:66, :85-87
                }
            } else {
                for (int j = 0; j < cnt; ++j) {
                    kp = lane == j ? phase : kp;
                    kf = lane == j ? freq : kf;
                    loop_step(phase, freq, mod_2pi(__fsub_rn(s_t[g0 + j], phase)), p);
                }
            }
            const long long i = (long long)s * n + base + g0 + lane;
            if (KIND == PLL_FREQDET) {
                if (lane < cnt) ((float *)out)[i] = kf;                                   // gr_pll_freqdet_cf.cc:81
            } else {
                float t_imag, t_real;
                sincos_rounded(kp, t_imag, t_real);                                       // gr_pll_refout_cc.cc:83
                if (KIND == PLL_REFOUT) {
                    if (lane < cnt) ((float2 *)out)[i] = make_float2(t_real, t_imag);     // :84
                } else {
                    const float2 xi = s_x[g0 + lane];
                    // gr_pll_carriertracking_cc.cc:105: iptr[i] * gr_complex(t_real, -t_imag)
                    float2 o = make_float2(__fsub_rn(__fmul_rn(xi.x, t_real), __fmul_rn(xi.y, -t_imag)),
                                           __fadd_rn(__fmul_rn(xi.x, -t_imag), __fmul_rn(xi.y, t_real)));
                    s_c[lane] = __fadd_rn(__fmul_rn(xi.x, t_real), __fmul_rn(xi.y, t_imag));      // :114
                    __syncthreads();
                    float kl = lock;                            // the lock signal behind this lane's sample
                    for (int j = 0; j < cnt; ++j) {
                        // :113-114: float * double + float, narrowed
                        lock = __double2float_rn(__dadd_rn(__dmul_rn((double)lock, lock_keep), (double)__fmul_rn(p.alpha, s_c[j])));
                        kl = lane == j ? lock : kl;
                    }
                    __syncthreads();
                    if (p.squelch && !(__builtin_fabsf(kl) > p.lock_threshold)) o = make_float2(0.f, 0.f);    // :116-117
                    if (lane < cnt) ((float2 *)out)[i] = o;
                }
            }
        }
        __syncthreads();
    }
    if (lane == 0) {
        state[s].phase = phase;
        state[s].freq = freq;
        if (CT) state[s].locksig = lock;
    }
}

// ---- Costas ------------------------------------------------------------------------------------------------------
template <int ORDER>
__device__ __forceinline__ float costas_detector(float re, float im)
{
    if (ORDER == 2) return __fmul_rn(re, im);                                             // digital_costas_loop_cc.cc:107
    const double a = re > 0 ? (double)im : -(double)im;         // (sample.real()>0 ? 1.0 : -1.0) * sample.imag()
    const double b = im > 0 ? (double)re : -(double)re;         // (sample.imag()>0 ? 1.0 : -1.0) * sample.real()
    if (ORDER == 4) return __double2float_rn(__dsub_rn(a, b));                            // :100-101
    const double K = (double)(float)(__builtin_sqrt(2.0) - 1);                            // :85
    if (__builtin_fabsf(re) >= __builtin_fabsf(im)) return __double2float_rn(__dsub_rn(a, __dmul_rn(b, K)));      // :86-88
    return __double2float_rn(__dsub_rn(__dmul_rn(a, K), b));                              // :91-92
}

template <int ORDER, bool FREQ_OUT, bool FASTNCO>
__global__ void __launch_bounds__(64)
costas_walk_kernel(const float2 *__restrict__ in, float2 *__restrict__ out, float *__restrict__ freq_out, long long n,
                   CarrierState *__restrict__ state, CarrierParams p)
{
    __shared__ float2 s_x[CARRIER_WIN];
    const int s = blockIdx.x, lane = threadIdx.x;
    const float2 *__restrict__ x = in + (long long)s * n;
    float phase = state[s].phase, freq = state[s].freq;
    float2 v[CARRIER_WIN / 64];
#pragma unroll
    for (int q = 0; q < CARRIER_WIN / 64; ++q) {
        const long long i = lane + 64 * q;
        v[q] = i < n ? x[i] : make_float2(0.f, 0.f);
    }
    for (long long base = 0; base < n; base += CARRIER_WIN) {
        const int m = (int)(n - base < CARRIER_WIN ? n - base : CARRIER_WIN);
#pragma unroll
        for (int q = 0; q < CARRIER_WIN / 64; ++q) s_x[lane + 64 * q] = v[q];
        __syncthreads();
        // the next window's loads, in flight while this one is walked
#pragma unroll
        for (int q = 0; q < CARRIER_WIN / 64; ++q) {
            const long long i = base + CARRIER_WIN + lane + 64 * q;
            v[q] = i < n ? x[i] : make_float2(0.f, 0.f);
        }
        for (int g0 = 0; g0 < m; g0 += 64) {
            const int cnt = m - g0 < 64 ? m - g0 : 64;
            float2 ko = make_float2(0.f, 0.f);                  // this lane's output
            float kf = freq;                                    // the frequency behind this lane's sample
#pragma unroll 2
            for (int j = 0; j < cnt; ++j) {
                const float2 xi = s_x[g0 + j];
                float sn, cs;                                   // gr_expj(-d_phase), :127
                if (FASTNCO) sincos_fast(-phase, sn, cs);
                else sincos_rounded(-phase, sn, cs);
                // :128, the complex product: ac - bd, ad + bc
                const float o_re = __fsub_rn(__fmul_rn(xi.x, cs), __fmul_rn(xi.y, sn));
                const float o_im = __fadd_rn(__fmul_rn(xi.x, sn), __fmul_rn(xi.y, cs));
                const float error = branchless_clip(costas_detector<ORDER>(o_re, o_im), 1.0f);    // :130-131
                loop_step(phase, freq, error, p);                                         // :133-135
                ko.x = lane == j ? o_re : ko.x;
                ko.y = lane == j ? o_im : ko.y;
                kf = lane == j ? freq : kf;                                               // :137
            }
            if (lane < cnt) {
                const long long i = (long long)s * n + base + g0 + lane;
                out[i] = ko;
                if (FREQ_OUT) freq_out[i] = kf;
            }
        }
        __syncthreads();
    }
    if (lane == 0) {
        state[s].phase = phase;
        state[s].freq = freq;
    }
}

template <int KIND>
int pll_go(const CarrierLaunch &a, const float *atan_tab, hipStream_t st)
{
    hipLaunchKernelGGL((pll_walk_kernel<KIND>), dim3(a.nstreams), dim3(64), 0, st, a.in, a.out, (long long)a.n, a.state, a.p,
                       atan_tab);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

template <int ORDER, bool FASTNCO>
int costas_go(const CarrierLaunch &a, hipStream_t st)
{
    if (a.freq_out)
        hipLaunchKernelGGL((costas_walk_kernel<ORDER, true, FASTNCO>), dim3(a.nstreams), dim3(64), 0, st, a.in, (float2 *)a.out,
                           a.freq_out, (long long)a.n, a.state, a.p);
    else
        hipLaunchKernelGGL((costas_walk_kernel<ORDER, false, FASTNCO>), dim3(a.nstreams), dim3(64), 0, st, a.in, (float2 *)a.out,
                           (float *)nullptr, (long long)a.n, a.state, a.p);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

}  // namespace

int pll_launch(int kind, const CarrierLaunch &a, const float *atan_tab, hipStream_t st)
{
    if (a.n <= 0 || a.nstreams <= 0) return GRHIP_OK;
    if (!atan_tab) return fail(GRHIP_EINVAL, "pll: no arctangent table");
    switch (kind) {
    case PLL_FREQDET: return pll_go<PLL_FREQDET>(a, atan_tab, st);
    case PLL_REFOUT: return pll_go<PLL_REFOUT>(a, atan_tab, st);
    case PLL_CARRIERTRACKING: return pll_go<PLL_CARRIERTRACKING>(a, atan_tab, st);
    }
    return fail(GRHIP_EINVAL, "pll: bad kind %d", kind);
}

int costas_launch(int order, bool fast_nco, const CarrierLaunch &a, hipStream_t st)
{
    if (a.n <= 0 || a.nstreams <= 0) return GRHIP_OK;
    switch (order) {
    case 2: return fast_nco ? costas_go<2, true>(a, st) : costas_go<2, false>(a, st);
    case 4: return fast_nco ? costas_go<4, true>(a, st) : costas_go<4, false>(a, st);
    case 8: return fast_nco ? costas_go<8, true>(a, st) : costas_go<8, false>(a, st);
    }
    return fail(GRHIP_EINVAL, "costas: order must be 2, 4 or 8");
}

}  // namespace grhip
