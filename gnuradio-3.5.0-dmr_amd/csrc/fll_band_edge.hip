// fll_band_edge.hip -- digital_fll_band_edge_cc (gr-digital/lib/digital_fll_band_edge_cc.cc:208-259), the last block
// built on gri_control_loop.
//
// What is computed (include/grhip.h states the contract): with fs = filter_size and xz = fs zeros followed by the
// stream, step j derotates d[j] = xz[j] * expj(phase), runs the two fs-tap band-edge filters over d[j-fs+1 .. j], takes
// error = |lower|^2 - |upper|^2 and advances the loop; output item n is d[n-(fs-1)].
//
// One wavefront per stream, the shape of costas_walk_kernel (carrier.hip): a window of FLL_WIN items of xz goes
// coalesced into LDS with the next window's loads in flight; the derotated samples sit in an LDS ring of FLL_RING
// items (the ring also holds the delayed output, so nothing else is kept of it); the taps sit in registers, lane l
// owning taps l, l + 64, ...  Per step: the NCO (uniform over the wave), lane 0 puts d[j] into the ring, every lane
// forms the products of its taps with consecutive ring words, the four sums are reduced across the lanes, and every
// lane takes the loop's step.  Lane l of each group of 64 steps keeps that step's frq, phs and err, reads its delayed
// output from the ring after the group, and the stores are coalesced.
//   GENERIC = true:  sine and cosine are the float-rounded double ones; every product and sum is rounded once as g++
//           forms complex<float> arithmetic without contraction; the lanes put their taps' products into LDS and the
//           two complex sums run serially in the reference's order k = 0 .. fs-1 (every lane runs them: the result is
//           uniform without a broadcast).
//   GENERIC = false: the float polynomial NCO of loop_math.h, fused multiply-adds per lane, and a transposing
//           butterfly: two half-wave swaps halve four quantities to two, one row swap halves two to one, four DPP steps
//           finish the sum within a row of 16 lanes (7 exchanges, none through LDS, where four separate butterflies
//           take 24), and four lane reads broadcast the results.
//
// phase_wrap: the error is a difference of two filter powers and is not bounded, so neither is the phase after
// advance_loop, and the reference's `while (phase > 2 pi) phase -= 2 pi` does not end once the subtraction rounds back
// to phase.  fll_wrap runs that loop for at most FLL_WRAP_TRIPS trips each way (|phase| up to about 1600: for
// max_freq <= 1024 that is every error with (alpha + beta) |error| below about 570, far beyond a signal of any sane
// scale) and beyond that takes the exact double remainder fmod(phase, 2 pi), narrowed, with one conditional step where
// the narrowing rounds up to float(2 pi).  A stated deviation (include/grhip.h).
//
// Termination and bounds, for every bit pattern of the samples and the state: the only loops whose trip count depends
// on data are fll_wrap's two, which count to FLL_WRAP_TRIPS; fmod on doubles ends for every argument (an infinite
// phase gives NaN, which fails every comparison that follows).  The walk's other loops run over n, fs and constants.
// No index depends on a sample: ring indices are masked with FLL_RING - 1, window indices are below FLL_WIN, product
// indices below fs <= FLL_MAX_TAPS, global indices below n (in and the outputs), fs (xh, the taps) and fs - 1 (dh), all
// checked by the host.  A ring slot is overwritten FLL_RING steps after it was written; the oldest slot read is
// fs - 1 + 63 steps old (a group's delayed outputs), which FLL_RING covers.
#include <cmath>

#include "control_loop.h"
#include "fll_band_edge.h"
#include "loop_math.h"

namespace grhip {

namespace {

static_assert((FLL_RING & (FLL_RING - 1)) == 0 && FLL_RING >= FLL_MAX_TAPS - 1 + 64 && FLL_WIN >= FLL_MAX_TAPS, "ring and window hold a filter");

// phase_wrap (gri_control_loop.cc:64-71) with a bounded trip count; the stored phase is NaN or within 2 pi
__device__ __forceinline__ float fll_wrap(float phase)
{
    for (int t = 0; t < FLL_WRAP_TRIPS && phase >= TWOPI_UP; ++t) phase = __double2float_rn(__dsub_rn((double)phase, CL_TWOPI));
    for (int t = 0; t < FLL_WRAP_TRIPS && phase <= -TWOPI_UP; ++t) phase = __double2float_rn(__dadd_rn((double)phase, CL_TWOPI));
    if (phase >= TWOPI_UP || phase <= -TWOPI_UP) {
        phase = __double2float_rn(fmod((double)phase, CL_TWOPI));
        if (phase >= TWOPI_UP) phase = __double2float_rn(__dsub_rn((double)phase, CL_TWOPI));
        else if (phase <= -TWOPI_UP) phase = __double2float_rn(__dadd_rn((double)phase, CL_TWOPI));
    }
    return phase;
}

// advance_loop, phase_wrap, frequency_limit (gri_control_loop.cc:56-80)
__device__ __forceinline__ void fll_step(float &phase, float &freq, float error, const CarrierParams &p)
{
    freq = __fadd_rn(freq, __fmul_rn(p.beta, error));                                    // :59
    phase = fll_wrap(__fadd_rn(__fadd_rn(phase, freq), __fmul_rn(p.alpha, error)));      // :60, :64-71
    if (freq > p.max_freq) freq = p.max_freq;                                            // :76-79
    else if (freq < p.min_freq) freq = p.min_freq;
}

__device__ __forceinline__ float lane_read(float v, int lane)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// v_permlane32_swap: lanes 32 .. 63 of a change places with lanes 0 .. 31 of b
__device__ __forceinline__ void half_swap(float &a, float &b)
{
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    a = __uint_as_float(r[0]);
    b = __uint_as_float(r[1]);
}

// v_permlane16_swap: the odd rows of 16 lanes of a change places with the even rows of b
__device__ __forceinline__ void row_swap(float &a, float &b)
{
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    a = __uint_as_float(r[0]);
    b = __uint_as_float(r[1]);
}

// v from another lane of the same row of 16, on the DPP path (CTRL: a quad_perm or a mirror; every lane has a source)
template <int CTRL>
__device__ __forceinline__ float dpp(float v)
{
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xf, 0xf, false));
}

// the ring slot of d[j]; j from -(fs - 1) on, taken modulo 2^32 (FLL_RING divides it)
__device__ __forceinline__ unsigned slot(unsigned j) { return (j + (unsigned)FLL_MAX_TAPS) & (unsigned)(FLL_RING - 1); }

template <int TPL, bool GENERIC>
__global__ void __launch_bounds__(64)
fll_walk_kernel(FllLaunch a)
{
    __shared__ float2 s_x[FLL_WIN];                             // the window's items of xz
    __shared__ float2 s_d[FLL_RING];                            // the derotated samples
    __shared__ float4 s_p[GENERIC ? FLL_MAX_TAPS : 1];          // a step's products: upper re, im, lower re, im
    const int s = blockIdx.x, lane = threadIdx.x, fs = a.fs;
    const long long n = a.n;
    const float2 *__restrict__ x = a.in + (long long)s * n;
    float2 *__restrict__ xh = a.xh + (long long)s * fs;
    float2 *__restrict__ dh = a.dh + (long long)s * fs;
    const CarrierParams p = a.p;
    float phase = a.state[s].phase, freq = a.state[s].freq;
    float2 tl[TPL], tu[TPL];
#pragma unroll
    for (int t = 0; t < TPL; ++t) {
        const int k = lane + 64 * t;
        tl[t] = k < fs ? a.lower[k] : make_float2(0.f, 0.f);
        tu[t] = k < fs ? a.upper[k] : make_float2(0.f, 0.f);
    }
    for (int q = lane; q < FLL_RING; q += 64) s_d[q] = make_float2(0.f, 0.f);
    __syncthreads();
    for (int k = lane; k < fs - 1; k += 64) s_d[slot((unsigned)(k - (fs - 1)))] = dh[k];        // d[-(fs-1) + k]
    // xz[j]: the last fs inputs of the calls before, then this call's
    float2 v[FLL_WIN / 64];
#pragma unroll
    for (int q = 0; q < FLL_WIN / 64; ++q) {
        const long long j = lane + 64 * q;
        v[q] = j < n ? (j < fs ? xh[j] : x[j - fs]) : make_float2(0.f, 0.f);
    }
    for (long long base = 0; base < n; base += FLL_WIN) {
        const int m = (int)(n - base < FLL_WIN ? n - base : FLL_WIN);
#pragma unroll
        for (int q = 0; q < FLL_WIN / 64; ++q) s_x[lane + 64 * q] = v[q];
        __syncthreads();
        // the next window's loads, in flight while this one is walked
#pragma unroll
        for (int q = 0; q < FLL_WIN / 64; ++q) {
            const long long j = base + FLL_WIN + lane + 64 * q;
            v[q] = j < n ? (j < fs ? xh[j] : x[j - fs]) : make_float2(0.f, 0.f);
        }
        for (int g0 = 0; g0 < m; g0 += 64) {
            const int cnt = m - g0 < 64 ? m - g0 : 64;
            float kf = 0.f, kp = 0.f, ke = 0.f;                 // frq, phs, err behind this lane's step
            for (int jj = 0; jj < cnt; ++jj) {
                const float2 xi = s_x[g0 + jj];
                const unsigned j = (unsigned)(base + g0 + jj);
                float sn, cs;                                   // gr_expj(d_phase), :235
                if (GENERIC) sincos_rounded(phase, sn, cs);
                else sincos_fast(phase, sn, cs);
                // :236, the complex product: ac - bd, ad + bc
                const float2 d = make_float2(__fsub_rn(__fmul_rn(xi.x, cs), __fmul_rn(xi.y, sn)),
                                             __fadd_rn(__fmul_rn(xi.x, sn), __fmul_rn(xi.y, cs)));
                if (lane == 0) s_d[slot(j)] = d;
                __syncthreads();
                const unsigned w0 = j - (unsigned)(fs - 1) + (unsigned)lane;     // tap k works on d[j - fs + 1 + k], :241-244
                float ur, ui, lr, li;
                if (GENERIC) {
#pragma unroll
                    for (int t = 0; t < TPL; ++t) {
                        const int k = lane + 64 * t;
                        if (k < fs) {
                            const float2 o = s_d[slot(w0 + 64u * t)];
                            s_p[k] = make_float4(__fsub_rn(__fmul_rn(tu[t].x, o.x), __fmul_rn(tu[t].y, o.y)),
                                                 __fadd_rn(__fmul_rn(tu[t].x, o.y), __fmul_rn(tu[t].y, o.x)),
                                                 __fsub_rn(__fmul_rn(tl[t].x, o.x), __fmul_rn(tl[t].y, o.y)),
                                                 __fadd_rn(__fmul_rn(tl[t].x, o.y), __fmul_rn(tl[t].y, o.x)));
                        }
                    }
                    __syncthreads();
                    ur = ui = lr = li = 0.f;                    // :239-240
                    for (int k = 0; k < fs; ++k) {
                        const float4 q = s_p[k];
                        ur = __fadd_rn(ur, q.x); ui = __fadd_rn(ui, q.y);
                        lr = __fadd_rn(lr, q.z); li = __fadd_rn(li, q.w);
                    }
                } else {
                    ur = ui = lr = li = 0.f;
#pragma unroll
                    for (int t = 0; t < TPL; ++t) {
                        const float2 o = s_d[slot(w0 + 64u * t)];
                        ur = __builtin_fmaf(-tu[t].y, o.y, __builtin_fmaf(tu[t].x, o.x, ur));
                        ui = __builtin_fmaf(tu[t].y, o.x, __builtin_fmaf(tu[t].x, o.y, ui));
                        lr = __builtin_fmaf(-tl[t].y, o.y, __builtin_fmaf(tl[t].x, o.x, lr));
                        li = __builtin_fmaf(tl[t].y, o.x, __builtin_fmaf(tl[t].x, o.y, li));
                    }
#ifndef GRHIP_FLL_SKIP_REDUCE       // a diagnostic build leaves the butterfly out to time the rest of the step
                    // four quantities to two: v_permlane32_swap hands the upper half's `ur` to the lower half and the lower
                    // half's `lr` to the upper half, so one add leaves ur's sum over lane pairs (l, l + 32) in lanes 0 .. 31
                    // and lr's in lanes 32 .. 63; likewise ui and li
                    half_swap(ur, lr);
                    half_swap(ui, li);
                    float k0 = __fadd_rn(ur, lr), k1 = __fadd_rn(ui, li);
                    // two to one: v_permlane16_swap exchanges the odd rows of k0 with the even rows of k1, so the rows of 16
                    // lanes then hold partial sums of ur, ui, lr, li in this order
                    row_swap(k0, k1);
                    float u = __fadd_rn(k0, k1);
                    // the sum over a row of 16 lanes, in every lane of it, on the DPP path: lanes l ^ 1, l ^ 2, then the
                    // mirror images within 8 and within 16 lanes
                    u = __fadd_rn(u, dpp<0xB1>(u));             // quad_perm:[1,0,3,2]
                    u = __fadd_rn(u, dpp<0x4E>(u));             // quad_perm:[2,3,0,1]
                    u = __fadd_rn(u, dpp<0x141>(u));            // row_half_mirror
                    u = __fadd_rn(u, dpp<0x140>(u));            // row_mirror
                    ur = lane_read(u, 0); ui = lane_read(u, 16); lr = lane_read(u, 32); li = lane_read(u, 48);
#else
                    ur = lane_read(ur, 0); ui = lane_read(ui, 0); lr = lane_read(lr, 0); li = lane_read(li, 0);
#endif
                }
                // :245, norm(out_lower) - norm(out_upper)
                const float error = GENERIC ? __fsub_rn(__fadd_rn(__fmul_rn(lr, lr), __fmul_rn(li, li)),
                                                        __fadd_rn(__fmul_rn(ur, ur), __fmul_rn(ui, ui)))
                                            : __fsub_rn(__builtin_fmaf(lr, lr, __fmul_rn(li, li)), __builtin_fmaf(ur, ur, __fmul_rn(ui, ui)));
                fll_step(phase, freq, error, p);                                          // :247-249
                kf = lane == jj ? freq : kf;                                              // :252-254
                kp = lane == jj ? phase : kp;
                ke = lane == jj ? error : ke;
            }
            if (lane < cnt) {
                const long long i = (long long)s * n + base + g0 + lane;
                a.out[i] = s_d[slot((unsigned)(base + g0 + lane) - (unsigned)(fs - 1))];  // d[n - (fs - 1)]
                if (a.frq) {
                    a.frq[i] = kf; a.phs[i] = kp; a.err[i] = ke;
                }
            }
        }
        __syncthreads();
    }
    // what the next call needs: the last fs - 1 derotated samples and the last fs inputs (through LDS: a short call
    // moves part of xh within itself)
    for (int k = lane; k < fs - 1; k += 64) dh[k] = s_d[slot((unsigned)n - (unsigned)(fs - 1) + (unsigned)k)];
    for (int k = lane; k < fs; k += 64) {
        const long long j = n + k;
        s_x[k] = j < fs ? xh[j] : x[j - fs];
    }
    __syncthreads();
    for (int k = lane; k < fs; k += 64) xh[k] = s_x[k];
    if (lane == 0) {
        a.state[s].phase = phase;
        a.state[s].freq = freq;
    }
}

template <int TPL>
int fll_go(bool generic, const FllLaunch &a, hipStream_t st)
{
    if (generic) hipLaunchKernelGGL((fll_walk_kernel<TPL, true>), dim3(a.nstreams), dim3(64), 0, st, a);
    else hipLaunchKernelGGL((fll_walk_kernel<TPL, false>), dim3(a.nstreams), dim3(64), 0, st, a);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

}  // namespace

int fll_band_edge_launch(bool generic, const FllLaunch &a, hipStream_t st)
{
    if (a.n <= 0 || a.nstreams <= 0) return GRHIP_OK;
    if (a.fs < 1 || a.fs > FLL_MAX_TAPS) return fail(GRHIP_EINVAL, "fll_band_edge_cc: filter size 1 .. %d", FLL_MAX_TAPS);
    const int tpl = (a.fs + 63) / 64;           // taps per lane
    if (tpl <= 1) return fll_go<1>(generic, a, st);
    if (tpl <= 2) return fll_go<2>(generic, a, st);
    if (tpl <= 3) return fll_go<3>(generic, a, st);
    if (tpl <= 4) return fll_go<4>(generic, a, st);
    if (tpl <= 8) return fll_go<8>(generic, a, st);
    return fll_go<16>(generic, a, st);
}

}  // namespace grhip
