// arb_resampler.hip -- gr_pfb_arb_resampler_ccf / _fff (filter/gr_pfb_arb_resampler_ccf.cc:158-209): kernel.
//
// Output k of the reference's general_work is  out = o0 + o1*acc  with  o0 = filters[j].filter(&in[count]),
// o1 = diff_filters[j].filter(&in[count]).  Where (count, j, acc) of output k comes from does not depend on the data
// (ArbSched, sched_plan.h): every lane computes the place of its own outputs, there is no serial pass.
//
// arb_kernel: one workgroup = `tile` consecutive outputs of one capture (blockIdx.y), one output per lane and step
// (lane t: outputs t, t + 256, ...; neighbouring lanes read neighbouring samples).  The tile's input span
// [count_first, count_last + tpf) is staged through LDS once, eight loads in flight per lane; both tap banks sit
// beside it as interleaved (h, dh) pairs.  The compiler reads two neighbouring pairs with one ds_read2_b64, and two
// neighbouring samples with another (ccf; ds_read2_b32 for fff), so every pair of taps costs two ds_read2 per lane:
// the LDS, at 128 B/clk/CU for ds_read2_b64, is what bounds the loop.  The filter index differs from
// lane to lane, so the rows have an odd stride in 8-byte pairs: lanes on different filters hit different banks.
//
//   generic = true : gr_fir_XXX_generic.cc.t:28-78 for both filters (two accumulators for ccf, four for fff, the
//                    tail into acc0, unfused multiply then add; the Makefile's -ffp-contract=off keeps them apart), then o0 + o1*acc
//                    as a multiply and an add per component: bit-exact against the reference's generic build.
//   generic = false: one blended tap h + acc*dh per tap (an FMA), then FMAs into two accumulators.
#include "arb_resampler.h"
#include "fir_arith.h"
#include "grhip_internal.h"

namespace grhip {

namespace {

template <class T, bool GENERIC>
__global__ void __launch_bounds__(ARB_THREADS) arb_kernel(ArbLaunch a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float2 *hs = reinterpret_cast<float2 *>(smem);                                     // [R][S]
    T *xs = reinterpret_cast<T *>(smem + (size_t)a.R * a.S * sizeof(float2));       // [span_cap]
    const int t = threadIdx.x;
    const long long k0 = (long long)blockIdx.x * a.tile;
    if (k0 >= a.nout) return;
    const int kn = (int)(a.nout - k0 < a.tile ? a.nout - k0 : a.tile);
    const T *in = static_cast<const T *>(a.in) + (long long)blockIdx.y * a.in_stride;
    T *out = static_cast<T *>(a.out) + (long long)blockIdx.y * a.out_stride + k0;
    const unsigned R = (unsigned)a.R;

    // the tile's first count, and what local positions start from
    long long cf, clast;
    unsigned rb = 0, Tm = 0;
    if (a.sc.steps) {
        cf = a.sc.steps[k0].count;
        clast = a.sc.steps[k0 + kn - 1].count;
    } else {
        const unsigned long long Tb = a.sc.A0 + (unsigned long long)k0 * a.sc.F;
        const unsigned long long pb = a.sc.j0 + (unsigned long long)k0 * a.sc.D + (Tb >> 23);
        cf = a.sc.c0 + (long long)(pb / R);
        rb = (unsigned)(pb % R);
        Tm = (unsigned)(Tb & 0x7fffffu);
        const unsigned long long tl = Tm + (unsigned long long)(kn - 1) * a.sc.F;
        const unsigned pl = rb + (unsigned)(kn - 1) * a.sc.D + (unsigned)(tl >> 23);
        clast = cf + pl / R;
    }
    int span = (int)(clast - cf) + a.tpf;
    if (span > a.span_cap) span = a.span_cap;           // never past the LDS image (the host sizes tiles so it fits)

    for (int i = t; i < a.R * a.S; i += ARB_THREADS) hs[i] = a.taps[i];
    // fir_arith.h's stage_span written out: as a call it costs this kernel a different scalar register allocation
    const long long p0 = cf - a.lead;                    // physical index of xs[0]
    for (int ub = t; ub < span; ub += ARB_THREADS * 8) {
        T v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int u = ub + ARB_THREADS * i;
            const long long p = p0 + u;
            v[i] = zero_of(T());
            if (u < span && p >= 0 && p < a.n_phys) v[i] = in[p];
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int u = ub + ARB_THREADS * i;
            if (u < span) xs[u] = v[i];
        }
    }
    __syncthreads();

    for (int k = t; k < kn; k += ARB_THREADS) {
        int off, j;
        float acc;
        if (a.sc.steps) {
            const ArbStep s = a.sc.steps[k0 + k];
            off = (int)(s.count - cf); j = s.j; acc = s.acc;
        } else {
            const unsigned long long tl = Tm + (unsigned long long)k * a.sc.F;
            const unsigned pl = rb + (unsigned)k * a.sc.D + (unsigned)(tl >> 23);
            off = (int)(pl / R); j = (int)(pl - (unsigned)off * R);
            acc = (float)(unsigned)(tl & 0x7fffffu) * (1.0f / 8388608.0f);
        }
        const float2 *h = hs + j * a.S;
        const T *x = xs + off;
        const int n = a.tpf;
        T r;
        if (GENERIC) {
            // N_UNROLL accumulators (generate_gr_fir_XXX.py:59-64: 2 for a complex accumulator, 4 for a float one)
            constexpr int NU = sizeof(T) == 8 ? 2 : 4;
            T ac[NU], dc[NU];
#pragma unroll
            for (int q = 0; q < NU; ++q) { ac[q] = zero_of(T()); dc[q] = zero_of(T()); }
            const int nn = (n / NU) * NU;
            int i = 0;
#pragma unroll 4
            for (; i < nn; i += NU) {
#pragma unroll
                for (int q = 0; q < NU; ++q) {
                    const float2 hq = h[i + q];
                    const T xq = x[i + q];
                    ac[q] = mac_unfused(ac[q], hq.x, xq);
                    dc[q] = mac_unfused(dc[q], hq.y, xq);
                }
            }
            for (; i < n; ++i) {
                const float2 h0 = h[i];
                const T x0 = x[i];
                ac[0] = mac_unfused(ac[0], h0.x, x0);
                dc[0] = mac_unfused(dc[0], h0.y, x0);
            }
            T o0 = ac[0], o1 = dc[0];
#pragma unroll
            for (int q = 1; q < NU; ++q) { o0 = add(o0, ac[q]); o1 = add(o1, dc[q]); }   // acc0 + acc1 (+ acc2 + acc3)
            r = mac_unfused(o0, acc, o1);                  // o0 + o1*acc
        } else {
            T a0 = zero_of(T()), a1 = zero_of(T());
            int i = 0;
#pragma unroll 4
            for (; i + 1 < n; i += 2) {
                const float2 h0 = h[i], h1 = h[i + 1];
                a0 = mac_fma(a0, __builtin_fmaf(acc, h0.y, h0.x), x[i]);
                a1 = mac_fma(a1, __builtin_fmaf(acc, h1.y, h1.x), x[i + 1]);
            }
            if (i < n) a0 = mac_fma(a0, __builtin_fmaf(acc, h[i].y, h[i].x), x[i]);
            r = add(a0, a1);
        }
        out[k] = r;
    }
}

template <class T, bool GENERIC>
int launch_t(const ArbLaunch &a, hipStream_t st)
{
    if (a.nout <= 0 || a.n_streams <= 0) return GRHIP_OK;
    const size_t lds = (size_t)a.R * a.S * sizeof(float2) + (size_t)a.span_cap * sizeof(T);
    const long long blocks = (a.nout + a.tile - 1) / a.tile;
    if (blocks > 0x7fffffffLL || a.n_streams > 65535) return fail(GRHIP_EINVAL, "pfb_arb_resampler: grid too large");
    hipLaunchKernelGGL((arb_kernel<T, GENERIC>), dim3((unsigned)blocks, (unsigned)a.n_streams), dim3(ARB_THREADS),
                       lds, st, a);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

}  // namespace

int arb_resampler_launch(bool complex, bool generic, const ArbLaunch &a, hipStream_t st)
{
    if (complex) return generic ? launch_t<float2, true>(a, st) : launch_t<float2, false>(a, st);
    return generic ? launch_t<float, true>(a, st) : launch_t<float, false>(a, st);
}

}  // namespace grhip
