// frac_interp.hip -- gr_fractional_interpolator_ff / _cc (filter/gr_fractional_interpolator_ff.cc:67-93): kernel.
//
// Output k of the reference's general_work is filters[imu_k]->filter(&in[ii_k]) with the 8-tap MMSE bank
// (filter/gri_mmse_fir_interpolator.cc:61-71).  Where (ii_k, imu_k) comes from does not depend on the data
// (FracSched, sched_plan.h): every lane computes the place of its own outputs, there is no serial pass.
//
// frac_kernel: one workgroup = `tile` consecutive outputs of one capture (blockIdx.y), one output per lane and step
// (lane t: outputs t, t + 256, ...; neighbouring lanes read neighbouring samples).  The tile's input span
// [ii_first, ii_last + 8) is staged through LDS once, eight loads in flight per lane.  The 129 x 8 bank sits beside it
// (4128 B) as 32-byte rows, one per filter, read as two 16-byte halves.  A 16-byte read is served to 16 lanes per LDS
// cycle from a 256-byte line of banks, which holds eight rows: with the halves in place, the sixteen lanes' first
// halves could use only eight of its sixteen slots.  So the rows of every other group of eight filters hold their
// halves swapped, and filters imu and imu + 8 never meet on a slot.
//
//   generic = true : gr_fir_fff_generic / gr_fir_ccf_generic (gr_fir_XXX_generic.cc.t:28-78) over 8 taps: four float
//                    accumulators acc_j = (0 + t[j]x[j]) + t[j+4]x[j+4] summed ((a0+a1)+a2)+a3 for ff, two complex
//                    ones over the even and the odd taps and their sum for cc; unfused multiply then add (the
//                    Makefile's -ffp-contract=off keeps them apart): bit-exact against the reference's generic build.
//   generic = false: FMAs into two accumulators.
#include "fir_arith.h"
#include "frac_interp.h"
#include "grhip_internal.h"

namespace grhip {

namespace {

constexpr int FRAC_BANK = FRAC_NTAPS * (FRAC_NSTEPS + 1);       // 1032 floats

template <class T, bool GENERIC>
__global__ void __launch_bounds__(FRAC_THREADS) frac_kernel(FracLaunch a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *hs = reinterpret_cast<float *>(smem);                                // [129][8], halves swizzled
    T *xs = reinterpret_cast<T *>(smem + (size_t)FRAC_BANK * sizeof(float));   // [span_cap]; 4128 is a multiple of 16
    const int t = threadIdx.x;
    const long long k0 = (long long)blockIdx.x * a.tile;
    if (k0 >= a.nout) return;
    const int kn = (int)(a.nout - k0 < a.tile ? a.nout - k0 : a.tile);
    const T *in = static_cast<const T *>(a.in) + (long long)blockIdx.y * a.in_stride;
    T *out = static_cast<T *>(a.out) + (long long)blockIdx.y * a.out_stride + k0;
    const bool first = a.sc.first_one && k0 == 0;        // this tile's output 0 is the mu == 1 one

    // the tile's first and last position, and what local positions start from
    long long cf, clast;
    unsigned long long Tm = 0;
    int boff = 0;
    if (a.sc.steps) {
        cf = (long long)(a.sc.steps[k0] >> 8);
        clast = (long long)(a.sc.steps[k0 + kn - 1] >> 8);
    } else {
        const unsigned long long Tb = a.sc.A0 + (unsigned long long)k0 * a.sc.F;
        const long long iib = a.sc.ii0 + (long long)(Tb >> 24);
        Tm = Tb & 0xffffffull;
        cf = first ? a.sc.ii0 : iib;
        boff = (int)(iib - cf);
        clast = (first && kn == 1) ? cf : iib + (long long)((Tm + (unsigned long long)(kn - 1) * a.sc.F) >> 24);
    }
    int span = (int)(clast - cf) + FRAC_NTAPS;
    if (span > a.span_cap) span = a.span_cap;           // never past the LDS image (the host sizes tiles so it fits)

    for (int i = t; i < FRAC_BANK; i += FRAC_THREADS) {
        const int k = i / (FRAC_NSTEPS + 1), imu = i - k * (FRAC_NSTEPS + 1);       // taps[k][imu], coalesced
        hs[imu * FRAC_NTAPS + (k ^ (((imu >> 3) & 1) << 2))] = a.taps[i];
    }
    stage_span<T, FRAC_THREADS>(xs, in, cf, span, a.n_phys);
    __syncthreads();

    const int off_max = a.span_cap - FRAC_NTAPS;
    for (int k = t; k < kn; k += FRAC_THREADS) {
        int off, imu;
        if (a.sc.steps) {
            const unsigned long long s = a.sc.steps[k0 + k];
            off = (int)((long long)(s >> 8) - cf); imu = (int)(s & 0xffu);
        } else if (first && k == 0) {
            off = 0; imu = FRAC_NSTEPS;
        } else {
            const unsigned long long tl = Tm + (unsigned long long)k * a.sc.F;
            off = boff + (int)(tl >> 24);
            imu = frac_imu_of((unsigned)(tl & 0xffffffull));
        }
        off = off < 0 ? 0 : (off > off_max ? off_max : off);        // the host's tiles keep it inside; never read past xs
        imu = imu > FRAC_NSTEPS ? FRAC_NSTEPS : imu;
        const float4 *row = reinterpret_cast<const float4 *>(hs + imu * FRAC_NTAPS);
        const int sw = (imu >> 3) & 1;
        const float4 ha = row[sw], hb = row[sw ^ 1];
        const float h[8] = {ha.x, ha.y, ha.z, ha.w, hb.x, hb.y, hb.z, hb.w};
        const T *xp = xs + off;
        T x[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) x[i] = xp[i];
        T r;
        if (GENERIC) {
            // N_UNROLL accumulators (generate_gr_fir_XXX.py:59-64: 2 for a complex accumulator, 4 for a float one),
            // each starting from 0 as the reference's do
            constexpr int NU = sizeof(T) == 8 ? 2 : 4;
            T ac[NU];
#pragma unroll
            for (int q = 0; q < NU; ++q) ac[q] = zero_of(T());
#pragma unroll
            for (int i = 0; i < FRAC_NTAPS; i += NU)
#pragma unroll
                for (int q = 0; q < NU; ++q) ac[q] = mac_unfused(ac[q], h[i + q], x[i + q]);
            r = ac[0];
#pragma unroll
            for (int q = 1; q < NU; ++q) r = add(r, ac[q]);
        } else {
            T a0 = zero_of(T()), a1 = zero_of(T());
#pragma unroll
            for (int i = 0; i < FRAC_NTAPS; i += 2) {
                a0 = mac_fma(a0, h[i], x[i]);
                a1 = mac_fma(a1, h[i + 1], x[i + 1]);
            }
            r = add(a0, a1);
        }
        out[k] = r;
    }
}

template <class T, bool GENERIC>
int launch_t(const FracLaunch &a, hipStream_t st)
{
    if (a.nout <= 0 || a.n_streams <= 0) return GRHIP_OK;
    if (a.tile < 1 || a.tile > FRAC_TILE || a.span_cap < FRAC_NTAPS || (size_t)a.span_cap * sizeof(T) > (size_t)FRAC_SPAN_BYTES)
        return fail(GRHIP_EINVAL, "fractional_interpolator: bad tile");
    const size_t lds = (size_t)FRAC_BANK * sizeof(float) + (size_t)a.span_cap * sizeof(T);
    const long long blocks = (a.nout + a.tile - 1) / a.tile;
    if (blocks > 0x7fffffffLL || a.n_streams > 65535) return fail(GRHIP_EINVAL, "fractional_interpolator: grid too large");
    hipLaunchKernelGGL((frac_kernel<T, GENERIC>), dim3((unsigned)blocks, (unsigned)a.n_streams), dim3(FRAC_THREADS),
                       lds, st, a);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

}  // namespace

int frac_interp_launch(bool complex, bool generic, const FracLaunch &a, hipStream_t st)
{
    if (complex) return generic ? launch_t<float2, true>(a, st) : launch_t<float2, false>(a, st);
    return generic ? launch_t<float, true>(a, st) : launch_t<float, false>(a, st);
}

}  // namespace grhip
