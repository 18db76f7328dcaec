// pfb_clock_sync.hip -- gr_pfb_clock_sync_ccf (gnuradio-core/src/lib/filter/gr_pfb_clock_sync_ccf.cc:351-427), the
// polyphase timing-recovery loop.
//
// What is computed (include/grhip.h states the contract): xz is tpf + isps - 1 zeros followed by the stream; a symbol
// takes osps outputs of the matched bank's arm floor(k) at pos, pos + 1, ..., one output of the derivative bank's arm
// at pos, steps k and rate_f with the error and moves pos on by isps; a wrap of k over [0, nfilters) carries into pos.
// The scalar chain is pcs_wrap / pcs_advance / pcs_step of pfb_clock_sync.h, the same text the host compiles.
//
// One wavefront per stream, the shape of fll_walk_kernel (fll_band_edge.hip).  A window of PCS_WIN items of xz sits in
// LDS, starting at the limit `lo` below which the next symbol cannot read; the PCS_WIN items behind it are requested
// while the window is walked and wait in registers.  When no further symbol fits, the window's tail moves to its
// front, the registers fill the rest and the next loads go out.  The two banks sit in LDS arm by arm with an arm's
// taps reversed and consecutive: lanes read consecutive words whichever the arm is, so the arm index costs no bank
// conflict.  Lane l owns taps l, l + 64, ... of the matched and of the derivative arm; the scalar chain is uniform over
// the wave.  The results of up to PCS_GROUP symbols are staged in LDS and stored coalesced.
//   GENERIC = true:  the lanes put their taps' products into LDS and the sums run in gr_fir_ccf_generic's order
//           (gr_fir_XXX_generic.cc.t:59-79: two complex accumulators over the even and the odd taps, the tail of an odd
//           count into the first, then acc0 + acc1), every product and sum rounded once; every lane runs them, so the
//           result is uniform without a broadcast.  Bit for bit the restatement, tests/pfb_clock_sync_ref.py.
//   GENERIC = false: fused multiply-adds per lane and the FLL's transposing butterfly over the four sums (two half-wave
//           swaps, a row swap, four DPP steps, four lane reads).  The scalar chain is the same arithmetic.
//
// Termination and bounds, for every bit pattern of the samples and the state.  The only loops whose trip count depends
// on data are pcs_wrap's two, which count to PCS_WRAP_TRIPS together; fmod on doubles ends for every argument, and a k
// that is not finite is made 0 before anything is derived from it.  Every symbol leaves `lo` at least one item further
// (pcs_wrap puts an evaluation at `lo` or behind it, and the next symbol's `lo` lies one item behind this symbol's last
// evaluation), and a symbol starts only while pos + need <= arrived, so the symbol loop ends after at most one trip per
// item, and every window holds at least one symbol (the static_assert of pfb_clock_sync_launch.h).  An evaluation
// stands at pos in [lo, start + osps * PCS_CARRY], so it reads window items from lo - w0 >= 0 up to start + need - w0
// <= PCS_WIN; the index is clamped to that range all the same, and a clamp that fires counts a slip.  Global reads go
// through xz_at, which returns 0 outside [arrived - hist, arrived + n); the stores are below produced <= out_cap, which the host holds against
// grhip_pfb_clock_sync_ccf_max_produced, and the store loop checks it again.  Bank indices are arm * tpf + j with the
// arm in [0, nfilters) by pcs_wrap and j < tpf.
#include <cmath>

#include "device_math.h"
#include "pfb_clock_sync_launch.h"

namespace grhip {

namespace {

constexpr int PCS_KEEP = PCS_WIN / 2;       // the most a window keeps of the one before

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

template <int CTRL>
__device__ __forceinline__ float dpp(float v)
{
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xf, 0xf, false));
}

// xz[j] for a stream: the kept history below `arrived`, this call's items from there on, 0 outside both
__device__ __forceinline__ float2 xz_at(long long j, long long arrived, int hist, int n, const float2 *__restrict__ h,
                                        const float2 *__restrict__ x)
{
    const long long ih = j - (arrived - hist), ix = j - arrived;
    if (ix >= 0) return ix < n ? x[ix] : make_float2(0.f, 0.f);
    return ih >= 0 ? h[ih] : make_float2(0.f, 0.f);
}

template <int TPL, bool GENERIC>
__global__ void __launch_bounds__(64)
pcs_walk_kernel(PcsLaunch a)
{
    __shared__ float2 s_x[PCS_WIN];                             // the window's items of xz
    __shared__ float s_b[PCS_MAX_BANK], s_d[PCS_MAX_BANK];      // the two banks
    __shared__ float4 s_p[GENERIC ? PCS_MAX_TPF : 1];           // an evaluation's products: matched re, im, derivative re, im
    __shared__ float2 s_o[PCS_GROUP * PCS_MAX_OSPS];            // a group's outputs
    __shared__ float4 s_a[PCS_GROUP];                           // a group's error, rate and k
    const int s = blockIdx.x, lane = threadIdx.x;
    const PcsParams p = a.p;
    const int nf = p.nfilters, tpf = p.tpf, isps = p.isps, osps = p.osps, n = a.n;
    const int need = pcs_need(tpf, osps), hist = pcs_hist(tpf, isps, osps);
    const long long arrived0 = a.arrived, arrived = a.arrived + n;
    const float2 *__restrict__ x = a.in + (long long)s * n;
    float2 *__restrict__ h = a.hist + (long long)s * hist;
    PcsState st = a.state[s];
    long long produced = 0;

    for (int q = lane; q < nf * tpf; q += 64) {
        s_b[q] = a.bank[q];
        s_d[q] = a.dbank[q];
    }

    long long w0 = st.pos - isps + 1 > 0 ? st.pos - isps + 1 : 0;       // the window starts at the next symbol's `lo`
    float2 v[PCS_WIN / 64];
    if (st.pos + need <= arrived) {
#pragma unroll
        for (int q = 0; q < PCS_WIN / 64; ++q) s_x[lane + 64 * q] = xz_at(w0 + lane + 64 * q, arrived0, hist, n, h, x);
    }
    while (st.pos + need <= arrived) {
        // the items behind the window, in flight while it is walked
#pragma unroll
        for (int q = 0; q < PCS_WIN / 64; ++q) v[q] = xz_at(w0 + PCS_WIN + lane + 64 * q, arrived0, hist, n, h, x);
        __syncthreads();
        const long long wend = arrived < w0 + PCS_WIN ? arrived : w0 + PCS_WIN;
        while (st.pos + need <= wend) {
            int m = 0;
            for (; m < PCS_GROUP && st.pos + need <= wend; ++m) {
                const long long lo = st.pos - isps + 1 > 0 ? st.pos - isps + 1 : 0;
                float o0r = 0.f, o0i = 0.f, dr = 0.f, di = 0.f;
                for (int kk = 0; kk < osps; ++kk) {
                    int trips = 0;
                    const int fn = pcs_wrap(st.k, st.pos, lo, nf, st.slips, trips);             // :381-395
                    const bool last = kk == osps - 1;
                    int rel = (int)(st.pos - w0) + kk, reld = (int)(st.pos - w0);
                    // out of reach by the argument above; were it ever broken, the clamp would show as a slip
                    if (reld < 0 || rel > PCS_WIN - tpf) ++st.slips;
                    rel = rel < 0 ? 0 : rel > PCS_WIN - tpf ? PCS_WIN - tpf : rel;
                    reld = reld < 0 ? 0 : reld > PCS_WIN - tpf ? PCS_WIN - tpf : reld;
                    const float *__restrict__ tb = s_b + fn * tpf, *__restrict__ td = s_d + fn * tpf;
                    float mr, mi;
                    if (GENERIC) {
                        __syncthreads();
#pragma unroll
                        for (int t = 0; t < TPL; ++t) {
                            const int j = lane + 64 * t;
                            if (j < tpf) {
                                const float2 xm = s_x[rel + j];
                                const float tm = tb[j];
                                float4 q = make_float4(__fmul_rn(tm, xm.x), __fmul_rn(tm, xm.y), 0.f, 0.f);
                                if (last) {                     // the derivative arm goes with the last evaluation only
                                    const float2 xd = s_x[reld + j];
                                    const float tdv = td[j];
                                    q.z = __fmul_rn(tdv, xd.x);
                                    q.w = __fmul_rn(tdv, xd.y);
                                }
                                s_p[j] = q;
                            }
                        }
                        __syncthreads();
                        const float4 sums = fir_ccf_generic_sums(s_p, tpf);                     // .cc.t:59-79 (device_math.h)
                        mr = sums.x; mi = sums.y;
                        if (last) {
                            dr = sums.z;
                            di = sums.w;
                        }
                    } else {
                        float er = 0.f, ei = 0.f;
                        mr = mi = 0.f;
#pragma unroll
                        for (int t = 0; t < TPL; ++t) {
                            const int j = lane + 64 * t;
                            if (j < tpf) {
                                const float2 xm = s_x[rel + j];
                                const float tm = tb[j];
                                mr = __builtin_fmaf(tm, xm.x, mr);
                                mi = __builtin_fmaf(tm, xm.y, mi);
                                if (last) {                     // the derivative arm goes with the last evaluation only
                                    const float2 xd = s_x[reld + j];
                                    const float tdv = td[j];
                                    er = __builtin_fmaf(tdv, xd.x, er);
                                    ei = __builtin_fmaf(tdv, xd.y, ei);
                                }
                            }
                        }
                        // the FLL's butterfly (fll_band_edge.hip): four quantities to two with two half-wave swaps, two
                        // to one with a row swap, then the sum over a row of 16 lanes on the DPP path
                        half_swap(mr, er);
                        half_swap(mi, ei);
                        float k0 = __fadd_rn(mr, er), k1 = __fadd_rn(mi, ei);
                        row_swap(k0, k1);
                        float u = __fadd_rn(k0, k1);
                        u = __fadd_rn(u, dpp<0xB1>(u));             // quad_perm:[1,0,3,2]
                        u = __fadd_rn(u, dpp<0x4E>(u));             // quad_perm:[2,3,0,1]
                        u = __fadd_rn(u, dpp<0x141>(u));            // row_half_mirror
                        u = __fadd_rn(u, dpp<0x140>(u));            // row_mirror
                        mr = lane_read(u, 0); mi = lane_read(u, 16);
                        if (last) {
                            dr = lane_read(u, 32);
                            di = lane_read(u, 48);
                        }
                    }
                    if (kk == 0) {
                        o0r = mr;
                        o0i = mi;
                    }
                    if (lane == 0) s_o[m * osps + kk] = make_float2(mr, mi);                    // :397
                    st.k = pcs_advance(st.k, p.rate_i, st.rate_f);                              // :398
                }
                if (lane == 0) s_a[m] = make_float4(st.error, st.rate_f, st.k, 0.f);            // :400-404
                pcs_step(st, p, o0r, o0i, dr, di);                                              // :408-419
                st.pos += isps;                                                                 // :422
            }
            __syncthreads();
            const int cnt = m * osps;
            for (int i = lane; i < cnt; i += 64) {
                const long long at = produced + i;
                if (at < a.out_cap) {
                    const long long g = (long long)s * a.out_cap + at;
                    a.out[g] = s_o[i];
                    if (a.err) {
                        const float4 q = s_a[i / osps];
                        a.err[g] = q.x; a.rate[g] = q.y; a.k[g] = q.z;
                    }
                }
            }
            produced += cnt;
            __syncthreads();
        }
        if (st.pos + need > arrived) break;
        // the next window starts at the next symbol's `lo`: its front is this window's tail, the rest waits in v
        const long long w1 = st.pos - isps + 1;
        int sh = (int)(w1 - w0);
        if (sh < PCS_WIN - PCS_KEEP || sh > PCS_WIN) ++st.slips;                               // as above: out of reach, and visible if not
        sh = sh < PCS_WIN - PCS_KEEP ? PCS_WIN - PCS_KEEP : sh > PCS_WIN ? PCS_WIN : sh;       // within [WIN - KEEP, WIN] by the bounds above
        float2 keep[PCS_KEEP / 64];
#pragma unroll
        for (int q = 0; q < PCS_KEEP / 64; ++q) {
            const int i = sh + lane + 64 * q;
            keep[q] = i < PCS_WIN ? s_x[i] : make_float2(0.f, 0.f);
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < PCS_KEEP / 64; ++q) {
            const int i = lane + 64 * q;
            if (i < PCS_WIN - sh) s_x[i] = keep[q];
        }
#pragma unroll
        for (int q = 0; q < PCS_WIN / 64; ++q) {
            const int i = PCS_WIN - sh + lane + 64 * q;
            if (i < PCS_WIN) s_x[i] = v[q];
        }
        w0 += sh;
    }
    __syncthreads();
    // what the next call needs: the last `hist` items of xz (through LDS: a short call moves part of the history
    // within itself) and the state
    for (int i = lane; i < hist; i += 64) s_x[i] = xz_at(arrived - hist + i, arrived0, hist, n, h, x);
    __syncthreads();
    for (int i = lane; i < hist; i += 64) h[i] = s_x[i];
    if (lane == 0) {
        a.state[s] = st;
        a.produced[s] = (int)produced;
    }
}

template <int TPL>
int pcs_go(bool generic, const PcsLaunch &a, hipStream_t st)
{
    if (generic) hipLaunchKernelGGL((pcs_walk_kernel<TPL, true>), dim3(a.nstreams), dim3(64), 0, st, a);
    else hipLaunchKernelGGL((pcs_walk_kernel<TPL, false>), dim3(a.nstreams), dim3(64), 0, st, a);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

}  // namespace

int pfb_clock_sync_launch(bool generic, const PcsLaunch &a, hipStream_t st)
{
    if (a.n < 0 || a.nstreams <= 0) return GRHIP_OK;
    const PcsParams &p = a.p;
    if (p.nfilters < 1 || p.nfilters > PCS_MAX_FILTERS || p.tpf < 1 || p.tpf > PCS_MAX_TPF || p.nfilters * p.tpf > PCS_MAX_BANK ||
        p.isps < 1 || p.isps >= PCS_MAX_SPS || p.osps < 1 || p.osps > PCS_MAX_OSPS)
        return fail(GRHIP_EINVAL, "pfb_clock_sync_ccf: shape out of range");
    const int tpl = (p.tpf + 63) / 64;          // taps per lane
    if (tpl <= 1) return pcs_go<1>(generic, a, st);
    if (tpl <= 2) return pcs_go<2>(generic, a, st);
    return pcs_go<4>(generic, a, st);
}

}  // namespace grhip
