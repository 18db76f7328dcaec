// resampler.hip -- gr_rational_resampler_base_XXX / gr_interp_fir_filter_XXX (ccf, fff, ccc): kernel.
//
// gr_rational_resampler_base_XXX.cc.t:144-172: out[i++] = firs[ctr]->filter(in); ctr += D; while (ctr >= I) { ctr -= I;
// in++; }.  Output o of a call that starts at ctr = c0 uses filter (c0 + o*D) % I at input (c0 + o*D) / I, and with
// g = gcd(I, D), P = I/g, Dp = D/g every output o = m*P + r of residue r uses the same filter f_r, at input s_r + m*Dp
// (RsLaunch, resampler.h).  gr_interp_fir_filter_XXX is the case D = 1, c0 = 0 on a stream that carries its history.
//
// rs_kernel: one workgroup = TM periods x RB residues of one capture (blockIdx.y).  A wave task is 64 consecutive
// periods (one per lane) of RG residues, so every lane of a wave uses the same taps: their loads are wave-uniform
// (scalar loads, no per-lane filter rows in LDS).  The workgroup's input span is staged in LDS in Dp phase rows (item v at
// row v % Dp, column v / Dp): the lanes of a wave then read consecutive LDS words for every Dp, with no bank conflicts.
// The outputs go through LDS too and leave as rows of RB consecutive items (the whole tile when RB = P).
//
//   generic = true : RG = 1; gr_fir_XXX_generic.cc.t:28-78 per output (2 accumulators for ccf/ccc, 4 for fff, the
//                    tail into acc0, products and sums unfused; the Makefile's -ffp-contract=off keeps them apart, the
//                    complex product as (ac - bd, ad + bc)): bit-exact against the reference's generic build.
//   generic = false: RG residues per task share each input item read from LDS (RG FMAs per read).  Residue q of the
//                    group starts d_q items after the group's first; its taps come from a bank row padded with WP zeros
//                    on both sides, so every residue runs the same loop over u < nt + d_max with tap [WP - d_q + u].
#include "fir_arith.h"
#include "resampler.h"
#include "grhip_internal.h"

#include <algorithm>

namespace grhip {

namespace {

template <class T, class H, bool GENERIC, int RG>
__global__ void __launch_bounds__(RS_THREADS)
rs_kernel(const T *__restrict__ in, T *__restrict__ out, const H *__restrict__ bank, RsLaunch a, int RB, int TM, int L,
          int nrb)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    T *xs = reinterpret_cast<T *>(smem);                       // [Dp][L] input phase rows
    T *os = xs + (size_t)a.Dp * L;                             // [TM][rn] outputs
    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const long long tile = blockIdx.x / nrb;
    const int rb = (int)(blockIdx.x - tile * nrb);
    const int P = a.P, Dp = a.Dp, nt = a.nt;
    const int r0 = rb * RB;
    const int rn = min(RB, P - r0);
    const long long m0 = tile * TM;
    const long long nper = (a.nout + P - 1) / P;
    if (m0 >= nper || rn <= 0) return;
    const int mn = (int)min((long long)TM, nper - m0);
    in += (long long)blockIdx.y * a.in_stride;
    out += (long long)blockIdx.y * a.out_stride;

    // the span: residues r0 .. r0+rn-1 of periods m0 .. m0+mn-1
    const unsigned long long p0 = a.c0 + (unsigned long long)r0 * a.D;
    const long long s0 = (long long)(p0 / a.I);
    const long long s_last = (long long)((a.c0 + (unsigned long long)(r0 + rn - 1) * a.D) / a.I);
    const long long first = s0 + m0 * Dp - a.lead;            // physical index of span item 0
    const int span = (int)(s_last - s0) + (mn - 1) * Dp + nt;
    for (int vb = t; vb < span; vb += RS_THREADS * 4) {
        T v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int u = vb + RS_THREADS * i;
            const long long p = first + u;
            v[i] = zero_of(T());
            if (u < span && p >= 0 && p < a.n_phys) v[i] = in[p];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int u = vb + RS_THREADS * i;
            if (u < span) xs[(u % Dp) * L + u / Dp] = v[i];
        }
    }
    __syncthreads();

    const int ng = (rn + RG - 1) / RG;
    const int tasks = (TM / 64) * ng;
    for (int task = wave; task < tasks; task += RS_THREADS / 64) {
        const int c = task / ng, gi = task - c * ng;
        const int ml = c * 64 + lane;
        const int rg0 = r0 + gi * RG;
        const unsigned long long pg = a.c0 + (unsigned long long)rg0 * a.D;
        const long long sg = (long long)(pg / a.I);
        const H *hrow[RG];
        int dmax = 0;
#pragma unroll
        for (int q = 0; q < RG; ++q) {
            const int r = rg0 + q;
            long long f = (long long)a.I, d = 0;                // row I: zeros (a residue past the block's last)
            if (r < r0 + rn) {
                const unsigned long long p = a.c0 + (unsigned long long)r * a.D;
                f = (long long)(p % a.I);
                d = (long long)(p / a.I) - sg;
                dmax = (int)d;
            }
            hrow[q] = bank + f * a.RS + a.WP - d;
        }
        // LDS walk: item v = base + ml*Dp + u sits at row (base + u) % Dp, column (base + u) / Dp + ml
        const int base = (int)(sg - s0);
        int ph = base % Dp;
        int uo = ph * L + base / Dp;
        const T *xl = xs + ml;
        T r;
        T acc[GENERIC ? (sizeof(T) == 8 ? 2 : 4) : RG];
        if (GENERIC) {
            constexpr int NU = sizeof(T) == 8 ? 2 : 4;     // generate_gr_fir_XXX.py:59-64
            const H *h = hrow[0];
#pragma unroll
            for (int q = 0; q < NU; ++q) acc[q] = zero_of(T());
            const int nn = (nt / NU) * NU;
            int k = 0;
            for (; k < nn; k += NU) {
#pragma unroll
                for (int q = 0; q < NU; ++q) {
                    acc[q] = mac_unfused(acc[q], h[k + q], xl[uo]);
                    if (++ph == Dp) { ph = 0; uo += 1 - (Dp - 1) * L; } else uo += L;
                }
            }
            for (; k < nt; ++k) {
                acc[0] = mac_unfused(acc[0], h[k], xl[uo]);
                if (++ph == Dp) { ph = 0; uo += 1 - (Dp - 1) * L; } else uo += L;
            }
            r = acc[0];
#pragma unroll
            for (int q = 1; q < NU; ++q) r = add(r, acc[q]);   // acc0 + acc1 (+ acc2 + acc3)
            if (ml < mn) os[ml * rn + (rg0 - r0)] = r;
        } else {
#pragma unroll
            for (int q = 0; q < RG; ++q) acc[q] = zero_of(T());
            const int nu = nt + dmax;
            // unrolled so that the scalar tap loads of UNR steps are issued together and waited for once
            constexpr int UNR = RG <= 2 ? 16 : RG <= 4 ? 8 : 4;
#pragma unroll UNR
            for (int u = 0; u < nu; ++u) {
                const T x = xl[uo];
#pragma unroll
                for (int q = 0; q < RG; ++q) acc[q] = mac_fma(acc[q], hrow[q][u], x);
                if (++ph == Dp) { ph = 0; uo += 1 - (Dp - 1) * L; } else uo += L;
            }
            if (ml < mn) {
#pragma unroll
                for (int q = 0; q < RG; ++q)
                    if (rg0 + q < r0 + rn) os[ml * rn + (rg0 + q - r0)] = acc[q];
            }
        }
    }
    __syncthreads();

    // rows of rn consecutive outputs: (m0 + ml)*P + r0 .. + rn - 1
    const int n_st = mn * rn;
    for (int i = t; i < n_st; i += RS_THREADS) {
        const int ml = i / rn, rr = i - ml * rn;
        const long long o = (m0 + ml) * P + r0 + rr;
        if (o < a.nout) out[o] = os[i];
    }
}

template <class T, class H, bool GENERIC, int RG>
void *kernel_ptr()
{
    return (void *)rs_kernel<T, H, GENERIC, RG>;
}

template <class T, class H, bool GENERIC, int RG>
int launch_t(const RsLaunch &a, const RsConfig &c, hipStream_t st)
{
    const long long nper = (a.nout + a.P - 1) / a.P;
    const long long tiles = (nper + c.TM - 1) / c.TM;
    const int nrb = (a.P + c.RB - 1) / c.RB;
    if (tiles * nrb > 0x7fffffffLL || a.n_streams > 65535) return fail(GRHIP_EINVAL, "rational_resampler: grid too large");
    hipLaunchKernelGGL((rs_kernel<T, H, GENERIC, RG>), dim3((unsigned)(tiles * nrb), (unsigned)a.n_streams),
                       dim3(RS_THREADS), c.lds, st, static_cast<const T *>(a.in), static_cast<T *>(a.out),
                       static_cast<const H *>(a.bank), a, c.RB, c.TM, c.L, nrb);
    GRHIP_HIP(hipGetLastError());
    return GRHIP_OK;
}

template <class T, class H>
int launch_kind(bool generic, const RsLaunch &a, const RsConfig &c, hipStream_t st)
{
    if (generic) return launch_t<T, H, true, 1>(a, c, st);
    switch (c.RG) {
    case 1: return launch_t<T, H, false, 1>(a, c, st);
    case 2: return launch_t<T, H, false, 2>(a, c, st);
    case 3: return launch_t<T, H, false, 3>(a, c, st);
    case 4: return launch_t<T, H, false, 4>(a, c, st);
    case 8: return launch_t<T, H, false, 8>(a, c, st);
    }
    return fail(GRHIP_EINVAL, "rational_resampler: bad residue group %d", c.RG);
}

template <class T, class H>
int prepare_kind()
{
    void *k[] = {kernel_ptr<T, H, true, 1>(), kernel_ptr<T, H, false, 1>(), kernel_ptr<T, H, false, 2>(),
                 kernel_ptr<T, H, false, 3>(), kernel_ptr<T, H, false, 4>(), kernel_ptr<T, H, false, 8>()};
    for (void *f : k)
        if (int rc = allow_lds(f, RS_LDS_MAX)) return rc;
    return GRHIP_OK;
}

size_t item_of(RsKind k) { return k == RS_FFF ? 4 : 8; }

unsigned long long gcd_u(unsigned long long a, unsigned long long b)
{
    while (b) { const unsigned long long t = a % b; a = b; b = t; }
    return a;
}

}  // namespace

int rs_group(int P, bool generic)
{
    if (generic) return 1;
    return P <= 4 ? P : 8;
}

int rs_config(RsKind kind, bool generic, unsigned long long I, unsigned long long D, int nt, long long nperiods,
              RsConfig *cfg)
{
    const unsigned long long g = gcd_u(I, D);
    const unsigned long long P = I / g, Dp = D / g;
    const size_t item = item_of(kind);
    RsConfig c;
    c.RG = rs_group((int)std::min<unsigned long long>(P, 64), generic);
    for (int RB : {64, 32, 16, 8}) {
        c.RB = P <= 64 ? (int)P : RB;
        if (P <= 64 && RB != 64) break;
        // s_{r0+RB-1} - s_{r0} <= ceil((RB-1)*D / I)
        const unsigned long long spr = ((unsigned long long)(c.RB - 1) * D + I - 1) / I;
        int best = 0;
        for (int C = 16; C >= 1; C /= 2) {
            const unsigned long long span = spr + (unsigned long long)(64 * C - 1) * Dp + (unsigned long long)nt;
            const unsigned long long Lr = span / Dp + 2;
            const unsigned long long lds = (Dp * Lr + (unsigned long long)64 * C * c.RB) * item;
            if (span > 0x7fffffffULL || lds > RS_LDS_MAX) continue;
            if (!best || lds <= RS_LDS_SOFT) best = C;
            if (lds <= RS_LDS_SOFT) break;
        }
        if (!best) continue;
        // small launches: smaller tiles, so that more workgroups share the work
        const int nrb = (int)((P + c.RB - 1) / c.RB);
        while (best > 1 && nperiods > 0 && (nperiods + 64LL * best - 1) / (64LL * best) * nrb < 512) best /= 2;
        c.TM = 64 * best;
        const unsigned long long span = spr + (unsigned long long)(c.TM - 1) * Dp + (unsigned long long)nt;
        c.span_cap = (int)span;
        c.L = (int)(span / Dp + 2);
        c.lds = (Dp * (unsigned long long)c.L + (unsigned long long)c.TM * c.RB) * item;
        *cfg = c;
        return GRHIP_OK;
    }
    return fail(GRHIP_EINVAL, "rational_resampler: a tile of 64 periods does not fit the LDS (%llu/%llu with %d taps "
                              "per filter: 63*D/gcd + taps per filter must stay below about %zu items)",
                (unsigned long long)I, (unsigned long long)D, nt, RS_LDS_MAX / item - 64 * 8);
}

int rs_prepare_device(RsKind kind)
{
    if (kind == RS_CCF) return prepare_kind<float2, float>();
    if (kind == RS_FFF) return prepare_kind<float, float>();
    return prepare_kind<float2, float2>();
}

int rs_launch(RsKind kind, bool generic, const RsLaunch &a, hipStream_t st)
{
    if (a.nout <= 0 || a.n_streams <= 0) return GRHIP_OK;
    RsConfig c;
    const long long nper = (a.nout + a.P - 1) / a.P;
    int rc = rs_config(kind, generic, a.I, a.D, a.nt, nper, &c);
    if (rc) return rc;
    if (kind == RS_CCF) return launch_kind<float2, float>(generic, a, c, st);
    if (kind == RS_FFF) return launch_kind<float, float>(generic, a, c, st);
    return launch_kind<float2, float2>(generic, a, c, st);
}

}  // namespace grhip
