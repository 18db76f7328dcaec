// analytic.h -- launchers of the real -> complex blocks (internal): gr_hilbert_fc / gr_filter_delay_fc and
// gr_goertzel_fc.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace grhip {

constexpr int AN_THREADS = 256;                 // lanes per workgroup of the tile kernels
constexpr int AN_R = 8;                         // consecutive outputs per lane
constexpr int AN_NT = AN_THREADS * AN_R;        // outputs per tile
constexpr int AN_FAST_MAX_TAPS = 2048;          // longer filters run the generic-order kernel in every mode
constexpr int AN_MAX_TAPS = 16384;              // the generic-order kernel keeps the taps in LDS

// out[n] = (in0[n + delay], sum_k taps_rev[k] in1[n + k]), n < n_out.  in1 has n_out + ntaps - 1 readable items, in0
// n_out + delay; both only 4-byte aligned.  in1 == in0 for the one-input form.
struct AnalyticLaunch {
    const float *in0, *in1;
    float2 *out;
    long long n_out;
    const float *taps_rev;      // device, d_taps order (reversed forward taps), ntaps floats
    const float *odd;           // device, sparse form only: forward taps h + 1, h + 3, ... (h = ntaps / 2), nodd floats
    int ntaps, delay, nodd;
};
enum { AN_GENERIC = 0, AN_DENSE = 1, AN_SPARSE = 2 };   // AN_SPARSE: in1 == in0, odd != null
int analytic_launch(int form, const AnalyticLaunch &a, hipStream_t st);

constexpr int GZ_ROWS = 64;                     // blocks per workgroup of the generic kernel: one lane each
constexpr int GZ_CH = 64;                       // samples of a block staged per pass
constexpr int GZ_WG_LEN = 2048;                 // FAST: from this block length a whole workgroup shares a block

// GENERIC: gri_goertzel::batch per block, bit-exact.  FAST: the closed form against tab[n] =
// (cos((len - n) w') / len, wi U_(len-1-n) / len), len entries built in double by the host.
// gri_goertzel::gri_setparms (gri_goertzel.cc:41-52): w in double, stored to float; cos and sin in float
inline void goertzel_setparms(int rate, float freq, float *wr, float *wi)
{
    const float w = 2.0 * M_PI * freq / rate;
    *wr = 2.0 * cosf(w);
    *wi = sinf(w);
}

// the FAST table of one tone, len entries, in double and rounded once (goertzel_fc; three of them for ctcss_squelch_ff)
inline void goertzel_build_table(int len, float wr, float wi, float2 *tab)
{
    double c = 0.5 * (double)wr;
    c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
    const double wp = acos(c), s = sin(wp), inv = 1.0 / (double)len;
    const bool flat = !(fabs(s) > 1e-300);                      // wr = +-2: U_k = (k + 1) (+-1)^k
    for (int n = 0; n < len; ++n) {
        const int k = len - 1 - n;
        const double u = flat ? (double)(k + 1) * ((c < 0 && (k & 1)) ? -1.0 : 1.0) : sin((double)(k + 1) * wp) / s;
        tab[n] = make_float2((float)(cos((double)(len - n) * wp) * inv), (float)((double)wi * u * inv));
    }
}

int goertzel_launch_generic(const float *in, float2 *out, long long nblocks, int len, float wr, float wi, hipStream_t st);
int goertzel_launch_fast(const float *in, float2 *out, long long nblocks, int len, const float2 *tab, hipStream_t st);

}  // namespace grhip
