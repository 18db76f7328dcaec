// pfb_clock_sync.h -- the arithmetic of gr_pfb_clock_sync_ccf (gnuradio-core/src/lib/filter/gr_pfb_clock_sync_ccf.cc;
// the line numbers below are that file's) in the reference's types: the arm partition, create_diff_taps, update_gains
// and one symbol's scalar step.  Host arithmetic only: no HIP, so host/pfb_clock_sync_test.cc runs it under the
// sanitizers and grhip_pfb_clock_sync_taps needs no device.  The functions marked PCS_HD are the loop's scalar chain
// itself; under hipcc they are also device functions, so the kernel of pfb_clock_sync.hip walks with the same text.
//
// The stream (include/grhip.h states the contract): xz is tpf + isps - 1 zeros followed by the input, `pos` an absolute
// index into xz; an evaluation at `pos` reads xz[pos .. pos + tpf - 1].
//
// Deviations, each counted in `slips`:
//   * backward: after its wraps an evaluation may not stand before `lo`, one item behind the position at which the
//     symbol before took its derivative arm (and never before 0); it is put at `lo`;
//   * forward: at most PCS_CARRY forward carries move `pos` per evaluation; k is wrapped fully;
//   * the wrap loops run PCS_WRAP_TRIPS trips at the most and only for |k| < 2^29; beyond that k becomes the exact
//     double remainder fmod(k, nfilters) (no slip by itself: the carries it stands for are then cut as above); a k
//     that is not finite becomes 0.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#ifdef __HIPCC__
#define PCS_HD __host__ __device__ inline
#else
#define PCS_HD inline
#endif

namespace grhip {

constexpr int PCS_CARRY = 8;                // forward carries that move the position, per evaluation
constexpr int PCS_WRAP_TRIPS = 64;          // trips of the reference's two wrap loops together, per evaluation
constexpr int PCS_MAX_FILTERS = 256;        // arms
constexpr int PCS_MAX_TPF = 256;            // taps per arm
constexpr int PCS_MAX_BANK = 4096;          // arms * taps per arm (one bank's floats in LDS)
constexpr int PCS_MAX_OSPS = 8;
constexpr int PCS_MAX_SPS = 256;            // sps below this

struct PcsState {
    float k, rate_f, error;                 // d_k, d_rate_f, d_error
    int slips;
    long long pos;                          // where the next symbol starts, an index into xz
};

struct PcsParams {
    float alpha, beta, max_dev, rate_i;     // d_rate_i is a float holding an integer (:79, gr_pfb_clock_sync_ccf.h:168)
    int nfilters, tpf, isps, osps;
};

// items of xz behind a symbol's start that have to be there before it starts
PCS_HD int pcs_need(int tpf, int osps) { return osps * PCS_CARRY + osps + tpf; }
// items of xz a stream keeps from call to call: what a later symbol may still read
PCS_HD int pcs_hist(int tpf, int isps, int osps) { return pcs_need(tpf, osps) + isps; }

// :381-395 for one evaluation: the arm, with k wrapped and pos carried.  `trips` counts the wrap loops' trips.
PCS_HD int pcs_wrap(float &k, long long &pos, long long lo, int nf, int &slips, int &trips)
{
    if (!(k - k == 0.f)) {                  // not finite
        k = 0.f;
        ++slips;
    }
    long long carry = 0;
    int fn = 0;
    bool far = true;
    if (fabsf(k) < 536870912.f) {           // 2^29: floor(k) is an int, and so is every fn below
        fn = (int)floorf(k);                // :381
        int t = 0;
        for (; fn >= nf && t < PCS_WRAP_TRIPS; ++t) {           // :386-390
            k = k - (float)nf;
            fn -= nf;
            ++carry;
        }
        for (; fn < 0 && t < PCS_WRAP_TRIPS; ++t) {             // :391-395
            k = k + (float)nf;
            fn += nf;
            --carry;
        }
        trips += t;
        far = fn >= nf || fn < 0;
    }
    if (far) {
        // what the loops would leave had they run on: the remainder is exact in double, and so is a float again
        // (a multiple of ulp(k) below nfilters)
        double r = fmod((double)k, (double)nf);
        if (r < 0) r += (double)nf;
        double c = ((double)k - r) / (double)nf;
        if (c > 1e12) c = 1e12;
        if (c < -1e12) c = -1e12;
        carry += (long long)c;
        fn = (int)r;
        if (fn > nf - 1) fn = nf - 1;
        k = (float)r;
    }
    if (carry > PCS_CARRY) {
        carry = PCS_CARRY;
        ++slips;
    }
    pos += carry;
    if (pos < lo) {
        pos = lo;
        ++slips;
    }
    return fn;
}

// gr_branchless_clip (general/gr_math.h:63-69)
PCS_HD float pcs_clip(float x, float clip)
{
    float x1 = fabsf(x + clip);
    float x2 = fabsf(x - clip);
    x1 -= x2;
    return (float)(0.5 * (double)x1);
}

// :398, the phase advance behind an evaluation
PCS_HD float pcs_advance(float k, float rate_i, float rate_f) { return (k + rate_i) + rate_f; }

// :409-419 behind a symbol: the error from the first output and the derivative arm's, the loop's step and the clip
PCS_HD void pcs_step(PcsState &s, const PcsParams &p, float out_re, float out_im, float diff_re, float diff_im)
{
    const float error_r = out_re * diff_re;
    const float error_i = out_im * diff_im;
    s.error = (float)((double)(error_i + error_r) / 2.0);
    s.rate_f = s.rate_f + p.beta * s.error;
    s.k = s.k + p.alpha * s.error;
    s.rate_f = pcs_clip(s.rate_f, p.max_dev);
}

// ---- host only -------------------------------------------------------------------------------------------------------

// update_gains (:200-205): the denominator is formed in double and narrowed, the numerators in float
inline void pcs_gains(float damping, float loop_bw, float &alpha, float &beta)
{
    const float denom = (float)(1.0 + 2.0 * damping * loop_bw + loop_bw * loop_bw);
    alpha = (4 * damping * loop_bw) / denom;
    beta = (4 * loop_bw * loop_bw) / denom;
}

// create_diff_taps (:250-274): pwr gathers |the partial sums|, and the taps are multiplied by it
inline void pcs_diff_taps(const float *taps, size_t ntaps, std::vector<float> &diff)
{
    const float diff_filter[3] = {-1, 0, 1};
    float pwr = 0;
    diff.clear();
    diff.push_back(0);
    for (size_t i = 0; i + 2 < ntaps; ++i) {
        float tap = 0;
        for (int j = 0; j < 3; ++j) {
            tap += diff_filter[j] * taps[i + j];
            pwr += fabsf(tap);
        }
        diff.push_back(tap);
    }
    diff.push_back(0);
    for (float &d : diff) d *= pwr;
}

inline int pcs_tpf(size_t ntaps, int nfilters) { return (int)((ntaps + (size_t)nfilters - 1) / (size_t)nfilters); }

// set_taps (:208-248): arm f's tap j is taps[f + j * nfilters], zeros beyond the prototype; bank[f * tpf + j]
inline void pcs_partition(const float *taps, size_t ntaps, int nfilters, int tpf, float *bank)
{
    for (int f = 0; f < nfilters; ++f)
        for (int j = 0; j < tpf; ++j) {
            const size_t i = (size_t)f + (size_t)j * (size_t)nfilters;
            bank[(size_t)f * tpf + j] = i < ntaps ? taps[i] : 0.f;
        }
}

// null, or why the prototype and the arm count are refused
inline const char *pcs_check_taps(const float *taps, long long ntaps, long long nfilters)
{
    if (!taps) return "pfb_clock_sync_ccf: null taps";
    if (ntaps < 2) return "pfb_clock_sync_ccf: at least 2 taps (create_diff_taps indexes with size() - 2)";
    if (nfilters < 1 || nfilters > PCS_MAX_FILTERS) return "pfb_clock_sync_ccf: filter_size 1 .. 256";
    const long long tpf = (ntaps + nfilters - 1) / nfilters;
    if (tpf > PCS_MAX_TPF || tpf * nfilters > PCS_MAX_BANK) return "pfb_clock_sync_ccf: at most 256 taps per arm and 4096 in a bank";
    for (long long i = 0; i < ntaps; ++i)
        if (!std::isfinite(taps[i])) return "pfb_clock_sync_ccf: taps must be finite";
    return nullptr;
}

// both banks, nfilters * tpf floats each; null, or why not
inline const char *pcs_design(const float *taps, long long ntaps, long long nfilters, std::vector<float> &bank, std::vector<float> &dbank,
                              int &tpf)
{
    if (const char *e = pcs_check_taps(taps, ntaps, nfilters)) return e;
    std::vector<float> diff;
    pcs_diff_taps(taps, (size_t)ntaps, diff);
    for (float d : diff)
        if (!std::isfinite(d)) return "pfb_clock_sync_ccf: the derivative taps are not finite";
    const int t = pcs_tpf((size_t)ntaps, (int)nfilters);
    std::vector<float> b((size_t)nfilters * t), d((size_t)nfilters * t);
    pcs_partition(taps, (size_t)ntaps, (int)nfilters, t, b.data());
    pcs_partition(diff.data(), diff.size(), (int)nfilters, t, d.data());
    bank.swap(b);
    dbank.swap(d);
    tpf = t;
    return nullptr;
}

// null, or why the constructor's other arguments are refused
inline const char *pcs_check_args(double sps, float loop_bw, float init_phase, float max_dev, int osps)
{
    if (!std::isfinite(sps) || !std::isfinite(loop_bw) || !std::isfinite(init_phase) || !std::isfinite(max_dev))
        return "pfb_clock_sync_ccf: arguments must be finite";
    if (sps < 1 || sps >= PCS_MAX_SPS) return "pfb_clock_sync_ccf: sps in [1, 256)";
    if (osps < 1 || osps > PCS_MAX_OSPS) return "pfb_clock_sync_ccf: osps 1 .. 8";
    if (loop_bw < 0) return "gr_pfb_clock_sync_cc: invalid bandwidth. Must be >= 0.";
    return nullptr;
}

// the loop's host side: the gains and their setters with the reference's checks (:121-159)
struct PcsLoop {
    float loop_bw = 0, damping = 0, alpha = 0, beta = 0, max_dev = 0;

    static bool unit(float v) { return v >= 0 && v <= 1.0f; }       // false for a NaN
    bool try_gains(float df, float bw)
    {
        float a, b;
        pcs_gains(df, bw, a, b);
        if (!std::isfinite(a) || !std::isfinite(b)) return false;   // a stated deviation
        damping = df; loop_bw = bw; alpha = a; beta = b;
        return true;
    }
    bool set_loop_bandwidth(float bw) { return bw >= 0 && std::isfinite(bw) && try_gains(damping, bw); }
    bool set_damping_factor(float df) { return unit(df) && try_gains(df, loop_bw); }
    bool set_alpha(float a) { return unit(a) ? (alpha = a, true) : false; }
    bool set_beta(float b) { return unit(b) ? (beta = b, true) : false; }
    bool set_max_dev(float m) { return std::isfinite(m) ? (max_dev = m, true) : false; }
    bool init(float bw, float md)
    {
        damping = sqrtf(2.0f) / 2.0f;                               // :69
        return set_max_dev(md) && set_loop_bandwidth(bw);
    }
};

// the constructor's split of the rate (:78-80); d_rate is a float
inline void pcs_rate(double sps, int nfilters, float &rate_i, float &rate_f)
{
    const float rate = (float)((sps - floor(sps)) * (double)nfilters);
    rate_i = (float)(int)floor(rate);
    rate_f = rate - rate_i;
}

}  // namespace grhip
