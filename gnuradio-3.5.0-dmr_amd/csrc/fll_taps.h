// fll_taps.h -- two filter designers in the reference's types: gr_firdes::root_raised_cosine (general/gr_firdes.cc:601-650)
// and digital_fll_band_edge_cc::design_filter (gr-digital/lib/digital_fll_band_edge_cc.cc:34-40, :148-188).
// Host arithmetic only: no HIP, so host/fll_taps_test.cc runs it under the sanitizers.
//
// Each returns 0, or a message where the design is refused and writes nothing then.
#pragma once
#ifndef _GNU_SOURCE
#define _GNU_SOURCE             // sincosf
#endif
#include <cmath>
#include <complex>
#include <vector>

namespace grhip {

constexpr int FLL_MAX_TAPS = 1024;              // filter_size of fll_band_edge_cc (a stated deviation)
constexpr int RRC_MAX_TAPS = 1 << 24;           // as firdes_low_pass
constexpr float FLL_FREQ_CAP = 1024.0f;         // CL_FREQ_CAP of control_loop.h

// gr_firdes.cc:601-650, statement for statement.  ntaps is made odd first, as the reference does.
inline const char *rrc_design(double gain, double sampling_freq, double symbol_rate, double alpha, int ntaps, std::vector<float> &taps)
{
    if (!std::isfinite(gain) || !std::isfinite(sampling_freq) || !std::isfinite(symbol_rate) || !std::isfinite(alpha))
        return "firdes_root_raised_cosine: an argument is not finite";
    if (ntaps < 1) return "firdes_root_raised_cosine: ntaps must be at least 1";
    if (ntaps >= RRC_MAX_TAPS) return "firdes_root_raised_cosine: too many taps";
    ntaps |= 1;                                                 // :608
    const double spb = sampling_freq / symbol_rate;             // :610
    taps.assign((size_t)ntaps, 0.f);
    double scale = 0;
    for (int i = 0; i < ntaps; i++) {
        double x1, x2, x3, num, den;
        const double xindx = i - ntaps / 2;
        x1 = M_PI * xindx / spb;
        x2 = 4 * alpha * xindx / spb;
        x3 = x2 * x2 - 1;
        if (fabs(x3) >= 0.000001) {                             // :620
            if (i != ntaps / 2) num = cos((1 + alpha) * x1) + sin((1 - alpha) * x1) / (4 * alpha * xindx / spb);
            else num = cos((1 + alpha) * x1) + (1 - alpha) * M_PI / (4 * alpha);
            den = x3 * M_PI;
        } else {
            if (alpha == 1) {                                   // :630-634: the tap is -1 and stays out of the scale
                taps[i] = -1;
                continue;
            }
            x3 = (1 - alpha) * x1;
            x2 = (1 + alpha) * x1;
            num = (sin(x2) * (1 + alpha) * M_PI - cos(x3) * ((1 - alpha) * M_PI * spb) / (4 * alpha * xindx) +
                   sin(x3) * spb * spb / (4 * alpha * xindx * xindx));
            den = -32 * M_PI * alpha * alpha * xindx / spb;
        }
        taps[i] = 4 * alpha * num / den;                        // :642
        scale += taps[i];
    }
    for (int i = 0; i < ntaps; i++) taps[i] = taps[i] * gain / scale;   // :646-647
    return nullptr;
}

// digital_fll_band_edge_cc.cc:34-40
inline float fll_sinc(float x)
{
    if (x == 0) return 1;
    return sin(M_PI * x) / (M_PI * x);
}

// gr_expj (general/gr_expj.h): sincosf, as a Linux build of the reference calls it
inline std::complex<float> fll_expj(float phase)
{
    float t_imag, t_real;
    sincosf(phase, &t_imag, &t_real);
    return std::complex<float>(t_real, t_imag);
}

// the loop's frequency limit, :58: M_TWOPI*(2.0/samps_per_sym) narrowed by gri_control_loop's float parameter
inline float fll_max_freq_of(float sps) { return (float)((2 * M_PI) * (2.0 / sps)); }

// what the reference's constructor and setters throw on (:62-77), and the deviations that bound the device walk
inline const char *fll_check(float sps, float rolloff, int filter_size)
{
    if (!(sps > 0)) return "digital_fll_band_edge_cc: invalid number of sps. Must be > 0.";
    if (!(rolloff >= 0 && rolloff <= 1.0)) return "digital_fll_band_edge_cc: invalid rolloff factor. Must be in [0,1].";
    if (filter_size <= 0) return "digital_fll_band_edge_cc: invalid filter size. Must be > 0.";
    if (filter_size > FLL_MAX_TAPS) return "fll_band_edge_cc: filter sizes above 1024 are not supported";
    if (!std::isfinite(sps) || !(fll_max_freq_of(sps) <= FLL_FREQ_CAP))
        return "fll_band_edge_cc: 2 pi 2 / sps must be finite and within 1024 rad/sample";
    return nullptr;
}

// :148-188.  lower and upper receive filter_size taps, stored reversed as the reference stores them.
inline const char *fll_design(float samps_per_sym, float rolloff, int filter_size, std::vector<std::complex<float>> &lower,
                              std::vector<std::complex<float>> &upper)
{
    if (const char *e = fll_check(samps_per_sym, rolloff, filter_size)) return e;
    const int M = rint(filter_size / samps_per_sym);            // :152
    float power = 0;
    std::vector<float> bb_taps;
    for (int i = 0; i < filter_size; i++) {
        float k = -M + i * 2.0 / samps_per_sym;                 // :158
        float tap = fll_sinc(rolloff * k - 0.5) + fll_sinc(rolloff * k + 0.5);
        power += tap;
        bb_taps.push_back(tap);
    }
    std::vector<std::complex<float>> lo((size_t)filter_size), up((size_t)filter_size);
    const int N = (bb_taps.size() - 1.0) / 2.0;                 // :171
    for (int i = 0; i < filter_size; i++) {
        float tap = bb_taps[i] / power;
        float k = (-N + (int)i) / (2.0 * samps_per_sym);        // :175
        std::complex<float> t1 = tap * fll_expj(-(2 * M_PI) * (1 + rolloff) * k);
        std::complex<float> t2 = tap * fll_expj((2 * M_PI) * (1 + rolloff) * k);
        if (!std::isfinite(t1.real()) || !std::isfinite(t1.imag()) || !std::isfinite(t2.real()) || !std::isfinite(t2.imag()))
            return "fll_band_edge_cc: the taps are not finite (the baseband taps sum to zero)";
        lo[filter_size - i - 1] = t1;
        up[filter_size - i - 1] = t2;
    }
    lower.swap(lo);
    upper.swap(up);
    return nullptr;
}

}  // namespace grhip
