// control_loop.h -- the loop parameters of gri_control_loop (general/gri_control_loop.{h,cc}) in the reference's types.
// Host arithmetic only: no HIP, so host/control_loop_test.cc runs it under the sanitizers.
//
// What lives here is what the reference's setters compute and check; phase and frequency are per stream and live on
// the device, so set_frequency and set_phase return the value to store.  A setter returns false where the reference
// throws std::out_of_range, and leaves the parameters as they were.
//
// Deviations, so that the device walk ends for every argument (include/grhip.h states them at the entries):
//   * limits_ok(): max_freq / min_freq that are not finite or above CL_FREQ_CAP in magnitude are refused;
//   * a bandwidth or damping factor whose gains (update_gains) come out not finite is refused: an infinite beta makes
//     the phase infinite, and the reference's phase_wrap then never ends;
//   * set_alpha / set_beta refuse a NaN (it passes the reference's two comparisons);
//   * phase_ok(): set_phase refuses values that are not finite or above CL_PHASE_CAP in magnitude.
#pragma once
#include <cmath>

namespace grhip {

constexpr float CL_FREQ_CAP = 1024.0f;          // rad/sample
constexpr float CL_PHASE_CAP = 1048576.0f;      // 2^20 rad
constexpr double CL_PI = 3.14159265358979323846;
constexpr double CL_TWOPI = 2.0f * CL_PI;       // gri_control_loop.cc:31 `#define M_TWOPI (2.0f*M_PI)`: a double

struct ControlLoop {
    float loop_bw = 0.f, damping = 0.f, alpha = 0.f, beta = 0.f, max_freq = 0.f, min_freq = 0.f;

    static bool limits_ok(float max_f, float min_f)
    {
        return std::isfinite(max_f) && std::isfinite(min_f) && std::fabs(max_f) <= CL_FREQ_CAP && std::fabs(min_f) <= CL_FREQ_CAP;
    }
    static bool phase_ok(float phase) { return std::isfinite(phase) && std::fabs(phase) <= CL_PHASE_CAP; }

    // gri_control_loop.cc:49-54: denom is a float formed from a double expression (d_loop_bw*d_loop_bw is a float
    // product inside it), alpha and beta are float expressions
    static void gains(float damp, float bw, float &a, float &b)
    {
        const float denom = (float)(1.0 + 2.0 * damp * bw + bw * bw);
        a = (4 * damp * bw) / denom;
        b = (4 * bw * bw) / denom;
    }

    bool try_gains(float damp, float bw)
    {
        float a, b;
        gains(damp, bw, a, b);
        if (!std::isfinite(a) || !std::isfinite(b)) return false;
        damping = damp; loop_bw = bw; alpha = a; beta = b;
        return true;
    }

    // gri_control_loop.cc:33-42: damping sqrtf(2.0f)/2.0f, then set_loop_bandwidth
    bool init(float bw, float max_f, float min_f)
    {
        if (!limits_ok(max_f, min_f)) return false;
        max_freq = max_f; min_freq = min_f;
        damping = sqrtf(2.0f) / 2.0f;
        return set_loop_bandwidth(bw);
    }

    bool set_loop_bandwidth(float bw)                   // :86-95
    {
        if (bw < 0) return false;
        return try_gains(damping, bw);
    }
    bool set_damping_factor(float df)                   // :97-106
    {
        if (df < 0 || df > 1.0) return false;
        return try_gains(df, loop_bw);
    }
    bool set_alpha(float a)                             // :108-115
    {
        if (a < 0 || a > 1.0 || a != a) return false;
        alpha = a;
        return true;
    }
    bool set_beta(float b)                              // :117-124
    {
        if (b < 0 || b > 1.0 || b != b) return false;
        beta = b;
        return true;
    }
    // :126-135: above the maximum gives the MINIMUM, below the minimum the MAXIMUM
    float set_frequency(float freq) const
    {
        if (freq > max_freq) return min_freq;
        if (freq < min_freq) return max_freq;
        return freq;
    }
    // :137-145; phase_ok(phase) bounds the trips by 2^20 / 2 pi
    static float set_phase(float phase)
    {
        while (phase > CL_TWOPI) phase = (float)(phase - CL_TWOPI);
        while (phase < -CL_TWOPI) phase = (float)(phase + CL_TWOPI);
        return phase;
    }
};

}  // namespace grhip
