// cpm.h -- host arithmetic of the continuous-phase transmitter: the tap designers gr_cpm::phase_response
// (general/gr_cpm.cc:43-218), gr_firdes::gaussian (general/gr_firdes.cc:571-594) and the taps of gmsk_mod
// (gr-digital/python/gmsk.py:99-107), statement for statement in the reference's types, and the layout of an
// interpolator's taps as the fused modulator reads them.  No device code: host/cpm_taps_test.cc runs it under the
// sanitizers.  Not part of the ABI.
//
// boost::math::erf of gr_cpm.cc:178-179 is std::erf here.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <vector>

namespace grhip {

enum CpmType { CPM_LRC = 0, CPM_LSRC = 1, CPM_LREC = 2, CPM_TFM = 3, CPM_GAUSSIAN = 4 };       // gr_cpm.h:31-38

constexpr unsigned CPM_MAX_TAPS = 4096;
constexpr double CPM_PI = 3.14159265358979323846, CPM_TWOPI = 2 * CPM_PI, CPM_PI_4 = 0.78539816339744830962;

inline bool cpm_type_valid(int type) { return type >= CPM_LRC && type <= CPM_GAUSSIAN; }

// the taps a call designs, or 0 where it is refused: sps * L == 0, more than CPM_MAX_TAPS taps, a non-finite beta.
// A type outside the enum gives LREC with L = 1 (gr_cpm.cc:214).
inline unsigned cpm_phase_response_ntaps(int type, unsigned sps, unsigned L, double beta)
{
    if (!cpm_type_valid(type)) L = 1;
    const unsigned long long n = (unsigned long long)sps * L;
    return (n == 0 || n > CPM_MAX_TAPS || !std::isfinite(beta)) ? 0u : (unsigned)n;
}

inline double cpm_sinc(double x)                                        // gr_cpm.cc:43-51
{
    if (x == 0) return 1.0;
    return sin(CPM_PI * x) / (CPM_PI * x);
}

inline double cpm_tfm_g0(double k, double sps)                          // gr_cpm.cc:117-127
{
    if (fabs(k) < 2 * DBL_EPSILON) return 1.145393004159143;
    const double pi2_24 = 0.411233516712057;
    double f = CPM_PI * k / sps;
    return cpm_sinc(k / sps) - pi2_24 * (2 * sin(f) - 2 * f * cos(f) - f * f * sin(f)) / (f * f * f);
}

// gr_cpm::phase_response; false where cpm_phase_response_ntaps gives 0
inline bool cpm_phase_response(int type, unsigned samples_per_sym, unsigned L, double beta, std::vector<float> &taps)
{
    const unsigned n = cpm_phase_response_ntaps(type, samples_per_sym, L, beta);
    if (!n) return false;
    if (!cpm_type_valid(type)) { type = CPM_LREC; L = 1; }
    const double Ls = (double)L * samples_per_sym;
    std::vector<double> taps_d(n, 0.0);
    switch (type) {
    case CPM_LRC:                                                       // :55-64
        taps.assign(n, (float)(1.0 / L / samples_per_sym));
        for (unsigned i = 0; i < n; i++) taps[i] = (float)(taps[i] * (1 - cos(CPM_TWOPI * i / L / samples_per_sym)));
        break;
    case CPM_LSRC: {                                                    // :72-101
        taps.assign(n, 0.0f);
        double sum = 0;
        for (unsigned i = 0; i < n; i++) {
            double k = i - Ls / 2;
            taps_d[i] = 1.0 / Ls * cpm_sinc(2.0 * k / Ls);
            if (fabs(fabs(k) - Ls / 4 / beta) < 2 * DBL_EPSILON) {
                taps_d[i] *= CPM_PI_4;
            } else {
                double tmp = 4.0 * beta * k / Ls;
                taps_d[i] *= cos(beta * CPM_TWOPI * k / Ls) / (1 - tmp * tmp);
            }
            sum += taps_d[i];
        }
        for (unsigned i = 0; i < n; i++) taps[i] = (float)((float)taps_d[i] / sum);         // (float) binds first, :98
        break;
    }
    case CPM_LREC:                                                      // :105-109
        taps.assign(n, (float)(1.0 / L / samples_per_sym));
        break;
    case CPM_TFM: {                                                     // :137-157
        taps.assign(n, 0.0f);
        const unsigned sps = samples_per_sym, causal_shift = sps * L / 2;
        double sum = 0;
        for (unsigned i = 0; i < n; i++) {
            double k = (double)(((int)i) - ((int)causal_shift));
            taps_d[i] = cpm_tfm_g0(k - sps, sps) + 2 * cpm_tfm_g0(k, sps) + cpm_tfm_g0(k + sps, sps);
            sum += taps_d[i];
        }
        for (unsigned i = 0; i < n; i++) taps[i] = (float)((float)taps_d[i] / sum);
        break;
    }
    default: {                                                          // CPM_GAUSSIAN, :171-189
        taps.assign(n, 0.0f);
        double alpha = 5.336446256636997 * beta;
        for (unsigned i = 0; i < n; i++) {
            double k = i - Ls / 2;
            taps_d[i] = (std::erf(alpha * (k / samples_per_sym + 0.5)) - std::erf(alpha * (k / samples_per_sym - 0.5))) * 0.5 / samples_per_sym;
            taps[i] = (float)taps_d[i];
        }
        break;
    }
    }
    return true;
}

// gr_firdes::gaussian; false for ntaps outside 1 .. CPM_MAX_TAPS or a non-finite argument
inline bool firdes_gaussian(double gain, double spb, double bt, int ntaps, std::vector<float> &taps)
{
    if (ntaps < 1 || (unsigned)ntaps > CPM_MAX_TAPS || !std::isfinite(gain) || !std::isfinite(spb) || !std::isfinite(bt)) return false;
    taps.assign((size_t)ntaps, 0.0f);
    double scale = 0;
    double dt = 1.0 / spb;
    double s = 1.0 / (sqrt(log(2.0)) / (2 * CPM_PI * bt));
    double t0 = -0.5 * ntaps;
    double ts;
    for (int i = 0; i < ntaps; i++) {
        t0++;
        ts = s * dt * t0;
        taps[i] = (float)exp(-0.5 * ts * ts);
        scale += taps[i];
    }
    for (int i = 0; i < ntaps; i++) taps[i] = (float)(taps[i] / scale * gain);
    return true;
}

constexpr unsigned GMSK_MAX_SPS = (CPM_MAX_TAPS + 1) / 5;               // 5 sps - 1 taps

// gmsk.py:99-107: firdes.gaussian(1, sps, bt, 4 sps) convolved in double with sps ones, then handed to
// interp_fir_filter_fff as floats; false for sps outside 2 .. GMSK_MAX_SPS (:87-88 raises below 2) or a non-finite bt
inline bool gmsk_mod_taps(unsigned sps, double bt, std::vector<float> &taps)
{
    if (sps < 2 || sps > GMSK_MAX_SPS) return false;
    std::vector<float> g;
    if (!firdes_gaussian(1, (double)sps, bt, (int)(4 * sps), g)) return false;
    const size_t n = g.size() + sps - 1;
    taps.assign(n, 0.0f);
    for (size_t o = 0; o < n; ++o) {
        double acc = 0;
        for (size_t k = o + 1 > sps ? o + 1 - sps : 0; k <= o && k < g.size(); ++k) acc += (double)g[k];
        taps[o] = (float)acc;
    }
    return true;
}

// ---- an interpolator's taps as the fused modulator reads them -------------------------------------------------------------
// gr_interp_fir_filter_fff pads zeros in FRONT up to a multiple of I (filter/gr_interp_fir_filter_XXX.cc.t:77-83) and
// gives filter f the taps padded[f + k I] (:99-100), which gr_fir_fff stores reversed.  rows[f * nt + k] is what
// gr_fir_fff_generic::filter multiplies with in[k]: padded[f + (nt - 1 - k) I].
inline unsigned cpm_taps_per_filter(size_t ntaps, unsigned I) { return (unsigned)((ntaps + I - 1) / I); }

inline std::vector<float> cpm_filter_rows(const std::vector<float> &taps, unsigned I)
{
    const unsigned nt = cpm_taps_per_filter(taps.size(), I);
    std::vector<float> padded((size_t)nt * I - taps.size(), 0.0f);
    padded.insert(padded.end(), taps.begin(), taps.end());
    std::vector<float> rows((size_t)nt * I);
    for (unsigned f = 0; f < I; ++f)
        for (unsigned k = 0; k < nt; ++k) rows[(size_t)f * nt + k] = padded[f + (size_t)(nt - 1 - k) * I];
    return rows;
}

// engine 1 of the hier handles keeps the rows in LDS and walks nt products per output
constexpr unsigned CPM_FUSED_MAX_NT = 16, CPM_FUSED_MAX_ROWS = 1024;
inline bool cpm_fused_fits(unsigned sps, unsigned nt) { return nt >= 1 && nt <= CPM_FUSED_MAX_NT && (unsigned long long)sps * nt <= CPM_FUSED_MAX_ROWS; }

}  // namespace grhip
