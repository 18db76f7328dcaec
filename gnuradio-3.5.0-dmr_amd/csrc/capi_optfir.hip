// capi_optfir.hip -- C ABI of gr_remez (general/gr_remez.cc:791-867) and of optfir.low_pass / high_pass / band_pass /
// band_reject (gnuradio/optfir.py:45-78, :116-156): host arithmetic only, no device is touched.  The arithmetic is
// remez.h's; this file checks the pointers, answers the size query and records the error text.
#include <cstring>

#include "grhip_internal.h"
#include "remez.h"

using namespace grhip;

namespace {

// the size query of grhip_firdes_low_pass: *ntaps always, the taps where they fit
template <class Design>
int deliver(const char *who, size_t need, double *out, size_t cap, size_t *ntaps, Design &&design)
{
    *ntaps = need;
    if (cap < need || !out) return fail(GRHIP_ERANGE, "%s: %zu taps, room for %zu", who, need, out ? cap : (size_t)0);
    std::vector<double> taps;
    const char *msg = "";
    const int rc = design(taps, &msg);
    if (rc) return fail(rc, "%s", msg);
    memcpy(out, taps.data(), taps.size() * sizeof(double));
    return GRHIP_OK;
}

int optfir(const char *who, int kind, double gain, double fs, const double *f, double ripple, double atten, int nextra, double *out,
           size_t cap, size_t *ntaps)
{
    if (!ntaps) return fail(GRHIP_EINVAL, "null argument");
    OptfirSpec s;
    const char *msg = "";
    int rc = optfir_spec(kind, gain, fs, f, ripple, atten, nextra, s, &msg);
    if (rc) return fail(rc, "%s", msg);
    if (s.order < 3) return fail(GRHIP_EINVAL, "gr_remez: number of taps must be >= 3");
    if (s.order > REMEZ_MAX_TAPS - 1) return fail(GRHIP_ERANGE, "%s: %d taps, at most %d", who, s.order + 1, REMEZ_MAX_TAPS);
    return deliver(who, (size_t)s.order + 1, out, cap, ntaps, [&](std::vector<double> &taps, const char **m) {
        return remez_design(s.order, s.bands.data(), s.bands.size(), s.ampl.data(), s.ampl.size(), s.weight.data(), s.weight.size(),
                            REMEZ_BANDPASS, 16, taps, m);
    });
}

}  // namespace

extern "C" {

int grhip_remez(int order, const double *bands, size_t nbands2, const double *ampl, const double *weight, size_t nweight,
                int filter_type, int grid_density, double *out, size_t cap, size_t *ntaps)
{
    if (!ntaps) return fail(GRHIP_EINVAL, "null argument");
    const char *msg = "";
    if (int rc = remez_check(order, bands, nbands2, ampl, nbands2, weight, nweight, filter_type, grid_density, &msg)) return fail(rc, "%s", msg);
    return deliver("gr_remez", (size_t)order + 1, out, cap, ntaps, [&](std::vector<double> &taps, const char **m) {
        return remez_design(order, bands, nbands2, ampl, nbands2, weight, nweight, filter_type, grid_density, taps, m);
    });
}

int grhip_optfir_low_pass(double gain, double fs, double freq1, double freq2, double passband_ripple_db, double stopband_atten_db,
                          int nextra_taps, double *out, size_t cap, size_t *ntaps)
{
    const double f[2] = {freq1, freq2};
    return optfir("optfir_low_pass", OPTFIR_LOW_PASS, gain, fs, f, passband_ripple_db, stopband_atten_db, nextra_taps, out, cap, ntaps);
}

int grhip_optfir_high_pass(double gain, double fs, double freq1, double freq2, double passband_ripple_db, double stopband_atten_db,
                           int nextra_taps, double *out, size_t cap, size_t *ntaps)
{
    const double f[2] = {freq1, freq2};
    return optfir("optfir_high_pass", OPTFIR_HIGH_PASS, gain, fs, f, passband_ripple_db, stopband_atten_db, nextra_taps, out, cap, ntaps);
}

int grhip_optfir_band_pass(double gain, double fs, double freq_sb1, double freq_pb1, double freq_pb2, double freq_sb2,
                           double passband_ripple_db, double stopband_atten_db, int nextra_taps, double *out, size_t cap, size_t *ntaps)
{
    const double f[4] = {freq_sb1, freq_pb1, freq_pb2, freq_sb2};
    return optfir("optfir_band_pass", OPTFIR_BAND_PASS, gain, fs, f, passband_ripple_db, stopband_atten_db, nextra_taps, out, cap, ntaps);
}

int grhip_optfir_band_reject(double gain, double fs, double freq_pb1, double freq_sb1, double freq_sb2, double freq_pb2,
                             double passband_ripple_db, double stopband_atten_db, int nextra_taps, double *out, size_t cap,
                             size_t *ntaps)
{
    const double f[4] = {freq_pb1, freq_sb1, freq_sb2, freq_pb2};
    return optfir("optfir_band_reject", OPTFIR_BAND_REJECT, gain, fs, f, passband_ripple_db, stopband_atten_db, nextra_taps, out, cap,
                  ntaps);
}

int grhip_optfir_spec(int kind, double gain, double fs, const double *freqs, size_t nfreqs, double passband_ripple_db,
                      double stopband_atten_db, int nextra_taps, int *order, double *bands, double *ampl, double *weight,
                      size_t *nbands)
{
    if (!freqs || !order || !bands || !ampl || !weight || !nbands) return fail(GRHIP_EINVAL, "null argument");
    if (kind < OPTFIR_LOW_PASS || kind > OPTFIR_BAND_REJECT) return fail(GRHIP_EINVAL, "optfir: unknown designer %d", kind);
    if (nfreqs != (size_t)(kind <= OPTFIR_HIGH_PASS ? 2 : 4)) return fail(GRHIP_EINVAL, "optfir: two band edges, or four for two transitions");
    OptfirSpec s;
    const char *msg = "";
    const int rc = optfir_spec(kind, gain, fs, freqs, passband_ripple_db, stopband_atten_db, nextra_taps, s, &msg);
    if (rc) return fail(rc, "%s", msg);
    *order = s.order;
    *nbands = s.weight.size();
    memcpy(bands, s.bands.data(), s.bands.size() * sizeof(double));
    memcpy(ampl, s.ampl.data(), s.ampl.size() * sizeof(double));
    memcpy(weight, s.weight.data(), s.weight.size() * sizeof(double));
    return GRHIP_OK;
}

}  // extern "C"
