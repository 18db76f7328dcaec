// spectrum.h -- launchers of the spectrum-estimate blocks (internal): gr_complex_to_mag_squared, gr_complex_to_mag,
// gr_single_pole_iir_filter_ff, gr_nlog10_ff and gr_keep_one_in_n.
#pragma once
#include <hip/hip_runtime.h>

#include "grhip_internal.h"

namespace grhip {

// FAST single_pole_iir: below IIR_FILL_LANES lanes (streams x vlen) the item axis is cut into chunks of IIR_CHUNK items.
// 65536 lanes are one wave on each of the 4 x 256 SIMDs: from there on the serial walk alone occupies the device.
constexpr int IIR_CHUNK = 256;
constexpr int IIR_FILL_LANES = 65536;

// out[i] = re * re + im * im: two rounded products, one rounded add (general/gr_complex_to_xxx.cc:180-203)
int mag_squared_launch(const float2 *in, float *out, long long n, hipStream_t st);

// out[i] = (float)sqrt((double)re * re + (double)im * im), mag_val of spectrum_math.h (the std::abs loop of
// general/gr_complex_to_xxx.cc)
int mag_launch(const float2 *in, float *out, long long n, hipStream_t st);

// out[i] = n * log10f(max(in[i], 1e-18f)) + k (general/gr_nlog10_ff.cc:60-61); in may be out
int nlog10_launch(const float *in, float *out, long long count, float n, float k, hipStream_t st);

// S streams of n_in items of item_size bytes back to back; item first + o * n of every stream becomes output item o
// (o < n_out); the outputs are S streams of n_out items back to back.
int keep_one_launch(const void *in, void *out, size_t item_size, long long n_in, long long n_out, long long first,
                    long long n, int nstreams, hipStream_t st);

// gr_keep_one_in_n.cc:80-90 in closed form.  count is the countdown before the call (1 .. n): the kept items are
// count - 1, count - 1 + n, ...
struct KeepOne {
    long long n = 1, count = 1;
    void set_n(long long v) { n = v < 1 ? 1 : v; count = n; }
    long long first() const { return count - 1; }
    long long produced(long long n_in) const { return n_in > first() ? (n_in - first() - 1) / n + 1 : 0; }
    void advance(long long n_in)
    {
        const long long p = produced(n_in);
        if (!p) count -= n_in;
        else count = n - (n_in - 1 - (first() + (p - 1) * n));
    }
};

// y = (float)(alpha * (double)x + (1.0 - alpha) * (double)y_prev) along the item axis of [S][n][vlen], one float of
// state per (stream, element) (filter/gr_single_pole_iir.h:87-97); in may be out.
struct IirLaunch {
    const float *in;
    float *out;
    long long n;            // items per stream
    int nstreams, vlen;
    double alpha;
    float *state;           // [S][vlen]
    // the outputs written as log_n * log10f(max(y, 1e-18f)) + log_k (gr_nlog10_ff.cc:60-61) instead of y; the state stays y
    bool log = false;
    float log_n = 1.f, log_k = 0.f;
};
// chunked: cut the item axis (FAST with few lanes); scratch then holds the chunks' end values and carries
bool iir_chunked(bool fast, const IirLaunch &a);
int single_pole_iir_launch(bool fast, const IirLaunch &a, DevBuf &scratch, hipStream_t st);

}  // namespace grhip
