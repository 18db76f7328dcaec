// logpwrfft_test -- the logpwrfft_c / logpwrfft_f blocks of grhip_blocks.h: that they report the item sizes and
// relative_rate of the reference's hier block, carry its setters and getters, throw what its preconditions throw, and,
// run under the stand-in executor (grhip_executor.h) on a stream of samples, produce bit for bit what the five C++
// blocks connected in a row (keep_one_in_n -> fft_vcc | fft_vfc -> complex_to_mag_squared -> single_pole_iir_filter_ff
// -> nlog10_ff) produce on the same stream as vectors (GRHIP_MODE_GENERIC: state and countdown carry across the
// executor's calls).  For tests/test_gpu_logpwrfft.py; no arguments.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <stdexcept>
#include <vector>

#include "grhip_blocks.h"
#include "grhip_executor.h"

static int properties()
{
    int fails = 0;
    try { gr_make_logpwrfft_c(1e6, 0, 2.0, 30, 0.2, true); fails++; } catch (const std::out_of_range &) {}
    try { gr_make_logpwrfft_f(1e6, 64, 2.0, 30, 1.5, true); fails++; } catch (const std::out_of_range &) {}
    try { gr_make_logpwrfft_c(1e6, 64, 0.0, 30, 0.2, true); fails++; } catch (const std::invalid_argument &) {}
    try { gr_make_logpwrfft_c(1e6, 1, 2.0, 30, 0.2, true); fails++; } catch (const std::invalid_argument &) {}
    grhip_logpwrfft_c_sptr c = gr_make_logpwrfft_c(10e6, 4096, 2.0, 30, 0.2, true);
    if (c->input_signature()->sizeof_stream_item(0) != sizeof(gr_complex) ||
        c->output_signature()->sizeof_stream_item(0) != 4096 * sizeof(float) || c->history() != 1) fails++;
    if (c->decimation() != 81 || c->relative_rate() != 1.0 / (4096.0 * 81) || c->sample_rate() != 10e6 ||
        c->frame_rate() != 10e6 / 4096 / 81 || !c->average() || c->avg_alpha() != 0.2) fails++;
    c->set_decimation(2.5);                                 // half away from zero
    if (c->decimation() != 3 || c->relative_rate() != 1.0 / (4096.0 * 3)) fails++;
    c->set_vec_rate(10e6 / 4096 / 7);
    if (c->decimation() != 7) fails++;
    c->set_sample_rate(20e6);
    if (c->decimation() != 14 || c->sample_rate() != 20e6) fails++;
    c->set_average(false);
    c->set_avg_alpha(0.5);
    if (c->average() || c->avg_alpha() != 0.5) fails++;
    try { c->set_avg_alpha(-0.1); fails++; } catch (const std::out_of_range &) {}
    grhip_logpwrfft_f_sptr f = gr_make_logpwrfft_f(1e6, 100, 0.5, 1e6 / 100, 1.0, false, std::vector<double>(100, 1.0));
    if (f->input_signature()->sizeof_stream_item(0) != sizeof(float) ||
        f->output_signature()->sizeof_stream_item(0) != 100 * sizeof(float) || f->decimation() != 1 || f->relative_rate() != 0.01) fails++;
    std::cout << "properties: " << (fails ? "FAIL" : "ok") << "\n";
    return fails;
}

static int same(const char *what, const std::vector<unsigned char> &y, const std::vector<unsigned char> &chain, size_t want_bytes)
{
    if (y.size() != want_bytes || y.size() != chain.size() || memcmp(y.data(), chain.data(), y.size())) {
        std::cout << what << ": the block's output differs from the five blocks' (" << y.size() << " vs " << chain.size()
                  << " bytes, " << want_bytes << " expected)\n";
        return 1;
    }
    std::cout << what << ": " << y.size() / sizeof(float) << " floats equal\n";
    return 0;
}

template <bool REAL>
static int against_the_five_blocks(int N, int F, int decim, double alpha, bool average, int chunk)
{
    typedef typename std::conditional<REAL, float, gr_complex>::type item_t;
    const size_t n = (size_t)N * F;
    unsigned lcg = 2463534242u + N;
    std::vector<item_t> x(n);
    for (size_t i = 0; i < n; ++i) {
        lcg = lcg * 1664525u + 1013904223u;
        const float re = (float)(lcg >> 8) / 8388608.f - 1.f;
        lcg = lcg * 1664525u + 1013904223u;
        const float im = (float)(lcg >> 8) / 8388608.f - 1.f;
        if constexpr (REAL) { x[i] = re + 0.25f * im; } else { x[i] = gr_complex(re, im); }
    }
    const double ref_scale = 2.0, frame_rate = 25.0, sample_rate = frame_rate * N * decim;
    // window and k as logpwrfft.py:52-62
    std::vector<double> wd(N);
    grhip_detail::check(grhip_window_blackmanharris(N, wd.data()));
    double window_power = 0.0;
    for (double v : wd) window_power += v * v;
    const double k = -20 * log10((double)N) - 10 * log10(window_power / N) - 20 * log10(ref_scale / 2);
    const std::vector<float> wf(wd.begin(), wd.end());

    std::vector<unsigned char> y, chain;
    {
        grhip_linear_flowgraph fg(chunk);
        gr_block_sptr b;
        if constexpr (REAL) {
            grhip_logpwrfft_f_sptr p = gr_make_logpwrfft_f(sample_rate, N, ref_scale, frame_rate, alpha, average);
            p->set_mode(GRHIP_MODE_GENERIC);
            if (p->decimation() != decim) return 1;
            b = p;
        } else {
            grhip_logpwrfft_c_sptr p = gr_make_logpwrfft_c(sample_rate, N, ref_scale, frame_rate, alpha, average);
            p->set_mode(GRHIP_MODE_GENERIC);
            if (p->decimation() != decim) return 1;
            b = p;
        }
        fg.connect(b);
        y = fg.run(x.data(), n);                            // items of one sample
    }
    {
        grhip_linear_flowgraph fg(chunk);
        grhip_keep_one_in_n_sptr keep = gr_make_keep_one_in_n((size_t)N * sizeof(item_t), decim);
        grhip_complex_to_mag_squared_sptr m = gr_make_complex_to_mag_squared(N);
        grhip_single_pole_iir_filter_ff_sptr f = gr_make_single_pole_iir_filter_ff(average ? alpha : 1.0, N);
        grhip_nlog10_ff_sptr l = gr_make_nlog10_ff(10, N, (float)k);
        m->set_mode(GRHIP_MODE_GENERIC); f->set_mode(GRHIP_MODE_GENERIC); l->set_mode(GRHIP_MODE_GENERIC);
        fg.connect(keep);
        if constexpr (REAL) fg.connect(grhip_make_fft_vfc(N, true, wf));
        else fg.connect(grhip_make_fft_vcc(N, true, wf));
        fg.connect(m); fg.connect(f); fg.connect(l);
        chain = fg.run(x.data(), F);                        // items of one frame (stream_to_vector's output)
    }
    char what[96];
    snprintf(what, sizeof what, "logpwrfft_%c N %d decimation %d averaging %s", REAL ? 'f' : 'c', N, decim, average ? "on" : "off");
    return same(what, y, chain, (size_t)(F / decim) * N * sizeof(float));
}

int main()
{
    try {
        int fails = properties();
        fails += against_the_five_blocks<false>(256, 200, 3, 0.2, true, 7);         // small calls: 7 output frames at most
        fails += against_the_five_blocks<true>(256, 200, 3, 0.2, true, 7);
        fails += against_the_five_blocks<false>(4096, 40, 2, 0.2, false, 3);
        fails += against_the_five_blocks<true>(100, 90, 1, 0.5, true, 50);          // composed path (Bluestein)
        return fails ? 1 : 0;
    } catch (const std::exception &e) {
        std::cerr << "logpwrfft_test: " << e.what() << "\n";
        return 1;
    }
}
