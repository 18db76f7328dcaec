// fm_demod_test -- the recursive-filter and FM-demodulator blocks of grhip_blocks.h: factory signatures, item sizes,
// history and relative rate, the host-only tap designers, and small flowgraphs under the stand-in executor
// (grhip_executor.h).  gr_make_iir_filter_ffd against a loop over gri_iir::filter restated here (filter/gri_iir.h:126-163),
// bit for bit, a latched set_taps included; gr_make_nbfm_rx as ONE block against the three blocks it stands for
// (quadrature_demod_cf -> fm_deemph -> fir_filter_fff) run one after the other under the same executor: bit for bit in
// GRHIP_MODE_GENERIC, within 1e-5 of the peak for the fused kernel.
// For tests/test_gpu_host_fm_demod.py; no arguments.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <stdexcept>
#include <vector>

#include "grhip_blocks.h"
#include "grhip_executor.h"

namespace {

// gri_iir<float, float, double>::filter over a whole vector
std::vector<float> iir_loop(const std::vector<double> &ff, const std::vector<double> &fb, const std::vector<float> &x)
{
    const size_t n = ff.size(), m = fb.size();
    std::vector<double> ys(m, 0.0);
    std::vector<float> xs(n, 0.f), y(x.size());
    for (size_t t = 0; t < x.size(); ++t) {
        volatile double acc = ff[0] * x[t];                     // volatile: every step rounds to double, whatever the compiler
        for (size_t i = 1; i < n; ++i) acc = acc + ff[i] * xs[i - 1];
        for (size_t i = 1; i < m; ++i) acc = acc + fb[i] * ys[i - 1];
        for (size_t i = n - 1; i > 0; --i) xs[i] = xs[i - 1];
        for (size_t i = m - 1; i > 0; --i) ys[i] = ys[i - 1];
        xs[0] = x[t];
        ys[0] = acc;
        y[t] = (float)acc;
    }
    return y;
}

std::vector<float> noise(int n)
{
    unsigned lcg = 2463534242u;
    std::vector<float> x(n);
    for (int i = 0; i < n; ++i) {
        lcg = lcg * 1664525u + 1013904223u;
        const float level = i < n / 3 ? 1.f : (i < n / 2 ? 30.f : 0.02f);
        x[i] = ((float)(lcg >> 8) / 8388608.f - 1.f) * level;
    }
    return x;
}

// a frequency-modulated carrier whose amplitude fades
std::vector<gr_complex> carrier(int n)
{
    std::vector<gr_complex> x(n);
    double phase = 0.0;
    for (int i = 0; i < n; ++i) {
        phase += 0.9 * (0.6 * std::sin(0.07 * i) + 0.3 * std::sin(0.23 * i + 1.0));
        const double amp = 0.5 + 0.45 * std::cos(i / 477.0);
        x[i] = gr_complex((float)(amp * std::cos(phase)), (float)(amp * std::sin(phase)));
    }
    return x;
}

template <class T>
std::vector<T> as(const std::vector<unsigned char> &b)
{
    std::vector<T> v(b.size() / sizeof(T));
    if (!v.empty()) memcpy(v.data(), b.data(), v.size() * sizeof(T));
    return v;
}

int properties()
{
    int fails = 0;
    std::vector<double> b, a;
    fm_deemph_taps(32e3, 75e-6, b, a);
    const double w_pp = std::tan((1 / 75e-6) / (32e3 * 2));    // fm_emph.py:55-63
    if (b.size() != 2 || a.size() != 2 || a[0] != 1.0 || a[1] != (w_pp - 1) / (w_pp + 1) || b[0] != w_pp / (1 + w_pp) || b[1] != b[0])
        fails++;
    grhip_iir_filter_ffd_sptr f = gr_make_fm_deemph(32e3);
    if (f->input_signature()->sizeof_stream_item(0) != sizeof(float) || f->output_signature()->sizeof_stream_item(0) != sizeof(float) ||
        f->history() != 1) fails++;
    const std::vector<float> lp = grhip_firdes_low_pass_taps(1.0, 32000, 2.7e3, 0.5e3);
    if (lp.size() != 211) fails++;
    grhip_fm_demod_cf_sptr rx = gr_make_nbfm_rx(16000, 32000);
    if (rx->input_signature()->sizeof_stream_item(0) != sizeof(gr_complex) || rx->output_signature()->sizeof_stream_item(0) != sizeof(float) ||
        rx->history() != 1 || rx->decimation() != 2 || rx->relative_rate() != 0.5) fails++;
    // the reference's refusals and the library's own
    try { gr_make_nbfm_rx(16000, 40000); fails++; } catch (const std::invalid_argument &) {}
    try { gr_make_iir_filter_ffd({1.0}, {}); fails++; } catch (const std::invalid_argument &) {}
    try { grhip_firdes_low_pass_taps(1.0, 32000, 20e3, 0.5e3); fails++; } catch (const std::invalid_argument &) {}
    std::cout << "properties: " << (fails ? "FAIL" : "ok") << "\n";
    return fails;
}

int iir_under_executor()
{
    int fails = 0;
    const int n = 6037;
    const std::vector<float> x = noise(n);
    const std::vector<double> ff = {0.2, 0.4, 0.2}, fb = {0.0, 1.0040916292848976, -0.5041};
    std::vector<double> b, a;
    fm_deemph_taps(32e3, 75e-6, b, a);
    for (int mode : {GRHIP_MODE_GENERIC, GRHIP_MODE_FAST}) {
        // calls of at most 37 items take the serial walk whatever the mode: bit for bit in both
        grhip_iir_filter_ffd_sptr blk = gr_make_iir_filter_ffd(ff, fb);
        blk->set_mode(mode);
        grhip_linear_flowgraph fg(37);
        fg.connect(blk);
        std::vector<float> y = as<float>(fg.run(x.data(), 4000));
        blk->set_taps(b, a);                                    // latched: holds from the next work call, from zero state
        const std::vector<float> y2 = as<float>(fg.run(x.data() + 4000, n - 4000));
        y.insert(y.end(), y2.begin(), y2.end());
        std::vector<float> want = iir_loop(ff, fb, std::vector<float>(x.begin(), x.begin() + 4000));
        const std::vector<float> want2 = iir_loop(b, a, std::vector<float>(x.begin() + 4000, x.end()));
        want.insert(want.end(), want2.begin(), want2.end());
        const bool same = y.size() == want.size() && !memcmp(y.data(), want.data(), y.size() * sizeof(float));
        std::cout << "iir_filter_ffd mode " << mode << ": " << n << (same ? " items equal\n" : " items: differs from the loop over filter()\n");
        fails += same ? 0 : 1;
    }
    return fails;
}

int nbfm_under_executor()
{
    int fails = 0;
    const int n = 3 * 8192 + 5;
    const std::vector<gr_complex> x = carrier(n);
    const std::vector<float> lp = grhip_firdes_low_pass_taps(1.0, 32000, 2.7e3, 0.5e3);
    // the three blocks, the FIR in its generic order
    grhip_set_default_mode(GRHIP_MODE_GENERIC);
    std::vector<float> want;
    {
        grhip_linear_flowgraph fg(4096);
        fg.connect(grhip_make_quadrature_demod_cf((float)(32000 / (2 * M_PI * 5e3))));
        grhip_iir_filter_ffd_sptr d = gr_make_fm_deemph(32000);
        d->set_mode(GRHIP_MODE_GENERIC);
        fg.connect(d);
        fg.connect(grhip_make_fir_filter_fff(2, lp));
        want = as<float>(fg.run(x.data(), n));
    }
    grhip_set_default_mode(GRHIP_MODE_FAST);
    float peak = 0.f;
    for (float v : want) peak = std::max(peak, std::fabs(v));
    for (int mode : {GRHIP_MODE_GENERIC, GRHIP_MODE_FAST}) {
        for (int max_noutput : {4096, 1 << 20}) {
            grhip_fm_demod_cf_sptr rx = gr_make_nbfm_rx(16000, 32000);
            rx->set_mode(mode);
            if (rx->engine() != (mode == GRHIP_MODE_FAST ? 1 : 0)) fails++;
            grhip_linear_flowgraph fg(max_noutput);
            fg.connect(rx);
            const std::vector<float> y = as<float>(fg.run(x.data(), n));
            bool ok = y.size() == want.size() && y.size() == (size_t)(n / 2);
            double err = 0.0;
            if (ok && mode == GRHIP_MODE_GENERIC) ok = !memcmp(y.data(), want.data(), y.size() * sizeof(float));
            if (ok && mode == GRHIP_MODE_FAST) {
                for (size_t i = 0; i < y.size(); ++i) err = std::max(err, (double)std::fabs(y[i] - want[i]));
                ok = err <= 1e-5 * peak;
            }
            std::cout << "nbfm_rx mode " << mode << ", calls of at most " << max_noutput << " outputs: " << y.size()
                      << (ok ? " items ok" : " items: differs from the three blocks") << " (error " << err / peak << " of the peak)\n";
            fails += ok ? 0 : 1;
        }
    }
    return fails;
}

}  // namespace

int main()
{
    try {
        const int fails = properties() + iir_under_executor() + nbfm_under_executor();
        if (!fails) std::cout << "fm_demod_test ok\n";
        return fails ? 1 : 0;
    } catch (const std::exception &e) {
        std::cerr << "fm_demod_test: " << e.what() << "\n";
        return 1;
    }
}
