// am_demod_test -- the magnitude, AM-demodulator and FM-preset blocks of grhip_blocks.h: factory signatures, item sizes,
// history and relative rate, the optfir tap designer, and small flowgraphs under the stand-in executor
// (grhip_executor.h).  gr_make_demod_10k0a3e_cf as ONE block against the blocks it stands for (complex_to_mag, the add
// of -1 done here in float, fir_filter_fff in its generic order) run one after the other under the same executor: bit
// for bit in GRHIP_MODE_GENERIC, within 1e-5 of the peak for the fused kernel; engine() as expected for every preset.
// For tests/test_gpu_host_am_demod.py; no arguments.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <stdexcept>
#include <vector>

#include "grhip_blocks.h"
#include "grhip_executor.h"

namespace {

// an amplitude-modulated carrier: 50 % tone modulation, a loud stretch, a faint one and a stretch of exact zeros
std::vector<gr_complex> carrier(int n)
{
    std::vector<gr_complex> x(n);
    for (int i = 0; i < n; ++i) {
        double amp = 1.0 + 0.5 * std::sin(0.081 * i);
        const int part = (i * 8) / n;
        if (part == 2) amp *= 30.0;
        if (part == 4) amp *= 1e-3;
        if (part == 6) amp = 0.0;
        x[i] = gr_complex((float)(amp * std::cos(0.31 * i)), (float)(amp * std::sin(0.31 * i)));
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
    const std::vector<double> lp = grhip_optfir_low_pass_taps(0.5, 16e3, 5000, 5500, 0.1, 60);
    if (lp.size() != 83) fails++;
    for (size_t i = 0; i < lp.size(); ++i)
        if (lp[i] != lp[lp.size() - 1 - i]) { fails++; break; }
    grhip_am_demod_cf_sptr rx = gr_make_demod_10k0a3e_cf(16e3, 1);
    if (rx->input_signature()->sizeof_stream_item(0) != sizeof(gr_complex) || rx->output_signature()->sizeof_stream_item(0) != sizeof(float) ||
        rx->history() != 1 || rx->decimation() != 1 || rx->relative_rate() != 1.0 || rx->engine() != 1 || rx->audio_taps().size() != 83)
        fails++;
    for (size_t i = 0; i < lp.size() && i < rx->audio_taps().size(); ++i)
        if (rx->audio_taps()[i] != (float)lp[i]) { fails++; break; }
    grhip_am_demod_cf_sptr am = gr_make_am_demod_cf(32e3, 4, 3000, 4500);
    if (am->decimation() != 4 || am->relative_rate() != 0.25 || am->engine() != 1) fails++;
    am->set_mode(GRHIP_MODE_GENERIC);
    if (am->engine() != 0) fails++;
    grhip_complex_to_mag_sptr m = gr_make_complex_to_mag(3);
    if (m->input_signature()->sizeof_stream_item(0) != 3 * sizeof(gr_complex) || m->output_signature()->sizeof_stream_item(0) != 3 * sizeof(float) ||
        m->history() != 1) fails++;
    // the FM presets: 61 taps run the fused kernel, the 1164 of the wide-band preset do not
    grhip_fm_demod_cf_sptr nb = gr_make_demod_20k0f3e_cf(32e3, 4);
    if (nb->decimation() != 4 || nb->engine() != 1) fails++;
    grhip_fm_demod_cf_sptr wb = gr_make_demod_200kf3e_cf(320e3, 10);
    if (wb->decimation() != 10 || wb->engine() != 0) fails++;
    if (grhip_optfir_low_pass_taps(1.0, 32e3, 3000, 4500, 0.1, 60).size() != 61 ||
        grhip_optfir_low_pass_taps(20.0, 320e3, 15000, 16000, 0.1, 60).size() != 1164) fails++;
    // refusals
    try { grhip_optfir_low_pass_taps(1.0, 32e3, 3000, 3001, 0.1, 60); fails++; } catch (const std::out_of_range &) {}
    try { grhip_optfir_low_pass_taps(1.0, 0.0, 3000, 4500, 0.1, 60); fails++; } catch (const std::invalid_argument &) {}
    try { grhip_make_am_demod_cf(0, {1.f, 2.f}); fails++; } catch (const std::invalid_argument &) {}
    try { grhip_make_am_demod_cf(1, std::vector<float>()); fails++; } catch (const std::invalid_argument &) {}
    std::cout << "properties: " << (fails ? "FAIL" : "ok") << "\n";
    return fails;
}

int am_under_executor()
{
    int fails = 0;
    const int n = 3 * 4096 + 5;
    const std::vector<gr_complex> x = carrier(n);
    const std::vector<float> taps = grhip_optfir_low_pass_taps_f(0.5, 16e3, 5000, 5500);
    for (int decim : {1, 3}) {
        // the blocks one after the other, the FIR in its generic order
        grhip_set_default_mode(GRHIP_MODE_GENERIC);
        std::vector<float> want;
        {
            grhip_linear_flowgraph mag(4096);
            mag.connect(gr_make_complex_to_mag());
            std::vector<float> v = as<float>(mag.run(x.data(), n));
            for (float &f : v) {
                volatile float w = f + -1.0f;                   // gr_add_const_ff(-1): one rounded float add
                f = w;
            }
            grhip_linear_flowgraph fir(4096);
            fir.connect(grhip_make_fir_filter_fff(decim, taps));
            want = as<float>(fir.run(v.data(), n));
        }
        grhip_set_default_mode(GRHIP_MODE_FAST);
        float peak = 0.f;
        for (float v : want) peak = std::max(peak, std::fabs(v));
        for (int mode : {GRHIP_MODE_GENERIC, GRHIP_MODE_FAST}) {
            for (int max_noutput : {1000, 1 << 20}) {
                grhip_am_demod_cf_sptr rx = decim == 1 ? gr_make_demod_10k0a3e_cf(16e3, 1) : grhip_make_am_demod_cf(decim, taps);
                rx->set_mode(mode);
                if (rx->engine() != (mode == GRHIP_MODE_FAST ? 1 : 0)) fails++;
                grhip_linear_flowgraph fg(max_noutput);
                fg.connect(rx);
                const std::vector<float> y = as<float>(fg.run(x.data(), n));
                bool ok = y.size() == want.size() && y.size() == (size_t)(n / decim);
                double err = 0.0;
                if (ok && mode == GRHIP_MODE_GENERIC) ok = !memcmp(y.data(), want.data(), y.size() * sizeof(float));
                if (ok && mode == GRHIP_MODE_FAST) {
                    for (size_t i = 0; i < y.size(); ++i) err = std::max(err, (double)std::fabs(y[i] - want[i]));
                    ok = err <= 1e-5 * peak;
                }
                std::cout << "am_demod_cf decim " << decim << " mode " << mode << ", calls of at most " << max_noutput << " outputs: "
                          << y.size() << (ok ? " items ok" : " items: differs from the blocks in a row") << " (error " << err / peak
                          << " of the peak)\n";
                fails += ok ? 0 : 1;
            }
        }
    }
    return fails;
}

}  // namespace

int main()
{
    try {
        const int fails = properties() + am_under_executor();
        if (!fails) std::cout << "am_demod_test ok\n";
        return fails ? 1 : 0;
    } catch (const std::exception &e) {
        std::cerr << "am_demod_test: " << e.what() << "\n";
        return 1;
    }
}
