// fll_band_edge_test -- the fll_band_edge_cc block of grhip_blocks.h: the reference's factory signature, four-output
// signature, history, setters and getters, and a flowgraph under the stand-in executor (grhip_executor.h): source ->
// the block in calls of at most 37 items -> sink.
//   * in GRHIP_MODE_GENERIC the block equals, bit for bit, a loop restated here from
//     gr-digital/lib/digital_fll_band_edge_cc.cc:208-259 and general/gri_control_loop.cc:56-80 on one linear output
//     buffer, with the float-rounded double sine and cosine and the library's taps;
//   * all four outputs, driven directly in two calls, equal the restated loop's;
//   * in GRHIP_MODE_FAST the loop's frequency settles where the restated loop's does.
// For tests/test_gpu_host_fll_band_edge.py; no arguments.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <stdexcept>
#include <vector>

#include "grhip_blocks.h"
#include "grhip_executor.h"

namespace {

const double TWOPI = 2 * M_PI;

struct fll_loop {           // digital_fll_band_edge_cc.cc:208-259 around gri_control_loop.cc:49-80
    float alpha, beta, max_freq, phase = 0, freq = 0;
    int fs;
    std::vector<gr_complex> lower, upper, out;      // out: the reference's output buffer, linear
    std::vector<float> frq, phs, err;
    fll_loop(float sps, float rolloff, int size, float bw) : fs(size), lower(size), upper(size)
    {
        const float damping = sqrtf(2.0f) / 2.0f;
        const float denom = (1.0 + 2.0 * damping * bw + bw * bw);
        alpha = (4 * damping * bw) / denom;
        beta = (4 * bw * bw) / denom;
        max_freq = TWOPI * (2.0 / sps);
        grhip_detail::check(grhip_fll_band_edge_taps(sps, rolloff, size, lower.data(), upper.data()));
    }
    void run(const std::vector<gr_complex> &x)
    {
        const size_t n = x.size();
        std::vector<gr_complex> in(fs, gr_complex(0, 0));           // history = fs + 1: in[0] is fs items back
        in.insert(in.end(), x.begin(), x.end());
        out.assign(n + fs, gr_complex(0, 0));
        frq.assign(n, 0); phs.assign(n, 0); err.assign(n, 0);
        for (size_t i = 0; i < n; ++i) {
            const float sn = (float)sin((double)phase), cs = (float)cos((double)phase);
            out[i + fs - 1] = gr_complex(in[i].real() * cs - in[i].imag() * sn, in[i].real() * sn + in[i].imag() * cs);
            gr_complex out_upper = 0, out_lower = 0;
            for (int k = 0; k < fs; ++k) {
                out_upper += upper[k] * out[i + k];
                out_lower += lower[k] * out[i + k];
            }
            const float error = norm(out_lower) - norm(out_upper);
            freq = freq + beta * error;
            phase = phase + freq + alpha * error;
            while (phase > TWOPI) phase -= TWOPI;
            while (phase < -TWOPI) phase += TWOPI;
            if (freq > max_freq) freq = max_freq;
            else if (freq < -max_freq) freq = -max_freq;
            frq[i] = freq; phs[i] = phase; err[i] = error;
        }
    }
};

template <class F> bool throws(F f)
{
    try { f(); } catch (const std::invalid_argument &) { return true; }
    return false;
}

int properties()
{
    int fails = 0;
    grhip_fll_band_edge_cc_sptr b = digital_make_fll_band_edge_cc(4.f, 0.35f, 45, 0.0628f);
    if (b->input_signature()->sizeof_stream_item(0) != sizeof(gr_complex) || b->input_signature()->max_streams() != 1 ||
        b->output_signature()->sizeof_stream_item(0) != sizeof(gr_complex) || b->output_signature()->sizeof_stream_item(1) != sizeof(float) ||
        b->output_signature()->sizeof_stream_item(3) != sizeof(float) || b->output_signature()->min_streams() != 1 ||
        b->output_signature()->max_streams() != 4 || b->history() != 46) fails++;
    const fll_loop want(4.f, 0.35f, 45, 0.0628f);
    if (b->get_samples_per_symbol() != 4.f || b->get_rolloff() != 0.35f || b->get_filter_size() != 45 || b->get_alpha() != want.alpha ||
        b->get_beta() != want.beta || b->get_phase() != 0.f || b->get_frequency() != 0.f) fails++;
    b->set_frequency(4.f);
    if (b->get_frequency() != -want.max_freq) fails++;
    b->set_filter_size(55); b->set_rolloff(0.5f); b->set_samples_per_symbol(2.f);
    if (b->history() != 56 || b->get_filter_size() != 55 || b->get_rolloff() != 0.5f || b->get_samples_per_symbol() != 2.f) fails++;
    if (!throws([&] { b->set_filter_size(0); }) || !throws([&] { b->set_rolloff(1.5f); }) || !throws([&] { b->set_samples_per_symbol(0.f); }) ||
        !throws([&] { digital_make_fll_band_edge_cc(4.f, 0.35f, 1025, 0.0628f); }) || !throws([&] { digital_make_fll_band_edge_cc(4.f, 0.35f, 45, -1.f); }) ||
        b->history() != 56) fails++;
    const std::vector<float> rrc = grhip_firdes_root_raised_cosine_taps(4, 4, 1.0, 0.35, 44);
    if (rrc.size() != 45 || rrc[22] <= rrc[21] || !throws([&] { grhip_firdes_root_raised_cosine_taps(4, 4, 1.0, 0.35, 0); })) fails++;
    std::cout << "properties: " << (fails ? "FAIL" : "ok") << "\n";
    return fails;
}

int loop()
{
    int fails = 0;
    const int n = 4001, sps = 4, ntaps = 45;
    // the QA's kind of signal: +-1 symbols through the root-raised-cosine pulse, spun by 0.2 rad/sample
    const std::vector<float> rrc = grhip_firdes_root_raised_cosine_taps(sps, sps, 1.0, 0.35, ntaps);
    std::vector<gr_complex> x(n);
    unsigned lcg = 2463534242u;
    std::vector<float> sym(n / sps + 1);
    for (float &s : sym) { lcg = lcg * 1664525u + 1013904223u; s = (lcg >> 20) & 1 ? 1.f : -1.f; }
    for (int i = 0; i < n; ++i) {
        double acc = 0;
        for (int k = i % sps; k < ntaps && k <= i; k += sps) acc += rrc[k] * sym[(i - k) / sps];
        x[i] = gr_complex((float)(acc * cos(0.2 * i)), (float)(acc * sin(0.2 * i)));
    }
    fll_loop r(sps, 0.35f, ntaps, 0.0628f);
    r.run(x);
    grhip_fll_band_edge_cc_sptr b = digital_make_fll_band_edge_cc(sps, 0.35f, ntaps, 0.0628f);
    b->set_mode(GRHIP_MODE_GENERIC);
    grhip_linear_flowgraph fg(37);
    fg.connect(b);
    const std::vector<unsigned char> y = fg.run(x.data(), x.size());
    const float ph = b->get_phase(), fr = b->get_frequency();
    bool same = y.size() == n * sizeof(gr_complex) && !memcmp(y.data(), r.out.data(), y.size()) && !memcmp(&ph, &r.phase, 4) && !memcmp(&fr, &r.freq, 4);
    // all four outputs, two calls, the scheduler's history in front of each
    grhip_fll_band_edge_cc_sptr b2 = digital_make_fll_band_edge_cc(sps, 0.35f, ntaps, 0.0628f);
    b2->set_mode(GRHIP_MODE_GENERIC);
    std::vector<gr_complex> in(ntaps, gr_complex(0, 0)), o(n);
    in.insert(in.end(), x.begin(), x.end());
    std::vector<float> f(n), p(n), e(n);
    for (int at = 0, m = 1500; at < n; at += m, m = n - at) {
        gr_vector_const_void_star ins(1, in.data() + at);
        gr_vector_void_star outs{o.data() + at, f.data() + at, p.data() + at, e.data() + at};
        if (b2->work(m, ins, outs) != m) same = false;
    }
    same = same && !memcmp(o.data(), r.out.data(), n * sizeof(gr_complex)) && !memcmp(f.data(), r.frq.data(), n * 4) &&
           !memcmp(p.data(), r.phs.data(), n * 4) && !memcmp(e.data(), r.err.data(), n * 4);
    // the float NCO and tree sums settle on the same frequency
    grhip_fll_band_edge_cc_sptr b3 = digital_make_fll_band_edge_cc(sps, 0.35f, ntaps, 0.0628f);
    b3->set_mode(GRHIP_MODE_FAST);
    grhip_linear_flowgraph fg3(37);
    fg3.connect(b3);
    fg3.run(x.data(), x.size());
    const float off = std::fabs(b3->get_frequency() - r.freq);
    same = same && off <= 5e-5f && std::fabs(r.freq + 0.2f) <= 5e-5f;
    std::cout << "fll_band_edge_cc: " << n << (same ? " items, the four outputs and the state equal the restated loop; " : " items: differs from the restated loop; ")
              << "frequency " << r.freq << ", FAST within " << off << "\n";
    fails += same ? 0 : 1;
    return fails;
}

}  // namespace

int main()
{
    try {
        const int fails = properties() + loop();
        if (!fails) std::cout << "fll_band_edge_test ok\n";
        return fails ? 1 : 0;
    } catch (const std::exception &e) {
        std::cerr << "fll_band_edge_test: " << e.what() << "\n";
        return 1;
    }
}
