// carrier_test -- the carrier-loop blocks of grhip_blocks.h: the reference's factory signatures, io signatures, setters
// and getters, and small flowgraphs under the stand-in executor (grhip_executor.h): the source in pieces of uneven size,
// each run in calls of at most 37 items -> the block -> sink.
//   * costas_loop_cc in GRHIP_MODE_GENERIC equals, bit for bit, a loop restated here from
//     gr-digital/lib/digital_costas_loop_cc.cc:110-153 and general/gri_control_loop.cc:56-80 with the float-rounded
//     double sine and cosine; its second output, driven directly, is the frequency behind every sample;
//   * the three PLLs give in uneven calls what they give in one call, bit for bit, and follow a clean tone:
//     pll_freqdet_cf settles on its frequency, pll_refout_cc on its phase, pll_carriertracking_cc mixes it down to a
//     constant and reports lock.
// For tests/test_gpu_host_carrier.py; no arguments.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <stdexcept>
#include <vector>

#include "grhip_blocks.h"
#include "grhip_executor.h"

namespace {

const double TWOPI = 2.0f * M_PI;       // gri_control_loop.cc:31

struct costas_loop {        // digital_costas_loop_cc.cc:110-153 around gri_control_loop.cc:49-80
    float alpha, beta, phase = 0, freq = 0;
    int order;
    costas_loop(float bw, int ord) : order(ord)
    {
        const float damping = sqrtf(2.0f) / 2.0f;
        const float denom = (1.0 + 2.0 * damping * bw + bw * bw);
        alpha = (4 * damping * bw) / denom;
        beta = (4 * bw * bw) / denom;
    }
    float detector(gr_complex s) const
    {
        if (order == 2) return s.real() * s.imag();
        if (order == 4) return ((s.real() > 0 ? 1.0 : -1.0) * s.imag() - (s.imag() > 0 ? 1.0 : -1.0) * s.real());
        float K = (sqrt(2.0) - 1);
        if (fabsf(s.real()) >= fabsf(s.imag()))
            return ((s.real() > 0 ? 1.0 : -1.0) * s.imag() - (s.imag() > 0 ? 1.0 : -1.0) * s.real() * K);
        return ((s.real() > 0 ? 1.0 : -1.0) * s.imag() * K - (s.imag() > 0 ? 1.0 : -1.0) * s.real());
    }
    gr_complex step(gr_complex in)
    {
        const float sn = (float)sin((double)-phase), cs = (float)cos((double)-phase);
        const gr_complex out(in.real() * cs - in.imag() * sn, in.real() * sn + in.imag() * cs);
        float error = detector(out);
        float x1 = fabsf(error + 1.0f), x2 = fabsf(error - 1.0f);
        x1 -= x2;
        error = 0.5 * x1;
        freq = freq + beta * error;
        phase = phase + freq + alpha * error;
        while (phase > TWOPI) phase -= TWOPI;
        while (phase < -TWOPI) phase += TWOPI;
        if (freq > 1.0f) freq = 1.0f;
        else if (freq < -1.0f) freq = -1.0f;
        return out;
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
    grhip_costas_loop_cc_sptr c = digital_make_costas_loop_cc(0.05f, 4);
    if (c->input_signature()->sizeof_stream_item(0) != sizeof(gr_complex) || c->output_signature()->sizeof_stream_item(0) != sizeof(gr_complex) ||
        c->output_signature()->sizeof_stream_item(1) != sizeof(float) || c->output_signature()->min_streams() != 1 ||
        c->output_signature()->max_streams() != 2 || c->history() != 1) fails++;
    const costas_loop want(0.05f, 4);
    if (c->get_loop_bandwidth() != 0.05f || c->get_damping_factor() != sqrtf(2.0f) / 2.0f || c->get_alpha() != want.alpha ||
        c->get_beta() != want.beta || c->get_phase() != 0.f || c->get_frequency() != 0.f) fails++;
    c->set_alpha(0.5f); c->set_beta(0.25f); c->set_frequency(2.f); c->set_phase(7.f);
    if (c->get_alpha() != 0.5f || c->get_beta() != 0.25f || c->get_frequency() != -1.f || c->get_phase() != (float)(7.0 - TWOPI)) fails++;
    c->set_frequency(-2.f);
    if (c->get_frequency() != 1.f) fails++;
    if (!throws([&] { c->set_loop_bandwidth(-1.f); }) || !throws([&] { c->set_damping_factor(2.f); }) || !throws([&] { c->set_alpha(-1.f); }) ||
        !throws([&] { c->set_beta(1.5f); }) || !throws([&] { digital_make_costas_loop_cc(0.05f, 3); }) ||
        !throws([&] { gr_make_pll_refout_cc(0.05f, 2000.f, -1.f); })) fails++;
    grhip_pll_freqdet_cf_sptr f = gr_make_pll_freqdet_cf(0.0628f, 2.2f, -2.2f);
    if (f->input_signature()->sizeof_stream_item(0) != sizeof(gr_complex) || f->output_signature()->sizeof_stream_item(0) != sizeof(float) ||
        f->history() != 1) fails++;
    grhip_pll_refout_cc_sptr r = gr_make_pll_refout_cc(0.0628f, -3.72f, -3.74f);
    if (r->output_signature()->sizeof_stream_item(0) != sizeof(gr_complex)) fails++;
    grhip_pll_carriertracking_cc_sptr t = gr_make_pll_carriertracking_cc(0.0314f, 1.f, -1.f);
    if (t->output_signature()->sizeof_stream_item(0) != sizeof(gr_complex) || t->lock_detector() || t->squelch_enable(true) != true ||
        t->set_lock_threshold(0.5f) != 0.5f) fails++;
    std::cout << "properties: " << (fails ? "FAIL" : "ok") << "\n";
    return fails;
}

template <class Blk, class Item>
std::vector<unsigned char> in_pieces(Blk b, const std::vector<Item> &x)
{
    const size_t pieces[] = {1000, 37, 1, 2999, 257};
    std::vector<unsigned char> y;
    size_t at = 0;
    for (int k = 0; at < x.size(); ++k) {
        const size_t m = std::min(k < 5 ? pieces[k] : (size_t)1301, x.size() - at);
        grhip_linear_flowgraph fg(37);
        fg.connect(b);
        const std::vector<unsigned char> part = fg.run(x.data() + at, m);
        y.insert(y.end(), part.begin(), part.end());
        at += m;
    }
    return y;
}

template <class Blk>
std::vector<unsigned char> one_call(Blk b, const std::vector<gr_complex> &x, size_t out_item)
{
    std::vector<unsigned char> y(x.size() * out_item);
    gr_vector_const_void_star in(1, x.data());
    gr_vector_void_star out(1, y.data());
    if (b->work((int)x.size(), in, out) != (int)x.size()) throw std::runtime_error("work came back short");
    return y;
}

int costas()
{
    int fails = 0;
    const int n = 6037;
    unsigned lcg = 2463534242u;
    for (int order : {2, 4, 8}) {
        std::vector<gr_complex> x(n);
        for (int i = 0; i < n; ++i) {
            lcg = lcg * 1664525u + 1013904223u;
            const int k = (lcg >> 20) % order;
            const double a = order == 2 ? M_PI * k : (order == 4 ? M_PI / 4 + M_PI / 2 * k : M_PI / 8 + M_PI / 4 * k);
            const double amp = order == 2 ? 1.0 : (order == 4 ? sqrt(2.0) : 2.0), rot = 0.2 + 1e-3 * i;
            x[i] = gr_complex((float)(amp * cos(a + rot)), (float)(amp * sin(a + rot)));
        }
        costas_loop r(0.05f, order);
        std::vector<gr_complex> want(n);
        std::vector<float> wantf(n);
        for (int i = 0; i < n; ++i) { want[i] = r.step(x[i]); wantf[i] = r.freq; }
        grhip_costas_loop_cc_sptr b = digital_make_costas_loop_cc(0.05f, order);
        b->set_mode(GRHIP_MODE_GENERIC);
        const std::vector<unsigned char> y = in_pieces(b, x);
        const float ph = b->get_phase(), fr = b->get_frequency();
        bool same = y.size() == n * sizeof(gr_complex) && !memcmp(y.data(), want.data(), y.size()) && !memcmp(&ph, &r.phase, 4) &&
                    !memcmp(&fr, &r.freq, 4);
        // both outputs, one call
        grhip_costas_loop_cc_sptr b2 = digital_make_costas_loop_cc(0.05f, order);
        b2->set_mode(GRHIP_MODE_GENERIC);
        std::vector<gr_complex> o(n);
        std::vector<float> f(n);
        gr_vector_const_void_star in(1, x.data());
        gr_vector_void_star out{o.data(), f.data()};
        b2->work(n, in, out);
        same = same && !memcmp(o.data(), want.data(), n * sizeof(gr_complex)) && !memcmp(f.data(), wantf.data(), n * sizeof(float));
        // the float NCO stays within 1e-5 of the peak
        grhip_costas_loop_cc_sptr b3 = digital_make_costas_loop_cc(0.05f, order);
        b3->set_mode(GRHIP_MODE_FAST);
        const std::vector<unsigned char> yf = in_pieces(b3, x);
        float worst = 0.f;
        for (int i = 0; i < n; ++i) worst = std::max(worst, std::abs(((const gr_complex *)yf.data())[i] - want[i]));
        same = same && worst <= 2e-5f;
        std::cout << "costas_loop_cc order " << order << ": " << n
                  << (same ? " items, both outputs and the state equal; FAST within " : " items: differs from the restated loop; FAST within ") << worst << "\n";
        fails += same ? 0 : 1;
    }
    return fails;
}

int plls()
{
    int fails = 0;
    const int n = 6037;
    const double w = 0.3, p0 = 1.0;
    std::vector<gr_complex> x(n);
    for (int i = 0; i < n; ++i) x[i] = gr_complex((float)(2.0 * cos(p0 + w * i)), (float)(2.0 * sin(p0 + w * i)));
    {
        const std::vector<unsigned char> a = in_pieces(gr_make_pll_freqdet_cf(0.05f, 1.f, -1.f), x);
        const std::vector<unsigned char> b = one_call(gr_make_pll_freqdet_cf(0.05f, 1.f, -1.f), x, sizeof(float));
        const float last = ((const float *)a.data())[n - 1];
        const bool ok = a == b && std::fabs(last - (float)w) < 1e-3f;
        std::cout << "pll_freqdet_cf: " << (ok ? "uneven calls equal one call; settles on " : "FAIL, last output ") << last << "\n";
        fails += ok ? 0 : 1;
    }
    {
        const std::vector<unsigned char> a = in_pieces(gr_make_pll_refout_cc(0.05f, 1.f, -1.f), x);
        const std::vector<unsigned char> b = one_call(gr_make_pll_refout_cc(0.05f, 1.f, -1.f), x, sizeof(gr_complex));
        const gr_complex last = ((const gr_complex *)a.data())[n - 1];
        const float err = std::abs(last - x[n - 1] / 2.0f);
        const bool ok = a == b && err < 2e-2f;
        std::cout << "pll_refout_cc: " << (ok ? "uneven calls equal one call; off the tone's phase by " : "FAIL, off by ") << err << "\n";
        fails += ok ? 0 : 1;
    }
    {
        grhip_pll_carriertracking_cc_sptr t = gr_make_pll_carriertracking_cc(0.05f, 1.f, -1.f);
        t->set_lock_threshold(1.0f);
        const std::vector<unsigned char> a = in_pieces(t, x);
        const std::vector<unsigned char> b = one_call(gr_make_pll_carriertracking_cc(0.05f, 1.f, -1.f), x, sizeof(gr_complex));
        const gr_complex last = ((const gr_complex *)a.data())[n - 1];
        const bool ok = a == b && std::abs(last - gr_complex(2.f, 0.f)) < 5e-2f && t->lock_detector();
        std::cout << "pll_carriertracking_cc: " << (ok ? "uneven calls equal one call; mixes the tone down to " : "FAIL, last output ") << last << "\n";
        fails += ok ? 0 : 1;
    }
    return fails;
}

}  // namespace

int main()
{
    try {
        const int fails = properties() + costas() + plls();
        if (!fails) std::cout << "carrier_test ok\n";
        return fails ? 1 : 0;
    } catch (const std::exception &e) {
        std::cerr << "carrier_test: " << e.what() << "\n";
        return 1;
    }
}
