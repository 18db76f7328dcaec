// agc_test -- the gain-loop blocks of grhip_blocks.h: the reference's factory signatures with their defaults, item
// sizes, accessors and setters, and a small flowgraph under the stand-in executor (grhip_executor.h): the source in
// pieces of uneven size, each run in calls of at most 37 items -> the block -> sink.  Output and final gain equal,
// bit for bit, a loop over scale() restated here (general/gri_agc_cc.h:53-61, gri_agc2_ff.h:55-75), in both modes: calls
// this short take the serial walk whatever the mode.
// For tests/test_gpu_agc.py; no arguments.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <stdexcept>
#include <vector>

#include "grhip_blocks.h"
#include "grhip_executor.h"

namespace {

struct agc_cc_loop {        // gri_agc_cc.h:53-61
    float rate, reference, gain, max_gain;
    gr_complex scale(gr_complex in)
    {
        const gr_complex out(in.real() * gain, in.imag() * gain);
        gain += rate * (reference - std::sqrt(out.real() * out.real() + out.imag() * out.imag()));
        if (max_gain > 0.0 && gain > max_gain) gain = max_gain;
        return out;
    }
};

struct agc2_ff_loop {       // gri_agc2_ff.h:55-75
    float attack, decay, reference, gain, max_gain;
    float scale(float in)
    {
        const float out = in * gain;
        const float tmp = std::fabs(out) - reference;
        const float rate = std::fabs(tmp) > gain ? attack : decay;
        gain -= tmp * rate;
        if (gain < 0.0) gain = 10e-5;
        if (max_gain > 0.0 && gain > max_gain) gain = max_gain;
        return out;
    }
};

int properties()
{
    int fails = 0;
    grhip_agc_cc_sptr a = gr_make_agc_cc();                 // 1e-4, 1.0, 1.0, 0.0
    if (a->input_signature()->sizeof_stream_item(0) != sizeof(gr_complex) ||
        a->output_signature()->sizeof_stream_item(0) != sizeof(gr_complex) || a->history() != 1) fails++;
    if (a->rate() != 1e-4f || a->reference() != 1.f || a->gain() != 1.f || a->max_gain() != 0.f) fails++;
    a->set_rate(0.5f); a->set_reference(2.f); a->set_gain(-3.f); a->set_max_gain(7.f);
    if (a->rate() != 0.5f || a->reference() != 2.f || a->gain() != -3.f || a->max_gain() != 7.f) fails++;
    grhip_agc_ff_sptr f = gr_make_agc_ff(1e-3, 1, 2, 1000);
    if (f->input_signature()->sizeof_stream_item(0) != sizeof(float) || f->rate() != 1e-3f || f->gain() != 2.f ||
        f->max_gain() != 1000.f) fails++;
    grhip_agc2_cc_sptr c = gr_make_agc2_cc();               // 1e-1, 1e-2, 1.0, 1.0, 0.0
    if (c->attack_rate() != 1e-1f || c->decay_rate() != 1e-2f || c->reference() != 1.f || c->gain() != 1.f ||
        c->max_gain() != 0.f || c->output_signature()->sizeof_stream_item(0) != sizeof(gr_complex)) fails++;
    grhip_agc2_ff_sptr d = gr_make_agc2_ff(1e-2, 1e-3, 1, 1, 1000);
    d->set_attack_rate(0.25f); d->set_decay_rate(0.125f);
    if (d->attack_rate() != 0.25f || d->decay_rate() != 0.125f || d->max_gain() != 1000.f || d->history() != 1) fails++;
    // nothing is refused at construction: the reference checks nothing
    try { gr_make_agc_cc(-1.f, NAN, INFINITY, -2.f); } catch (const std::exception &) { fails++; }
    std::cout << "properties: " << (fails ? "FAIL" : "ok") << "\n";
    return fails;
}

// noise of three levels: 1, 30 and 0.02
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

int under_executor()
{
    int fails = 0;
    const int n = 6037;
    const std::vector<float> raw = noise(2 * n);
    std::vector<gr_complex> xc(n);
    for (int i = 0; i < n; ++i) xc[i] = gr_complex(raw[2 * i], raw[2 * i + 1]);
    const std::vector<float> xf(raw.begin(), raw.begin() + n);
    for (int mode : {GRHIP_MODE_GENERIC, GRHIP_MODE_FAST}) {
        {
            grhip_agc_cc_sptr b = gr_make_agc_cc(1e-3, 1, 1, 2.0);
            b->set_mode(mode);
            const std::vector<unsigned char> y = in_pieces(b, xc);
            agc_cc_loop r = {1e-3f, 1.f, 1.f, 2.0f};
            std::vector<gr_complex> want(n);
            for (int i = 0; i < n; ++i) want[i] = r.scale(xc[i]);
            const float g = b->gain();
            const bool same = y.size() == n * sizeof(gr_complex) && !memcmp(y.data(), want.data(), y.size()) &&
                              !memcmp(&g, &r.gain, sizeof g);
            std::cout << "agc_cc mode " << mode << ": " << n << (same ? " items and the gain equal\n" : " items: differs from the loop over scale()\n");
            fails += same ? 0 : 1;
        }
        {
            grhip_agc2_ff_sptr b = gr_make_agc2_ff(0.5, 0.1, 1, 1, 1000);
            b->set_mode(mode);
            const std::vector<unsigned char> y = in_pieces(b, xf);
            agc2_ff_loop r = {0.5f, 0.1f, 1.f, 1.f, 1000.f};
            std::vector<float> want(n);
            for (int i = 0; i < n; ++i) want[i] = r.scale(xf[i]);
            const float g = b->gain();
            const bool same = y.size() == n * sizeof(float) && !memcmp(y.data(), want.data(), y.size()) &&
                              !memcmp(&g, &r.gain, sizeof g);
            std::cout << "agc2_ff mode " << mode << ": " << n << (same ? " items and the gain equal\n" : " items: differs from the loop over scale()\n");
            fails += same ? 0 : 1;
        }
    }
    return fails;
}

}  // namespace

int main()
{
    try {
        const int fails = properties() + under_executor();
        if (!fails) std::cout << "agc_test ok\n";
        return fails ? 1 : 0;
    } catch (const std::exception &e) {
        std::cerr << "agc_test: " << e.what() << "\n";
        return 1;
    }
}
