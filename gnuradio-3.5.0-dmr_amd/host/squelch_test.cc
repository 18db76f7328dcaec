// squelch_test -- the power squelch blocks of grhip_blocks.h (pwr_squelch_cc, pwr_squelch_ff, simple_squelch_cc): the
// reference's factory signatures with their defaults, item sizes and accessors, what the preconditions throw, a
// hand-evaluated case of the machine (the values tests/squelch_ref.py gives for it, test_machine_by_hand), and, run
// under the stand-in executor (grhip_executor.h) in small calls, bit for bit what ONE call of the C ABI produces on the
// whole stream (GRHIP_MODE_GENERIC: detector, machine and ramp position carry across the executor's calls).
// For tests/test_gpu_squelch.py; no arguments.
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
    try { gr_make_pwr_squelch_cc(-20, 1.5); fails++; } catch (const std::out_of_range &) {}
    try { gr_make_pwr_squelch_ff(-20, 0.1, -1); fails++; } catch (const std::invalid_argument &) {}
    try { gr_make_simple_squelch_cc(-20, -0.5); fails++; } catch (const std::out_of_range &) {}
    grhip_pwr_squelch_cc_sptr c = gr_make_pwr_squelch_cc(-33.0);                   // alpha 0.0001, ramp 0, gate false
    if (c->input_signature()->sizeof_stream_item(0) != sizeof(gr_complex) ||
        c->output_signature()->sizeof_stream_item(0) != sizeof(gr_complex) || c->history() != 1) fails++;
    if (c->ramp() != 0 || c->gate() || c->unmuted() || c->threshold() != 10 * std::log10(std::pow(10.0, -33.0 / 10))) fails++;
    std::vector<float> r = c->squelch_range();
    if (r.size() != 3 || r[0] != -50.f || r[1] != 50.f || r[2] != 1.f) fails++;
    c->set_ramp(5); c->set_gate(true); c->set_threshold(-7.5); c->set_alpha(0.25);
    if (c->ramp() != 5 || !c->gate() || c->threshold() != 10 * std::log10(std::pow(10.0, -7.5 / 10))) fails++;
    try { c->set_alpha(1.0001); fails++; } catch (const std::out_of_range &) {}
    try { c->set_ramp(-3); fails++; } catch (const std::invalid_argument &) {}

    // alpha 1: the detector is the sample's power; -20 dB is 0.01; ramp 2
    const float x[9] = {0, 1, 1, 1, 1, 0, 0, 0, 1};
    const float e1 = (float)(1.0 * (0.5 - std::cos(M_PI * 1 / 2) / 2.0));
    {
        grhip_pwr_squelch_ff_sptr f = gr_make_pwr_squelch_ff(-20, 1.0, 2, false);
        if (f->input_signature()->sizeof_stream_item(0) != sizeof(float)) fails++;
        float y[9];
        gr_vector_int ni(1, 9);
        gr_vector_const_void_star in(1, x);
        gr_vector_void_star out(1, y);
        const float want[9] = {0, 0, e1, 1, 1, 0, 0, 0, 0};
        if (f->general_work(9, ni, in, out) != 9 || f->consumed() != 9 || memcmp(y, want, sizeof want) || !f->unmuted()) fails++;
        try { f->set_ramp(0); fails++; } catch (const std::out_of_range &) {}       // the stream is in its attack
    }
    {
        grhip_pwr_squelch_ff_sptr f = gr_make_pwr_squelch_ff(-20, 1.0, 2, true);
        float y[9];
        gr_vector_int ni(1, 9);
        gr_vector_const_void_star in(1, x);
        gr_vector_void_star out(1, y);
        const float want[7] = {0, e1, 1, 1, 0, 0, 0};
        if (f->general_work(9, ni, in, out) != 7 || f->consumed() != 9 || memcmp(y, want, sizeof want)) fails++;
    }
    {
        grhip_simple_squelch_cc_sptr s = gr_make_simple_squelch_cc(-20, 1.0);
        gr_complex z[9], y[9];
        for (int i = 0; i < 9; ++i) z[i] = gr_complex(x[i], x[i]);
        gr_vector_const_void_star in(1, z);
        gr_vector_void_star out(1, y);
        if (s->unmuted() || s->work(9, in, out) != 9 || memcmp(y, z, sizeof z) || !s->unmuted()) fails++;
        if (s->work(5, in, out) != 5 || !s->unmuted() || s->work(8, in, out) != 8 || s->unmuted()) fails++;
        if (s->threshold() != 10 * std::log10(std::pow(10.0, -20 / 10.0)) || s->squelch_range().size() != 3) fails++;
    }
    std::cout << "properties: " << (fails ? "FAIL" : "ok") << "\n";
    return fails;
}

template <class T>
static int same(const char *what, const std::vector<unsigned char> &y, const std::vector<T> &one)
{
    if (y.size() != one.size() * sizeof(T) || memcmp(y.data(), one.data(), y.size())) {
        std::cout << what << ": executor output differs from the single call (" << y.size() / sizeof(T) << " vs " << one.size() << " items)\n";
        return 1;
    }
    std::cout << what << ": " << one.size() << " items equal\n";
    return 0;
}

static int under_executor()
{
    int fails = 0;
    const int n = 30000;
    unsigned lcg = 2463534242u;
    std::vector<gr_complex> z(n);
    std::vector<float> x(n);
    for (int i = 0; i < n; ++i) {                           // noise of 0.01, bursts of 0.7 on [4000, 9000), [15000, 15300), [29000, n)
        const bool on = (i >= 4000 && i < 9000) || (i >= 15000 && i < 15300) || i >= 29000;
        lcg = lcg * 1664525u + 1013904223u;
        const float a = ((float)(lcg >> 8) / 8388608.f - 1.f) * 0.01f;
        lcg = lcg * 1664525u + 1013904223u;
        const float b = ((float)(lcg >> 8) / 8388608.f - 1.f) * 0.01f;
        x[i] = a + (on ? 0.7f : 0.f);
        z[i] = gr_complex(x[i], b);
    }
    for (int gate = 0; gate < 2; ++gate) {
        {
            grhip_linear_flowgraph fg(37);
            grhip_pwr_squelch_cc_sptr b = gr_make_pwr_squelch_cc(-20, 0.05, 64, gate != 0);
            b->set_mode(GRHIP_MODE_GENERIC);
            fg.connect(b);
            std::vector<unsigned char> y = fg.run(z.data(), n);
            grhip_pwr_squelch_cc *h = nullptr;
            grhip_detail::check(grhip_pwr_squelch_cc_create(&h, -20, 0.05, 64, gate, 0));
            grhip_detail::check(grhip_pwr_squelch_cc_set_mode(h, GRHIP_MODE_GENERIC));
            std::vector<gr_complex> one(n);
            int produced = 0;
            grhip_detail::check(grhip_pwr_squelch_cc_work(h, n, z.data(), one.data(), &produced));
            if (b->unmuted() != (grhip_pwr_squelch_cc_unmuted(h, 0) != 0) || !b->unmuted()) fails++;
            grhip_pwr_squelch_cc_destroy(h);
            if (gate ? !(produced > 5000 && produced < n) : produced != n) fails++;
            one.resize(produced);
            fails += same(gate ? "pwr_squelch_cc, gated" : "pwr_squelch_cc", y, one);
        }
        {
            grhip_linear_flowgraph fg(50);
            grhip_pwr_squelch_ff_sptr b = gr_make_pwr_squelch_ff(-20, 0.05, 7, gate != 0);
            b->set_mode(GRHIP_MODE_GENERIC);
            fg.connect(b);
            std::vector<unsigned char> y = fg.run(x.data(), n);
            grhip_pwr_squelch_ff *h = nullptr;
            grhip_detail::check(grhip_pwr_squelch_ff_create(&h, -20, 0.05, 7, gate, 0));
            grhip_detail::check(grhip_pwr_squelch_ff_set_mode(h, GRHIP_MODE_GENERIC));
            std::vector<float> one(n);
            int produced = 0;
            grhip_detail::check(grhip_pwr_squelch_ff_work(h, n, x.data(), one.data(), &produced));
            grhip_pwr_squelch_ff_destroy(h);
            one.resize(produced);
            fails += same(gate ? "pwr_squelch_ff, gated" : "pwr_squelch_ff", y, one);
        }
    }
    {
        grhip_linear_flowgraph fg(61);
        grhip_simple_squelch_cc_sptr b = gr_make_simple_squelch_cc(-20, 0.05);
        b->set_mode(GRHIP_MODE_GENERIC);
        fg.connect(b);
        std::vector<unsigned char> y = fg.run(z.data(), n);
        grhip_simple_squelch_cc *h = nullptr;
        grhip_detail::check(grhip_simple_squelch_cc_create(&h, -20, 0.05, 0));
        grhip_detail::check(grhip_simple_squelch_cc_set_mode(h, GRHIP_MODE_GENERIC));
        std::vector<gr_complex> one(n);
        int produced = 0;
        grhip_detail::check(grhip_simple_squelch_cc_work(h, n, z.data(), one.data(), &produced));
        grhip_simple_squelch_cc_destroy(h);
        if (produced != n || !b->unmuted()) fails++;
        fails += same("simple_squelch_cc", y, one);
    }
    return fails;
}

int main()
{
    try {
        return (properties() + under_executor()) ? 1 : 0;
    } catch (const std::exception &e) {
        std::cerr << "squelch_test: " << e.what() << "\n";
        return 1;
    }
}
