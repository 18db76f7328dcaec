// ctcss_squelch_test -- grhip_ctcss_squelch_ff of grhip_blocks.h: the reference's factory signature with its defaults,
// item sizes and accessors, what the preconditions throw, and, run under the stand-in executor (grhip_executor.h) in
// uneven calls most of which complete no block, bit for bit what ONE call of the C ABI produces on the whole stream (the
// blocks of len samples, the last decision and the machine carry across the executor's calls).
// For tests/test_gpu_ctcss_squelch.py; no arguments.
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
    try { gr_make_ctcss_squelch_ff(0, 100.f); fails++; } catch (const std::invalid_argument &) {}
    try { gr_make_ctcss_squelch_ff(8000, 100.f, 0.01, -1); fails++; } catch (const std::invalid_argument &) {}
    try { gr_make_ctcss_squelch_ff(8000, 100.f, 0.01, (1 << 20) + 1); fails++; } catch (const std::out_of_range &) {}
    try { gr_make_ctcss_squelch_ff(5, 100.f); fails++; } catch (const std::out_of_range &) {}           // default len 0
    try { gr_make_ctcss_squelch_ff(8000, NAN); fails++; } catch (const std::invalid_argument &) {}
    try { gr_make_ctcss_squelch_ff(8000, 100.f, 0.01, 0, -2); fails++; } catch (const std::invalid_argument &) {}
    grhip_ctcss_squelch_ff_sptr c = gr_make_ctcss_squelch_ff(8000, 100.f);       // level 0.01, len rate / 10, ramp 0, no gate
    if (c->input_signature()->sizeof_stream_item(0) != sizeof(float) ||
        c->output_signature()->sizeof_stream_item(0) != sizeof(float) || c->history() != 1) fails++;
    if (c->level() != 0.01f || c->len() != 800 || c->ramp() != 0 || c->gate() || c->unmuted()) fails++;
    std::vector<float> r = c->squelch_range();
    if (r.size() != 3 || r[0] != 0.f || r[1] != 1.f || r[2] != 0.01f) fails++;
    c->set_level(0.25f); c->set_ramp(5); c->set_gate(true);
    if (c->level() != 0.25f || c->ramp() != 5 || !c->gate()) fails++;
    try { c->set_ramp(-3); fails++; } catch (const std::invalid_argument &) {}
    std::cout << "properties: " << (fails ? "FAIL" : "ok") << "\n";
    return fails;
}

static int under_executor()
{
    int fails = 0;
    const int n = 30000, rate = 1000, len = 100;
    unsigned lcg = 2463534242u;
    std::vector<float> x(n);
    for (int i = 0; i < n; ++i) {            // noise of 0.01, a 100 Hz tone of 0.1 on [4000, 9030), [15000, 15350), [29000, n)
        const bool on = (i >= 4000 && i < 9030) || (i >= 15000 && i < 15350) || i >= 29000;
        lcg = lcg * 1664525u + 1013904223u;
        x[i] = ((float)(lcg >> 8) / 8388608.f - 1.f) * 0.01f + (on ? 0.1f * (float)std::sin(2.0 * M_PI * 100.0 * i / rate) : 0.f);
    }
    for (int mode : {GRHIP_MODE_GENERIC, GRHIP_MODE_FAST}) {
        for (int gate = 0; gate < 2; ++gate) {
            for (int ramp : {0, 64, 250}) {
                grhip_linear_flowgraph fg(37);
                grhip_ctcss_squelch_ff_sptr b = gr_make_ctcss_squelch_ff(rate, 100.f, 0.01, len, ramp, gate != 0);
                b->set_mode(mode);
                fg.connect(b);
                std::vector<unsigned char> y = fg.run(x.data(), n);
                grhip_ctcss_squelch_ff *h = nullptr;
                grhip_detail::check(grhip_ctcss_squelch_ff_create(&h, rate, 100.f, 0.01f, len, ramp, gate, 0));
                grhip_detail::check(grhip_ctcss_squelch_ff_set_mode(h, mode));
                std::vector<float> one(n);
                int produced = 0;
                grhip_detail::check(grhip_ctcss_squelch_ff_work(h, n, x.data(), one.data(), &produced));
                if (b->unmuted() != (grhip_ctcss_squelch_ff_unmuted(h, 0) != 0) || !b->unmuted()) fails++;
                grhip_ctcss_squelch_ff_destroy(h);
                if (gate ? !(produced > 5000 && produced < n) : produced != n) fails++;
                const bool same = y.size() == (size_t)produced * sizeof(float) && !memcmp(y.data(), one.data(), y.size());
                std::cout << "ctcss_squelch_ff mode " << mode << " ramp " << ramp << (gate ? " gated: " : ": ") << produced
                          << (same ? " items equal\n" : " items, executor output differs from the single call\n");
                fails += same ? 0 : 1;
            }
        }
    }
    return fails;
}

int main()
{
    try {
        return (properties() + under_executor()) ? 1 : 0;
    } catch (const std::exception &e) {
        std::cerr << "ctcss_squelch_test: " << e.what() << "\n";
        return 1;
    }
}
