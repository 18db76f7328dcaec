// running_sum_test -- the dc_blocker / moving_average / integrate blocks of grhip_blocks.h: that they report the
// reference's history, relative_rate and get_group_delay, throw what the reference's preconditions throw, and, run
// under the stand-in executor (grhip_executor.h) with its default chunking, produce bit for bit what ONE call of the C
// ABI produces on the whole stream (GRHIP_MODE_GENERIC; dc_blocker's state carries across the executor's calls, and a
// moving average with max_iter above every call is chunk-independent only in exact arithmetic, so it runs the integer
// type).  For tests/test_gpu_running_sum.py; no arguments.
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
    try { grhip_make_dc_blocker_ff(0); fails++; } catch (const std::invalid_argument &) {}
    try { grhip_make_dc_blocker_cc(-1, false); fails++; } catch (const std::invalid_argument &) {}
    try { grhip_make_moving_average_ff(0, 1.f); fails++; } catch (const std::invalid_argument &) {}
    try { grhip_make_integrate_ii(0); fails++; } catch (const std::invalid_argument &) {}
    grhip_dc_blocker_ff_sptr a = grhip_make_dc_blocker_ff();                        // (32, true)
    if (a->get_group_delay() != 62 || a->history() != 1 || a->relative_rate() != 1.0) fails++;
    grhip_dc_blocker_cc_sptr b = grhip_make_dc_blocker_cc(32, false);
    if (b->get_group_delay() != 31 || b->history() != 1 || b->relative_rate() != 1.0) fails++;
    if (b->input_signature()->sizeof_stream_item(0) != sizeof(gr_complex)) fails++;
    if (grhip_make_dc_blocker_ff(1, true)->get_group_delay() != 0 || grhip_make_dc_blocker_ff(100, true)->get_group_delay() != 198) fails++;
    grhip_moving_average_ff_sptr m = grhip_make_moving_average_ff(10, 0.1f);
    if (m->history() != 10 || m->relative_rate() != 1.0) fails++;
    grhip_moving_average_cc_sptr mc = grhip_make_moving_average_cc(7, gr_complex(0.5f, 0.5f), 100);
    if (mc->history() != 7 || mc->output_signature()->sizeof_stream_item(0) != sizeof(gr_complex)) fails++;
    grhip_moving_average_ss_sptr ms = grhip_make_moving_average_ss(3, 2);
    if (ms->history() != 3 || ms->input_signature()->sizeof_stream_item(0) != sizeof(short)) fails++;
    grhip_integrate_ff_sptr i = grhip_make_integrate_ff(10);
    if (i->decimation() != 10 || i->history() != 1 || i->relative_rate() != 0.1) fails++;
    grhip_integrate_ss_sptr is = grhip_make_integrate_ss(3);
    if (is->decimation() != 3 || is->output_signature()->sizeof_stream_item(0) != sizeof(short)) fails++;
    // the latched setter: the next work returns 0 and the history follows
    std::vector<float> x(64, 1.f), y(64);
    gr_vector_const_void_star in(1, x.data());
    gr_vector_void_star out(1, y.data());
    m->set_length_and_scale(4, 0.25f);
    if (m->history() != 10 || m->work(8, in, out) != 0 || m->history() != 4) fails++;
    if (m->work(8, in, out) != 8 || y[0] != 1.f) fails++;
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
    const size_t n = 70000;                                 // more than one default scheduler call
    unsigned lcg = 12345u;
    std::vector<float> x(n);
    std::vector<int> xi(n);
    for (size_t k = 0; k < n; ++k) {
        lcg = lcg * 1664525u + 1013904223u;
        x[k] = 10.f + (float)(lcg >> 8) / 8388608.f - 1.f;
        xi[k] = (int)lcg;
    }
    {
        grhip_linear_flowgraph fg;
        grhip_dc_blocker_ff_sptr b = grhip_make_dc_blocker_ff(32, true);
        b->set_mode(GRHIP_MODE_GENERIC);
        fg.connect(b);
        std::vector<unsigned char> y = fg.run(x.data(), n);
        grhip_dc_blocker_ff *h = nullptr;
        grhip_detail::check(grhip_dc_blocker_ff_create(&h, 32, 1, 0));
        grhip_detail::check(grhip_dc_blocker_ff_set_mode(h, GRHIP_MODE_GENERIC));
        std::vector<float> one(n);
        grhip_detail::check(grhip_dc_blocker_ff_work(h, (int)n, x.data(), one.data()));
        grhip_dc_blocker_ff_destroy(h);
        fails += same("dc_blocker_ff", y, one);
    }
    {
        grhip_linear_flowgraph fg;
        grhip_moving_average_ii_sptr b = grhip_make_moving_average_ii(10, 3, 4096);
        fg.connect(b);
        std::vector<unsigned char> y = fg.run(xi.data(), n);
        grhip_moving_average_ii *h = nullptr;
        grhip_detail::check(grhip_moving_average_ii_create(&h, 10, 3, (int)n, 0));
        std::vector<int> xh(9, 0), one(n);
        xh.insert(xh.end(), xi.begin(), xi.end());
        grhip_detail::check(grhip_moving_average_ii_work(h, (int)n, xh.data(), one.data()));
        grhip_moving_average_ii_destroy(h);
        fails += same("moving_average_ii", y, one);
    }
    {
        grhip_linear_flowgraph fg;
        grhip_integrate_ff_sptr b = grhip_make_integrate_ff(10);
        b->set_mode(GRHIP_MODE_GENERIC);
        fg.connect(b);
        std::vector<unsigned char> y = fg.run(x.data(), n);
        grhip_integrate_ff *h = nullptr;
        grhip_detail::check(grhip_integrate_ff_create(&h, 10, 0));
        grhip_detail::check(grhip_integrate_ff_set_mode(h, GRHIP_MODE_GENERIC));
        std::vector<float> one(n / 10);
        grhip_detail::check(grhip_integrate_ff_work(h, (int)(n / 10), x.data(), one.data()));
        grhip_integrate_ff_destroy(h);
        fails += same("integrate_ff", y, one);
    }
    return fails;
}

int main()
{
    try {
        return (properties() + under_executor()) ? 1 : 0;
    } catch (const std::exception &e) {
        std::cerr << "running_sum_test: " << e.what() << "\n";
        return 1;
    }
}
