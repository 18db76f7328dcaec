// xlating_test -- drives the real-input blocks (grhip_fir_filter_{fcc,scc,fsf}, grhip_freq_xlating_fir_filter_{ccf,fcf,
// fcc,scf,scc}) through the stand-in executor (grhip_executor.h) in scheduler-style calls, and the gr_fir_{fcc,scc,fsf}_hip
// seams the way the reference's QA checks every implementation (filter/qa_gr_fir_fcc.cc: random taps and input, each
// implementation against the generic one).  Everything runs in GRHIP_MODE_GENERIC and must equal, bit for bit, the
// restatement of the reference's generic code below (filter/gr_fir_XXX_generic.cc.t, gr_freq_xlating_fir_filter_XXX.cc.t,
// gr_rotator.h), compiled here for x86-64.  For tests/test_gpu_realin.py.
//
//   xlating_test            prints one line per check, exits non-zero on any mismatch
#include <cmath>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <random>
#include <string>
#include <vector>

#include "grhip_blocks.h"
#include "grhip_executor.h"
#include "grhip_fir_kernels.h"

typedef std::complex<float> cf;

// ---- the reference's generic FIRs (d = d_taps, reversed taps) ----
static cf fir_cc_one(const std::vector<cf> &d, const float *x)          // gr_fir_fcc_generic, N_UNROLL 2
{
    cf acc0 = 0, acc1 = 0;
    unsigned i = 0, n = (d.size() / 2) * 2;
    for (i = 0; i < n; i += 2) { acc0 += d[i + 0] * x[i + 0]; acc1 += d[i + 1] * x[i + 1]; }
    for (; i < d.size(); i++) acc0 += d[i] * x[i];
    return acc0 + acc1;
}
static cf fir_cc_one(const std::vector<cf> &d, const short *x)          // gr_fir_scc_generic: (float) input
{
    cf acc0 = 0, acc1 = 0;
    unsigned i = 0, n = (d.size() / 2) * 2;
    for (i = 0; i < n; i += 2) { acc0 += d[i + 0] * (float)x[i + 0]; acc1 += d[i + 1] * (float)x[i + 1]; }
    for (; i < d.size(); i++) acc0 += d[i] * (float)x[i];
    return acc0 + acc1;
}
static short fir_fsf_one(const std::vector<float> &d, const float *x)  // gr_fir_fsf_generic, N_UNROLL 4
{
    float acc0 = 0, acc1 = 0, acc2 = 0, acc3 = 0;
    unsigned i = 0, n = (d.size() / 4) * 4;
    for (i = 0; i < n; i += 4) {
        acc0 += d[i + 0] * x[i + 0]; acc1 += d[i + 1] * x[i + 1];
        acc2 += d[i + 2] * x[i + 2]; acc3 += d[i + 3] * x[i + 3];
    }
    for (; i < d.size(); i++) acc0 += d[i] * x[i];
    return (short)(acc0 + acc1 + acc2 + acc3);
}
template <class T> static std::vector<T> rev(const std::vector<T> &v) { return std::vector<T>(v.rbegin(), v.rend()); }

// ---- gr_freq_xlating_fir_filter_XXX on a whole stream with its history zeros in front ----
template <class IN, class TAP>
static std::vector<cf> xlating_ref(int D, const std::vector<TAP> &proto, double fc, double fs, const std::vector<IN> &xh,
                                   size_t nout)
{
    float fwT0 = 2 * M_PI * fc / fs;                                   // build_composite_fir (.cc.t:72-83)
    std::vector<cf> ctaps(proto.size());
    for (unsigned i = 0; i < proto.size(); i++) ctaps[i] = proto[i] * exp(cf(0, i * fwT0));
    const std::vector<cf> d = ctaps;                                   // set_taps(gr_reverse(ctaps)): d_taps = ctaps
    cf incr = exp(cf(0, fwT0 * D));
    incr = incr / std::abs(incr);                                      // gr_rotator::set_phase_incr
    cf phase = 1;
    unsigned counter = 0;
    std::vector<cf> y(nout);
    for (size_t n = 0; n < nout; ++n) {
        cf v;
        if constexpr (std::is_same<IN, cf>::value) {
            v = 0;
            cf acc0 = 0, acc1 = 0;                                     // gr_fir_ccc_generic
            unsigned i = 0, m = (d.size() / 2) * 2;
            for (i = 0; i < m; i += 2) { acc0 += d[i] * xh[n * D + i]; acc1 += d[i + 1] * xh[n * D + i + 1]; }
            for (; i < d.size(); i++) acc0 += d[i] * xh[n * D + i];
            v = acc0 + acc1;
        } else {
            v = fir_cc_one(d, xh.data() + n * D);
        }
        y[n] = v * phase;                                              // gr_rotator::rotate (gr_rotator.h:40-50)
        phase *= incr;
        if ((++counter % 512) == 0) phase /= std::abs(phase);
    }
    return y;
}

static int fails = 0;
static void report(const std::string &what, const void *a, const void *b, size_t bytes)
{
    const bool ok = memcmp(a, b, bytes) == 0;
    std::cout << what << ": " << (ok ? "ok" : "MISMATCH") << "\n";
    if (!ok) fails++;
}

template <class IN> static std::vector<IN> make_input(std::mt19937 &rng, size_t n)
{
    std::vector<IN> x(n);
    std::normal_distribution<float> nd(0.f, 1.f);
    std::uniform_int_distribution<int> ud(-32768, 32767);
    for (auto &v : x) {
        if constexpr (std::is_same<IN, short>::value) v = (short)ud(rng);
        else if constexpr (std::is_same<IN, float>::value) v = nd(rng) * 3000.f;
        else v = cf(nd(rng), nd(rng));
    }
    return x;
}
template <class TAP> static std::vector<TAP> make_taps(std::mt19937 &rng, size_t n)
{
    std::normal_distribution<float> nd(0.f, 1.f);
    std::vector<TAP> t(n);
    for (auto &v : t) {
        if constexpr (std::is_same<TAP, float>::value) v = nd(rng) / (float)n;
        else v = cf(nd(rng), nd(rng)) / (float)n;
    }
    return t;
}

// a block under the executor: whole stream with history zeros in front
template <class IN, class OUT, class SPTR> static std::vector<OUT> run_block(SPTR b, const std::vector<IN> &x)
{
    grhip_linear_flowgraph fg(4099);
    fg.connect(b);
    std::vector<unsigned char> y = fg.run(x.data(), x.size());
    std::vector<OUT> o(y.size() / sizeof(OUT));
    memcpy(o.data(), y.data(), o.size() * sizeof(OUT));
    return o;
}

template <class IN, class TAP, class MAKE>
static void check_xlating(const char *name, MAKE make, std::mt19937 &rng, int D, int ntaps)
{
    const std::vector<TAP> proto = make_taps<TAP>(rng, ntaps);
    const size_t nout = 5000;
    const std::vector<IN> x = make_input<IN>(rng, nout * D);
    std::vector<IN> xh(ntaps - 1, IN());
    xh.insert(xh.end(), x.begin(), x.end());
    const std::vector<cf> want = xlating_ref<IN, TAP>(D, proto, 1234.0, 48000.0, xh, nout);
    const std::vector<cf> got = run_block<IN, cf>(make(D, proto, 1234.0, 48000.0, 0), x);
    report(std::string(name) + " D=" + std::to_string(D) + " taps=" + std::to_string(ntaps), got.data(), want.data(),
           got.size() == want.size() ? want.size() * sizeof(cf) : 0);
    if (got.size() != want.size()) fails++;
}

template <class IN, class OUT, class TAP, class SEAM, class MAKE, class ONE>
static void check_fir(const char *name, MAKE make, std::mt19937 &rng, int D, int ntaps, ONE one)
{
    const std::vector<TAP> taps = make_taps<TAP>(rng, ntaps);
    const size_t nout = 3000;
    const std::vector<IN> x = make_input<IN>(rng, nout * D);
    std::vector<IN> xh(ntaps - 1, IN());
    xh.insert(xh.end(), x.begin(), x.end());
    const std::vector<TAP> d = rev(taps);
    std::vector<OUT> want(nout);
    for (size_t n = 0; n < nout; ++n) want[n] = one(d, xh.data() + n * D);
    const std::vector<OUT> got = run_block<IN, OUT>(make(D, taps, 0), x);
    report(std::string(name) + " D=" + std::to_string(D) + " taps=" + std::to_string(ntaps), got.data(), want.data(),
           got.size() == want.size() ? want.size() * sizeof(OUT) : 0);
    if (got.size() != want.size()) fails++;
    // the kernel-level seam, as qa_gr_fir_XXX.cc runs every implementation: filterNdec against the generic one
    SEAM seam(taps);
    std::vector<OUT> s(nout / D);
    seam.filterNdec(s.data(), xh.data(), s.size(), D);
    report(std::string("gr_fir_") + &name[11] + "_hip filterNdec D=" + std::to_string(D), s.data(), want.data(), s.size() * sizeof(OUT));
    OUT one_out = seam.filter(xh.data());
    report(std::string("gr_fir_") + &name[11] + "_hip filter", &one_out, &want[0], sizeof(OUT));
}

int main()
{
    try {
        grhip_detail::check(grhip_set_default_mode(GRHIP_MODE_GENERIC));
        std::mt19937 rng(12345);
        for (int D : {1, 4, 3}) {
            for (int T : {1, 7, 64}) {
                check_fir<float, cf, cf, gr_fir_fcc_hip>("fir_filter_fcc", grhip_make_fir_filter_fcc, rng, D, T,
                                                         [](const std::vector<cf> &d, const float *x) { return fir_cc_one(d, x); });
                check_fir<short, cf, cf, gr_fir_scc_hip>("fir_filter_scc", grhip_make_fir_filter_scc, rng, D, T,
                                                         [](const std::vector<cf> &d, const short *x) { return fir_cc_one(d, x); });
                check_fir<float, short, float, gr_fir_fsf_hip>("fir_filter_fsf", grhip_make_fir_filter_fsf, rng, D, T, fir_fsf_one);
            }
        }
        for (int D : {4, 1, 5}) {
            const int T = D == 4 ? 256 : 33;
            check_xlating<cf, float>("freq_xlating_fir_filter_ccf", grhip_make_freq_xlating_fir_filter_ccf, rng, D, T);
            check_xlating<float, float>("freq_xlating_fir_filter_fcf", grhip_make_freq_xlating_fir_filter_fcf, rng, D, T);
            check_xlating<float, cf>("freq_xlating_fir_filter_fcc", grhip_make_freq_xlating_fir_filter_fcc, rng, D, T);
            check_xlating<short, float>("freq_xlating_fir_filter_scf", grhip_make_freq_xlating_fir_filter_scf, rng, D, T);
            check_xlating<short, cf>("freq_xlating_fir_filter_scc", grhip_make_freq_xlating_fir_filter_scc, rng, D, T);
        }
        // the sysconfig table gets one more entry per signature
        std::vector<gr_fir_fcc_info> fi; grhip_fir_sysconfig::get_gr_fir_fcc_info(&fi);
        std::vector<gr_fir_scc_info> si; grhip_fir_sysconfig::get_gr_fir_scc_info(&si);
        std::vector<gr_fir_fsf_info> ti; grhip_fir_sysconfig::get_gr_fir_fsf_info(&ti);
        if (fi.size() != 1 || si.size() != 1 || ti.size() != 1 || std::string(fi[0].name) != "hip-gfx950") fails++;
        std::cout << (fails ? "FAIL" : "all ok") << "\n";
        return fails ? 1 : 0;
    } catch (const std::exception &e) {
        std::cerr << "xlating_test: " << e.what() << "\n";
        return 1;
    }
}
