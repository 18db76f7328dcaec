// arb_resampler_test -- drives grhip_pfb_arb_resampler_{ccf,fff} (grhip_blocks.h) through the stand-in executor
// (grhip_executor.h) in scheduler-style calls and writes what the block produced, for tests/test_gpu_arb_resampler.py.
//
//   arb_resampler_test ccf|fff <rate> <filter_size> generic|fast <taps.f32> <in.bin> <out.bin>
//   arb_resampler_test errors
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "grhip_blocks.h"
#include "grhip_executor.h"

static std::vector<unsigned char> read_file(const char *path)
{
    std::vector<unsigned char> v;
    FILE *f = fopen(path, "rb");
    if (!f) throw std::runtime_error(std::string("cannot open ") + path);
    unsigned char buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}

static int errors()
{
    int fails = 0;
    const std::vector<float> taps(64, 0.5f);
    // the preconditions the reference leaves undefined are refused (include/grhip.h)
    try { grhip_make_pfb_arb_resampler_ccf(0.5f, std::vector<float>()); fails++; }
    catch (const std::invalid_argument &) {}
    try { grhip_make_pfb_arb_resampler_fff(0.5f, taps, 0); fails++; }
    catch (const std::invalid_argument &) {}
    try { grhip_make_pfb_arb_resampler_ccf(0.0f, taps); fails++; }
    catch (const std::invalid_argument &) {}
    try { grhip_make_pfb_arb_resampler_fff(-1.0f, taps); fails++; }
    catch (const std::invalid_argument &) {}
    grhip_pfb_arb_resampler_ccf_sptr c = grhip_make_pfb_arb_resampler_ccf(0.5f, taps);
    if (c->history() != 3 || c->relative_rate() != 0.5) fails++;         // tpf = 2
    gr_vector_int req(1);
    c->forecast(100, req);
    if (req[0] != 102) fails++;                                           // gr_block's default
    c->set_rate(1.25f);
    if (std::fabs(c->relative_rate() - 1.25) > 1e-9) fails++;
    try { c->set_rate(NAN); fails++; }
    catch (const std::invalid_argument &) {}
    grhip_pfb_arb_resampler_fff_sptr f = grhip_make_pfb_arb_resampler_fff(3.0f, std::vector<float>(100, 1.f), 16);
    if (f->history() != 8 || f->relative_rate() != 3.0) fails++;         // tpf = ceil(100 / 16) = 7
    std::cout << "errors test: " << (fails ? "FAIL" : "ok") << "\n";
    return fails;
}

int main(int argc, char **argv)
{
    try {
        if (argc == 2 && std::string(argv[1]) == "errors") return errors();
        if (argc != 8) {
            std::cerr << "usage: " << argv[0] << " ccf|fff rate filter_size generic|fast taps.f32 in.bin out.bin\n";
            return 2;
        }
        const bool cplx = std::string(argv[1]) == "ccf";
        const float rate = strtof(argv[2], nullptr);
        const unsigned R = (unsigned)strtoul(argv[3], nullptr, 10);
        const int mode = std::string(argv[4]) == "generic" ? GRHIP_MODE_GENERIC : GRHIP_MODE_FAST;
        std::vector<unsigned char> tb = read_file(argv[5]), xb = read_file(argv[6]);
        std::vector<float> taps(tb.size() / 4);
        memcpy(taps.data(), tb.data(), taps.size() * 4);
        grhip_linear_flowgraph fg(1 << 16);
        size_t item;
        if (cplx) {
            grhip_pfb_arb_resampler_ccf_sptr b = grhip_make_pfb_arb_resampler_ccf(rate, taps, R);
            b->set_mode(mode);
            fg.connect(b);
            item = sizeof(gr_complex);
        } else {
            grhip_pfb_arb_resampler_fff_sptr b = grhip_make_pfb_arb_resampler_fff(rate, taps, R);
            b->set_mode(mode);
            fg.connect(b);
            item = sizeof(float);
        }
        std::vector<unsigned char> y = fg.run(xb.data(), xb.size() / item);
        FILE *fo = fopen(argv[7], "wb");
        if (!fo || fwrite(y.data(), 1, y.size(), fo) != y.size()) throw std::runtime_error("cannot write output");
        fclose(fo);
        std::cout << y.size() / item << " items\n";
        return 0;
    } catch (const std::exception &e) {
        std::cerr << "arb_resampler_test: " << e.what() << "\n";
        return 1;
    }
}
