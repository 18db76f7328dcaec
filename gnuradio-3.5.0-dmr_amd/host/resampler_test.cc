// resampler_test -- drives grhip_interp_fir_filter_XXX and grhip_rational_resampler_base_XXX (grhip_blocks.h) through
// the stand-in executor (grhip_executor.h) in scheduler-style calls and writes what the block produced, for
// tests/test_gpu_resampler.py.
//
//   resampler_test interp|rational ccf|fff|ccc <I> <D> generic|fast <taps.bin> <in.bin> <out.bin>
//   resampler_test errors
// taps.bin holds float taps (complex pairs for ccc); D is ignored by interp.
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
    const std::vector<float> taps(10, 0.5f);
    try { grhip_make_rational_resampler_base_ccf(0, 2, taps); fails++; }
    catch (const std::out_of_range &) {}
    try { grhip_make_rational_resampler_base_fff(3, 0, taps); fails++; }
    catch (const std::out_of_range &) {}
    try { grhip_make_interp_fir_filter_ccc(0, std::vector<gr_complex>(4)); fails++; }
    catch (const std::out_of_range &) {}
    try { grhip_make_interp_fir_filter_ccf(3, std::vector<float>()); fails++; }
    catch (const std::invalid_argument &) {}
    grhip_rational_resampler_base_ccf_sptr r = grhip_make_rational_resampler_base_ccf(3, 2, taps);
    if (r->history() != 1 || r->resampler_history() != 4 || r->relative_rate() != 1.5) fails++;   // nt = 12/3
    gr_vector_int req(1);
    r->forecast(100, req);
    if (req[0] != (int)(101.0 * 2 / 3) + 3) fails++;
    grhip_interp_fir_filter_fff_sptr i = grhip_make_interp_fir_filter_fff(4, taps);
    if (i->history() != 3 || i->output_multiple() != 4 || i->relative_rate() != 4.0) fails++;    // nt = 12/4
    i->forecast(40, req);
    if (req[0] != 10 + 2) fails++;
    std::cout << "errors test: " << (fails ? "FAIL" : "ok") << "\n";
    return fails;
}

template <class SPTR> static void setup(grhip_linear_flowgraph &fg, SPTR b, int mode)
{
    b->set_mode(mode);
    fg.connect(b);
}

int main(int argc, char **argv)
{
    try {
        if (argc == 2 && std::string(argv[1]) == "errors") return errors();
        if (argc != 9) {
            std::cerr << "usage: " << argv[0] << " interp|rational ccf|fff|ccc I D generic|fast taps.bin in.bin out.bin\n";
            return 2;
        }
        const bool interp = std::string(argv[1]) == "interp";
        const std::string kind = argv[2];
        const unsigned I = (unsigned)strtoul(argv[3], nullptr, 10), D = (unsigned)strtoul(argv[4], nullptr, 10);
        const int mode = std::string(argv[5]) == "generic" ? GRHIP_MODE_GENERIC : GRHIP_MODE_FAST;
        std::vector<unsigned char> tb = read_file(argv[6]), xb = read_file(argv[7]);
        std::vector<float> ft(tb.size() / 4);
        memcpy(ft.data(), tb.data(), ft.size() * 4);
        std::vector<gr_complex> ct(ft.size() / 2);
        memcpy(ct.data(), tb.data(), ct.size() * 8);
        // the interpolator insists on whole output multiples (the reference's scheduler never asks for less)
        grhip_linear_flowgraph fg(1 << 16, !interp);
        const size_t item = kind == "fff" ? sizeof(float) : sizeof(gr_complex);
        if (interp) {
            if (kind == "ccf") setup(fg, grhip_make_interp_fir_filter_ccf(I, ft), mode);
            else if (kind == "fff") setup(fg, grhip_make_interp_fir_filter_fff(I, ft), mode);
            else setup(fg, grhip_make_interp_fir_filter_ccc(I, ct), mode);
        } else {
            if (kind == "ccf") setup(fg, grhip_make_rational_resampler_base_ccf(I, D, ft), mode);
            else if (kind == "fff") setup(fg, grhip_make_rational_resampler_base_fff(I, D, ft), mode);
            else setup(fg, grhip_make_rational_resampler_base_ccc(I, D, ct), mode);
        }
        std::vector<unsigned char> y = fg.run(xb.data(), xb.size() / item);
        FILE *fo = fopen(argv[8], "wb");
        if (!fo || fwrite(y.data(), 1, y.size(), fo) != y.size()) throw std::runtime_error("cannot write output");
        fclose(fo);
        std::cout << y.size() / item << " items\n";
        return 0;
    } catch (const std::exception &e) {
        std::cerr << "resampler_test: " << e.what() << "\n";
        return 1;
    }
}
