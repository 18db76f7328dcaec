// pfb_synth_test -- drives grhip_pfb_synthesis_filterbank_ccf and grhip_pfb_interpolator_ccf (grhip_blocks.h) in
// scheduler-sized calls (4096 output items at most) and writes what the block produced, for
// tests/test_gpu_pfb_synth.py.
//
//   pfb_synth_test synth <numchans> <numsigs> generic|fast <taps.bin> <in.bin> <out.bin>
//   pfb_synth_test interp <interp> 1 generic|fast <taps.bin> <in.bin> <out.bin>
//   pfb_synth_test errors
// in.bin holds the numsigs streams one after the other (equal lengths).  The interpolator and a synthesis bank with
// one connected stream run under the stand-in executor (grhip_executor.h, one input per block); with more streams
// the bank is driven here the way the scheduler would: history() - 1 zeros in front of every stream, forecast(),
// general_work(), consume.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "grhip_blocks.h"
#include "grhip_executor.h"

static const int MAX_NOUTPUT = 4096;

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
    const std::vector<float> taps(30, 0.5f);
    try { grhip_make_pfb_synthesis_filterbank_ccf(0, taps); fails++; }
    catch (const std::invalid_argument &) {}
    try { grhip_make_pfb_synthesis_filterbank_ccf(4, std::vector<float>()); fails++; }
    catch (const std::invalid_argument &) {}
    try { grhip_make_pfb_interpolator_ccf(0, taps); fails++; }
    catch (const std::out_of_range &) {}
    try { grhip_make_pfb_interpolator_ccf(3, std::vector<float>()); fails++; }
    catch (const std::invalid_argument &) {}
    grhip_pfb_synthesis_filterbank_ccf_sptr s = grhip_make_pfb_synthesis_filterbank_ccf(4, taps);     // tpf = ceil(30/4)
    if (s->history() != 9 || s->taps_per_filter() != 8 || s->output_multiple() != 4 || s->relative_rate() != 4.0) fails++;
    if (s->input_signature()->min_streams() != 1 || s->input_signature()->max_streams() != 4) fails++;
    gr_vector_int req(4);
    s->forecast(400, req);
    if (req[0] != 100 + 8 || req[3] != 100 + 8) fails++;
    grhip_pfb_interpolator_ccf_sptr i = grhip_make_pfb_interpolator_ccf(4, taps);
    if (i->history() != 8 || i->output_multiple() != 4 || i->relative_rate() != 4.0) fails++;
    i->forecast(40, req);
    if (req[0] != 10 + 7) fails++;
    std::cout << "errors test: " << (fails ? "FAIL" : "ok") << "\n";
    return fails;
}

// numsigs streams of n items each through the bank, in calls of at most MAX_NOUTPUT outputs
static std::vector<gr_complex> run_bank(grhip_pfb_synthesis_filterbank_ccf_sptr b, const gr_complex *x, int numsigs,
                                        size_t n)
{
    const size_t hist = b->history() - 1;
    std::vector<std::vector<gr_complex>> in(numsigs);
    for (int s = 0; s < numsigs; ++s) {
        in[s].assign(hist, gr_complex(0, 0));
        in[s].insert(in[s].end(), x + (size_t)s * n, x + (size_t)(s + 1) * n);
    }
    std::vector<gr_complex> out;
    const int mult = b->output_multiple();
    size_t rd = 0;
    while (true) {
        const size_t avail = in[0].size() - rd;
        int nout = (MAX_NOUTPUT / mult) * mult;
        gr_vector_int req(numsigs);
        for (; nout >= mult; nout -= mult) {            // the largest request whose forecast fits
            b->forecast(nout, req);
            if ((size_t)req[0] <= avail) break;
        }
        if (nout < mult) break;
        const size_t old = out.size();
        out.resize(old + nout);
        gr_vector_int ninput(numsigs, (int)avail);
        gr_vector_const_void_star ins(numsigs);
        for (int s = 0; s < numsigs; ++s) ins[s] = in[s].data() + rd;
        gr_vector_void_star outs(1, out.data() + old);
        const int r = b->general_work(nout, ninput, ins, outs);
        if (r < 0) throw std::runtime_error("block returned " + std::to_string(r));
        out.resize(old + r);
        rd += b->consumed();
    }
    return out;
}

int main(int argc, char **argv)
{
    try {
        if (argc == 2 && std::string(argv[1]) == "errors") return errors();
        if (argc != 8) {
            std::cerr << "usage: " << argv[0] << " synth|interp N numsigs generic|fast taps.bin in.bin out.bin\n";
            return 2;
        }
        const bool synth = std::string(argv[1]) == "synth";
        const unsigned N = (unsigned)strtoul(argv[2], nullptr, 10);
        const int numsigs = atoi(argv[3]);
        const int mode = std::string(argv[4]) == "generic" ? GRHIP_MODE_GENERIC : GRHIP_MODE_FAST;
        std::vector<unsigned char> tb = read_file(argv[5]), xb = read_file(argv[6]);
        std::vector<float> taps(tb.size() / 4);
        memcpy(taps.data(), tb.data(), taps.size() * 4);
        std::vector<gr_complex> y;
        if (synth && numsigs > 1) {
            grhip_pfb_synthesis_filterbank_ccf_sptr b = grhip_make_pfb_synthesis_filterbank_ccf(N, taps);
            b->set_mode(mode);
            y = run_bank(b, reinterpret_cast<const gr_complex *>(xb.data()), numsigs,
                         xb.size() / sizeof(gr_complex) / numsigs);
        } else {
            // whole output multiples only (the reference's scheduler never asks for less)
            grhip_linear_flowgraph fg(MAX_NOUTPUT, false);
            if (synth) {
                grhip_pfb_synthesis_filterbank_ccf_sptr b = grhip_make_pfb_synthesis_filterbank_ccf(N, taps);
                b->set_mode(mode);
                fg.connect(b);
            } else {
                grhip_pfb_interpolator_ccf_sptr b = grhip_make_pfb_interpolator_ccf(N, taps);
                b->set_mode(mode);
                fg.connect(b);
            }
            std::vector<unsigned char> yb = fg.run(xb.data(), xb.size() / sizeof(gr_complex));
            y.resize(yb.size() / sizeof(gr_complex));
            memcpy(y.data(), yb.data(), y.size() * sizeof(gr_complex));
        }
        FILE *fo = fopen(argv[7], "wb");
        if (!fo || fwrite(y.data(), sizeof(gr_complex), y.size(), fo) != y.size()) throw std::runtime_error("cannot write output");
        fclose(fo);
        std::cout << y.size() << " items\n";
        return 0;
    } catch (const std::exception &e) {
        std::cerr << "pfb_synth_test: " << e.what() << "\n";
        return 1;
    }
}
