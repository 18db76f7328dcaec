// capi_lfsr.hip -- C ABI of gr_scrambler_bb (general/gr_scrambler_bb.cc:30-57), gr_descrambler_bb
// (general/gr_descrambler_bb.cc:30-57) and gr_additive_scrambler_bb (general/gr_additive_scrambler_bb.cc:30-65), all on
// gri_lfsr (general/gri_lfsr.h:103-147).
//
// One handle type serves the three: S streams back to back, per stream the register (and d_bits) on the device, carried
// across calls.  GRHIP_MODE_GENERIC walks every stream serially with the reference's statements; every other mode runs
// the parallel kernels of csrc/lfsr_blocks.hip and gives the same bytes.
#include <vector>

#include "packet.h"
#include "stream_block.h"

using namespace grhip;

namespace {

struct LfsrBlock : StreamBlock {
    int kind = LFSR_SCRAMBLE;
    LfsrParams p{0, 0, 0, 0};
    // The scrambler's register feeds back, so a seed's bits above reg_len keep the OR of gri_lfsr.h:123 from being an
    // XOR until they have shifted out: the first LFSR_HEAD items of a stream's life are walked serially.  `age` counts
    // them; it is the same for every stream, as every call brings each stream the same number of items.
    // Only the parallel form's calls advance it, at once and whatever the launch then answers: it may lag behind the
    // stream's true age (after GENERIC calls, after a failed launch), which costs up to 32 items walked serially
    // that need not have been, never a wrong byte, since the serial walk is right at any age.
    int age = 0;
    DevBuf d_state, d_mats, d_scratch;

    const char *name() const { return kind == LFSR_SCRAMBLE ? "scrambler_bb" : kind == LFSR_DESCRAMBLE ? "descrambler_bb" : "additive_scrambler_bb"; }

    int restart()
    {
        age = 0;
        return fill_state(d_state, LfsrState{p.seed, 0u});      // gri_lfsr.h:104, d_bits(0)
    }
    int init(int k, int mask, int seed, int len, int count, int dev)
    {
        kind = k;
        if (len < 0 || (unsigned)len > LFSR_MAX_LEN)            // gri_lfsr.h:109-110 throws
            return fail(GRHIP_EINVAL, "%s: reg_len must be 0 .. 31", name());
        p = LfsrParams{(unsigned)mask, (unsigned)seed, (unsigned)len, count > 0 ? (unsigned)count : 0u};   // d_count > 0, .cc:56
        mode = default_mode();
        int rc = init_device(dev);
        if (rc) return rc;
        std::vector<unsigned> m((size_t)LFSR_MATS * 32);
        Gf2Mat pw = lfsr_matrix(p.mask, p.len);
        for (int j = 0; j < 31; ++j) {
            std::memcpy(&m[(size_t)(LFSR_MAT_POW + j) * 32], pw.c, sizeof(pw.c));
            pw = gf2_matmul(pw, pw);
        }
        Gf2Mat sc = gf2_matpow(lfsr_matrix(p.mask, p.len), LFSR_CHUNK);
        for (int j = 0; j < 8; ++j) {
            std::memcpy(&m[(size_t)(LFSR_MAT_SCAN + j) * 32], sc.c, sizeof(sc.c));
            sc = gf2_matmul(sc, sc);
        }
        const Gf2Mat tile = gf2_matpow(lfsr_matrix(p.mask, p.len), LFSR_TILE);
        std::memcpy(&m[(size_t)LFSR_MAT_TILE * 32], tile.c, sizeof(tile.c));
        if ((rc = d_mats.reserve(m.size() * sizeof(unsigned)))) return rc;
        GRHIP_HIP(hipMemcpy(d_mats.p, m.data(), m.size() * sizeof(unsigned), hipMemcpyHostToDevice));
        return restart();
    }
    int set_streams(int S)
    {
        return StreamBlock::set_streams(S, [&] { return restart(); });
    }
    int work_device(int n, const void *d_in, void *d_out, void *stream)
    {
        const int c = check_count(n);
        if (c <= 0) return c;
        int rc = check_io(d_in, 1, d_out, 1);
        if (rc) return rc;
        if ((rc = bind())) return rc;
        hipStream_t st = pick(stream);
        std::lock_guard<std::mutex> lk(setter_mutex);
        const size_t items = (size_t)nstreams * (size_t)n;
        if ((rc = check_apart(name(), d_in, items, d_out, items))) return rc;
        const unsigned char *in = (const unsigned char *)d_in;
        unsigned char *out = (unsigned char *)d_out;
        LfsrState *state = d_state.as<LfsrState>();
        if (!mode_fast(mode)) return lfsr_serial_launch(kind, in, out, n, 0, n, nstreams, p, state, st);
        long long first = 0;
        if (kind == LFSR_SCRAMBLE) {
            first = LFSR_HEAD - age < n ? LFSR_HEAD - age : n;
            if ((rc = lfsr_serial_launch(kind, in, out, n, 0, first, nstreams, p, state, st))) return rc;
            age += (int)first;
            if ((rc = d_scratch.reserve((size_t)nstreams * (size_t)lfsr_tiles(n - first) * sizeof(unsigned)))) return rc;
        }
        return lfsr_parallel_launch(kind, in, out, n, first, nstreams, p, state, d_mats.as<unsigned>(), d_scratch.as<unsigned>(), st);
    }
    int work(int n, const void *in, void *out)
    {
        return host_work(n, 1, in, (size_t)n, 1, out, 0, [&](void *d_in, void *d_out, hipStream_t st) {
            return work_device(n, d_in, d_out, st);
        });
    }
};

}  // namespace

struct grhip_scrambler_bb : LfsrBlock {};
struct grhip_descrambler_bb : LfsrBlock {};
struct grhip_additive_scrambler_bb : LfsrBlock {};

extern "C" {

#define GRHIP_LF_NULL(h) if (!(h)) return fail(GRHIP_EINVAL, "null handle")
#define GRHIP_LF_BLOCK(NAME)                                                                                          \
    void grhip_##NAME##_destroy(grhip_##NAME *h) { destroy_handle(h); }                                               \
    int grhip_##NAME##_set_mode(grhip_##NAME *h, int mode) { GRHIP_LF_NULL(h); return h->set_mode(mode); }            \
    int grhip_##NAME##_set_streams(grhip_##NAME *h, int nstreams) { GRHIP_LF_NULL(h); return h->set_streams(nstreams); } \
    int grhip_##NAME##_work(grhip_##NAME *h, int n, const void *in, void *out) { GRHIP_LF_NULL(h); return h->work(n, in, out); } \
    int grhip_##NAME##_work_device(grhip_##NAME *h, int n, const void *d_in, void *d_out, void *stream)               \
    {                                                                                                                 \
        GRHIP_LF_NULL(h);                                                                                             \
        return h->work_device(n, d_in, d_out, stream);                                                                \
    }

int grhip_scrambler_bb_create(grhip_scrambler_bb **h, int mask, int seed, int len, int device)
{
    if (!h) return fail(GRHIP_EINVAL, "null argument");
    return make_handle(h, [&](grhip_scrambler_bb *b) { return b->init(LFSR_SCRAMBLE, mask, seed, len, 0, device); });
}
GRHIP_LF_BLOCK(scrambler_bb)

int grhip_descrambler_bb_create(grhip_descrambler_bb **h, int mask, int seed, int len, int device)
{
    if (!h) return fail(GRHIP_EINVAL, "null argument");
    return make_handle(h, [&](grhip_descrambler_bb *b) { return b->init(LFSR_DESCRAMBLE, mask, seed, len, 0, device); });
}
GRHIP_LF_BLOCK(descrambler_bb)

int grhip_additive_scrambler_bb_create(grhip_additive_scrambler_bb **h, int mask, int seed, int len, int count, int device)
{
    if (!h) return fail(GRHIP_EINVAL, "null argument");
    return make_handle(h, [&](grhip_additive_scrambler_bb *b) { return b->init(LFSR_ADDITIVE, mask, seed, len, count, device); });
}
GRHIP_LF_BLOCK(additive_scrambler_bb)

#undef GRHIP_LF_BLOCK
#undef GRHIP_LF_NULL

}  // extern "C"
