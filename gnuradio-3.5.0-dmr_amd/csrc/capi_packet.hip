// capi_packet.hip -- C ABI of the packet layer: digital_crc32 / digital_update_crc32 (gr-digital/lib/digital_crc32.cc:45-134)
// over device and host buffers, make_packet (gr-digital/python/packet_utils.py:104-172) and unmake_packet (:175-194,
// gr-digital/python/crc.py:26-38) in batches, and the whitening table (:198-454), which is generated (csrc/gf2.h).
#include <climits>
#include <cmath>
#include <vector>

#include "packet.h"
#include "stream_block.h"

using namespace grhip;

namespace {

int upload_whitening(DevBuf &d)
{
    std::vector<unsigned char> t(WHITEN_LEN);
    whitening_table(t.data());
    int rc = d.reserve(WHITEN_LEN);
    if (rc) return rc;
    GRHIP_HIP(hipMemcpy(d.p, t.data(), WHITEN_LEN, hipMemcpyHostToDevice));
    return GRHIP_OK;
}

}  // namespace

struct grhip_crc32 : HandleBase {
    long long passes_per_wg = 0;        // 0: chosen per call
    DevBuf d_partial, d_crc;

    int init(int dev)
    {
        int rc = init_device(dev);
        if (rc) return rc;
        return d_crc.reserve(sizeof(unsigned));
    }
    int update_device(unsigned crc_in, unsigned final_xor, const void *d_buf, long long len, unsigned *crc, void *stream)
    {
        if (!crc) return fail(GRHIP_EINVAL, "null crc");
        if (len < 0 || len > INT_MAX) return fail(GRHIP_EINVAL, "crc32: len must be 0 .. 2^31 - 1");
        if (len && !d_buf) return fail(GRHIP_EINVAL, "null buffer");
        int rc = bind();
        if (rc) return rc;
        hipStream_t st = pick(stream);
        std::lock_guard<std::mutex> lk(setter_mutex);
        const CrcSplit s = crc_split(d_buf, len, passes_per_wg, device_cus());
        if ((rc = d_partial.reserve((size_t)(s.groups + 1) * sizeof(unsigned)))) return rc;
        if ((rc = crc32_launch((const unsigned char *)d_buf, len, s, crc_in, final_xor, d_partial.as<unsigned>(), d_crc.as<unsigned>(), st)))
            return rc;
        GRHIP_HIP(hipMemcpyAsync(crc, d_crc.p, sizeof(unsigned), hipMemcpyDeviceToHost, st));
        GRHIP_HIP(hipStreamSynchronize(st));
        return GRHIP_OK;
    }
    int update_host(unsigned crc_in, unsigned final_xor, const void *buf, long long len, unsigned *crc)
    {
        if (len < 0 || len > INT_MAX) return fail(GRHIP_EINVAL, "crc32: len must be 0 .. 2^31 - 1");
        if (len && !buf) return fail(GRHIP_EINVAL, "null buffer");
        int rc = bind();
        if (rc) return rc;
        if ((rc = stage_in.reserve((size_t)len + 16))) return rc;
        if (len) GRHIP_H2D(this, stage_in.p, buf, (size_t)len, own_stream);
        return update_device(crc_in, final_xor, stage_in.p, len, crc, own_stream);
    }
};

struct grhip_packet_maker : HandleBase {
    PacketFormat f{};
    int sps = 1, bps = 1;
    bool pad = true;
    DevBuf d_mask, d_jobs, d_out;

    int init(const char *access_code, double samples_per_symbol, int bits_per_symbol, int pad_for_usrp, int whitening, int dev)
    {
        // more than 64 characters is refused: the correlator takes 64 (a stated deviation)
        f.access_bytes = pack_access_code(access_code, f.access);
        if (f.access_bytes < 0) return fail(GRHIP_EINVAL, "packet_maker: access_code must be 1 .. 64 characters '0' or '1'");   // :121-122
        if (!std::isfinite(samples_per_symbol) || samples_per_symbol < 1.0 || samples_per_symbol > 65536.0)
            return fail(GRHIP_EINVAL, "packet_maker: int(samples_per_symbol) must be 1 .. 65536");
        if (bits_per_symbol < 1 || bits_per_symbol > 65536) return fail(GRHIP_EINVAL, "packet_maker: bits_per_symbol must be 1 .. 65536");
        sps = (int)samples_per_symbol;                          // int(samples_per_symbol), :146
        bps = bits_per_symbol;
        pad = pad_for_usrp != 0;
        f.whitening = whitening != 0;
        f.byte_modulus = 0;
        if (pad) {
            const long long bm = packet_byte_modulus(sps, bps);
            if (bm <= 0) return fail(GRHIP_EINVAL, "packet_maker: samples_per_symbol and bits_per_symbol leave a byte modulus of 0");
            f.byte_modulus = (unsigned)bm;
        }
        int rc = init_device(dev);
        if (rc) return rc;
        return upload_whitening(d_mask);
    }
    int plan(int n, const int *lengths, const int *whitener_offsets, grhip_packet_job *jobs, long long *total_in, long long *total_out)
    {
        if (n < 0) return fail(GRHIP_EINVAL, "negative packet count");
        if (n && (!lengths || !jobs)) return fail(GRHIP_EINVAL, "null argument");
        static_assert(sizeof(grhip_packet_job) == sizeof(PacketJob) && sizeof(PacketJob) == 16, "job records are 16 bytes");
        if (const char *bad = packet_plan(n, lengths, whitener_offsets, f.access_bytes, sps, bps, pad, (PacketJob *)jobs, total_in, total_out))
            return fail(GRHIP_EINVAL, "packet_maker: %s", bad);
        return GRHIP_OK;
    }
    int work_device(int n, const void *d_jobs_in, const void *d_payloads, void *d_packets, void *stream)
    {
        const int c = check_count(n);
        if (c <= 0) return c;
        if (!d_jobs_in || !d_packets) return fail(GRHIP_EINVAL, "null buffer");      // payloads may all be empty
        if (!aligned(d_jobs_in, 4)) return fail(GRHIP_EINVAL, "packet_maker: job records not aligned");
        int rc = bind();
        if (rc) return rc;
        return packet_make_launch(n, (const PacketJob *)d_jobs_in, (const unsigned char *)d_payloads, (unsigned char *)d_packets, f,
                                  d_mask.as<unsigned char>(), pick(stream));
    }
    // host buffers: payloads back to back in, packets back to back out
    int work(int n, const int *lengths, const int *whitener_offsets, const void *payloads, void *out, long long out_capacity, long long *total)
    {
        if (!total) return fail(GRHIP_EINVAL, "null total");
        *total = 0;
        const int c = check_count(n);
        if (c <= 0) return c;
        std::vector<PacketJob> jobs((size_t)n);
        long long tin = 0, tout = 0;
        int rc = plan(n, lengths, whitener_offsets, (grhip_packet_job *)jobs.data(), &tin, &tout);
        if (rc) return rc;
        if (out_capacity < tout) return fail(GRHIP_EINVAL, "packet_maker: the packets take %lld bytes, out_capacity is %lld", tout, out_capacity);
        if (!out || (tin && !payloads)) return fail(GRHIP_EINVAL, "null buffer");
        if ((rc = bind())) return rc;
        std::lock_guard<std::mutex> lk(setter_mutex);
        if ((rc = d_jobs.reserve(jobs.size() * sizeof(PacketJob))) || (rc = stage_in.reserve((size_t)tin + 16)) ||
            (rc = stage_out.reserve((size_t)tout + 16)))
            return rc;
        hipStream_t st = own_stream;
        GRHIP_HIP(hipMemcpyAsync(d_jobs.p, jobs.data(), jobs.size() * sizeof(PacketJob), hipMemcpyHostToDevice, st));
        if (tin) GRHIP_H2D(this, stage_in.p, payloads, (size_t)tin, st);
        if ((rc = work_device(n, d_jobs.p, stage_in.p, stage_out.p, st)) < 0) return rc;
        GRHIP_D2H(this, out, stage_out.p, (size_t)tout, st);
        GRHIP_HIP(hipStreamSynchronize(st));
        *total = tout;
        return GRHIP_OK;
    }
};

struct grhip_packet_check : HandleBase {
    DevBuf d_mask;
    int init(int dev)
    {
        int rc = init_device(dev);
        if (rc) return rc;
        return upload_whitening(d_mask);
    }
    int work_device(int n_streams, int max_msgs, const grhip_packet_rec *d_recs, long long rec_stride, const unsigned *d_counts,
                    int count_stride_words, const void *d_pool, long long pool_stride, int dewhitening, void *d_payload_out,
                    unsigned char *d_ok, void *stream)
    {
        if (n_streams < 0 || max_msgs < 0) return fail(GRHIP_EINVAL, "negative count");
        if (n_streams == 0 || max_msgs == 0) return GRHIP_OK;
        if (!d_recs || !d_pool || !d_payload_out || !d_ok) return fail(GRHIP_EINVAL, "null buffer");
        if (!aligned(d_recs, 4) || !aligned(d_counts, 4)) return fail(GRHIP_EINVAL, "packet_check: records or counts not aligned");
        if (rec_stride < 0 || pool_stride < 0 || count_stride_words < 0) return fail(GRHIP_EINVAL, "negative stride");
        if (n_streams > 1 && rec_stride < max_msgs) return fail(GRHIP_EINVAL, "packet_check: rec_stride shorter than max_msgs");
        static_assert(sizeof(grhip_packet_rec) == sizeof(PacketJob), "message records are 16 bytes");
        int rc = bind();
        if (rc) return rc;
        return packet_check_launch(n_streams, max_msgs, (const PacketJob *)d_recs, rec_stride, d_counts, count_stride_words,
                                   (const unsigned char *)d_pool, pool_stride, dewhitening != 0, (unsigned char *)d_payload_out, d_ok,
                                   d_mask.as<unsigned char>(), pick(stream));
    }
};

extern "C" {

#define GRHIP_PK_NULL(h) if (!(h)) return fail(GRHIP_EINVAL, "null handle")

int grhip_whitening_table(unsigned char *table, size_t capacity)
{
    if (!table || capacity < (size_t)WHITEN_LEN) return fail(GRHIP_EINVAL, "whitening_table: room for 4096 bytes");
    whitening_table(table);
    return WHITEN_LEN;
}

int grhip_crc32_create(grhip_crc32 **h, int device)
{
    if (!h) return fail(GRHIP_EINVAL, "null argument");
    return make_handle(h, [&](grhip_crc32 *b) { return b->init(device); });
}
void grhip_crc32_destroy(grhip_crc32 *h) { destroy_handle(h); }
int grhip_crc32_set_segment_bytes(grhip_crc32 *h, long long bytes)
{
    GRHIP_PK_NULL(h);
    if (bytes < 0) return fail(GRHIP_EINVAL, "negative segment");
    std::lock_guard<std::mutex> lk(h->setter_mutex);
    h->passes_per_wg = bytes == 0 ? 0 : (bytes + CRC_PASS_BYTES - 1) / CRC_PASS_BYTES;
    return GRHIP_OK;
}
int grhip_crc32_compute_device(grhip_crc32 *h, const void *d_buf, long long len, unsigned *crc, void *stream)
{
    GRHIP_PK_NULL(h);
    return h->update_device(0xffffffffu, 0xffffffffu, d_buf, len, crc, stream);      // digital_crc32.cc:133
}
int grhip_crc32_update_device(grhip_crc32 *h, unsigned crc_in, const void *d_buf, long long len, unsigned *crc, void *stream)
{
    GRHIP_PK_NULL(h);
    return h->update_device(crc_in, 0u, d_buf, len, crc, stream);
}
int grhip_crc32_compute(grhip_crc32 *h, const void *buf, long long len, unsigned *crc)
{
    GRHIP_PK_NULL(h);
    return h->update_host(0xffffffffu, 0xffffffffu, buf, len, crc);
}
int grhip_crc32_update(grhip_crc32 *h, unsigned crc_in, const void *buf, long long len, unsigned *crc)
{
    GRHIP_PK_NULL(h);
    return h->update_host(crc_in, 0u, buf, len, crc);
}

int grhip_packet_maker_create(grhip_packet_maker **h, const char *access_code, double samples_per_symbol, int bits_per_symbol,
                              int pad_for_usrp, int whitening, int device)
{
    if (!h) return fail(GRHIP_EINVAL, "null argument");
    return make_handle(h, [&](grhip_packet_maker *b) {
        return b->init(access_code, samples_per_symbol, bits_per_symbol, pad_for_usrp, whitening, device);
    });
}
void grhip_packet_maker_destroy(grhip_packet_maker *h) { destroy_handle(h); }
long long grhip_packet_maker_packet_bytes(grhip_packet_maker *h, int payload_len)
{
    GRHIP_PK_NULL(h);
    if (const char *bad = packet_refusal(payload_len, 0)) return fail(GRHIP_EINVAL, "packet_maker: %s", bad);
    return packet_bytes(h->f.access_bytes, payload_len, h->sps, h->bps, h->pad);
}
int grhip_packet_maker_plan(grhip_packet_maker *h, int n, const int *lengths, const int *whitener_offsets, grhip_packet_job *jobs_out,
                            long long *total_in, long long *total_out)
{
    GRHIP_PK_NULL(h);
    return h->plan(n, lengths, whitener_offsets, jobs_out, total_in, total_out);
}
int grhip_packet_maker_work_device(grhip_packet_maker *h, int n, const grhip_packet_job *d_jobs, const void *d_payloads, void *d_out,
                                   void *stream)
{
    GRHIP_PK_NULL(h);
    return h->work_device(n, d_jobs, d_payloads, d_out, stream);
}
int grhip_packet_maker_work(grhip_packet_maker *h, int n, const int *lengths, const int *whitener_offsets, const void *payloads, void *out,
                            long long out_capacity, long long *total)
{
    GRHIP_PK_NULL(h);
    return h->work(n, lengths, whitener_offsets, payloads, out, out_capacity, total);
}

int grhip_packet_check_create(grhip_packet_check **h, int device)
{
    if (!h) return fail(GRHIP_EINVAL, "null argument");
    return make_handle(h, [&](grhip_packet_check *b) { return b->init(device); });
}
void grhip_packet_check_destroy(grhip_packet_check *h) { destroy_handle(h); }
int grhip_packet_check_work_device(grhip_packet_check *h, int n_streams, int max_msgs, const grhip_packet_rec *d_recs, long long rec_stride,
                                   const unsigned *d_counts, int count_stride_words, const void *d_pool, long long pool_stride,
                                   int dewhitening, void *d_payload_out, unsigned char *d_ok, void *stream)
{
    GRHIP_PK_NULL(h);
    return h->work_device(n_streams, max_msgs, d_recs, rec_stride, d_counts, count_stride_words, d_pool, pool_stride, dewhitening,
                          d_payload_out, d_ok, stream);
}

#undef GRHIP_PK_NULL

}  // extern "C"
