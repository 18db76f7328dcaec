// constellation_blocks.h -- launchers of the blocks behind timing recovery (internal): digital_constellation_decoder_cb,
// digital_constellation_receiver_cb, gr_diff_decoder_bb, gr_map_bb and the fused tail of constellation_demod_cb.
#pragma once
#include <hip/hip_runtime.h>

#include "carrier.h"
#include "constellation.h"
#include "grhip_internal.h"

// the constellation handle of the C ABI (csrc/capi_constellation.hip makes them; the blocks copy what they are given)
struct grhip_constellation {
    grhip::Constellation c;
};

namespace grhip {

// how the receiver's walk forms decision and error
enum { RX_FORM_GENERIC = 0, RX_FORM_CARTESIAN = 1, RX_FORM_ANGLE = 2 };

// what a stream remembers: gri_control_loop's d_phase and d_freq, and (constellation_demod_cb) the symbol in front of
// the next call's first one, which gr_diff_decoder_bb keeps as history
struct ConstState {
    float phase, freq;
    unsigned prev, pad;
};

// a constellation on the device.  points: arity * dim; sval: the sector table (psk, rect) as bytes; ang: the angle of
// the point that index i decides for, i a sector (psk) or a symbol (bpsk, qpsk, dqpsk, 8psk).
struct ConstDev {
    int kind;
    unsigned arity, dim, n_sectors, n_real, n_imag, n_ang;
    float w_real, w_imag;
    const cfloat *points;
    const unsigned char *sval;
    const float *ang;
};

struct ReceiverLaunch {
    const float2 *in;               // [S][n] gr_complex
    unsigned char *sym;             // [S][n] symbols, or [S][n * k] bits when tail is set
    float *err, *phase, *freq;      // [S][n] each, all three or none
    int n, nstreams;
    CarrierParams p;
    ConstState *state;              // [S]
    // the fused tail (constellation_demod_cb, engine 1): diff_decoder_bb(arity) if differential, map_bb(map) if map,
    // unpack_k_bits_bb(k)
    bool tail, differential;
    const unsigned char *map;       // 256 bytes on the device, or null
    unsigned k;
};

// form: RX_FORM_*; RX_FORM_ANGLE needs c.ang, and a kind whose decision depends on the angle alone
int receiver_launch(int form, const ConstDev &c, const ReceiverLaunch &a, hipStream_t st);
// [S][n * dim] complex in, [S][n] bytes out: the host's decision_maker byte for byte
int decoder_launch(const ConstDev &c, const float2 *in, unsigned char *out, int n, int nstreams, hipStream_t st);
// out[i] = (unsigned)(in[i] - in[i-1]) % modulus per stream; *(prev + s * prev_stride) is in[-1] and becomes in[n-1]
int diff_decoder_launch(const unsigned char *in, unsigned char *out, int n, int nstreams, unsigned modulus, unsigned *prev,
                        int prev_stride, hipStream_t st);
// out[i] = map[in[i]], map: 256 bytes on the device
int map_launch(const unsigned char *in, unsigned char *out, long long n, const unsigned char *map, hipStream_t st);

}  // namespace grhip
