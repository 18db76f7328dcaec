// running_sum.h -- launchers of the sliding / running sum blocks (internal): gr_dc_blocker_ff / _cc,
// gr_moving_average_XX and gr_integrate_XX.
#pragma once
#include <hip/hip_runtime.h>

namespace grhip {

enum { RSUM_F = 0, RSUM_C = 1, RSUM_S = 2, RSUM_I = 3 };      // item type: float, gr_complex, short, int
inline size_t rsum_item(int type) { return type == RSUM_C ? 8 : type == RSUM_S ? 2 : 4; }

constexpr int RSUM_THREADS = 256;               // lanes per workgroup of the FAST window kernel
constexpr int RSUM_LDS_BYTES = 150 * 1024;      // what one workgroup of it may stage
constexpr int RSUM_MIN_TILE = 1024;             // outputs a tile keeps at least, whatever the halo
// The FAST kernel stages 256 R elements (R odd) per buffer: three buffers for dc_blocker (input, prefix, stage), two
// for moving_average.  The complex forms are the tightest: 150 KB / (3 * 8 B) = 6400 elements = 256 * 25 and
// 150 KB / (2 * 8 B) = 9600 -> 256 * 37 = 9472.  A long-form halo is 4 (D - 1), a moving average's length - 1:
constexpr int RSUM_DC_MAX_D = (6400 - RSUM_MIN_TILE) / 4 + 1;          // 1345
constexpr int RSUM_MA_MAX_LEN = 9472 - RSUM_MIN_TILE + 1;              // 8449
constexpr int RSUM_GEN_WIN = 256;               // samples the serial dc_blocker wave walks per window

// dc_blocker, both modes.  S streams of n items back to back in `in` and `out`.
//   GENERIC: state = S x dc_state_elems(D, stages) items: per stage the stage's last inputs (2 D for stage 0, which
//            also feeds the delayed signal; D for the others), then the stages' running sums y.
//   FAST:    hist_old / hist_new = S x halo items, halo = stages (D - 1): the last inputs before / after this call.
struct DcLaunch {
    const void *in;
    void *out;
    long long n;
    int nstreams, D, stages;        // stages: 2 (short form) or 4 (long form)
    void *state;
    const void *hist_old;
    void *hist_new;
};
__host__ __device__ inline size_t dc_state_elems(int D, int stages) { return (size_t)(stages + 1) * D + stages; }
int dc_blocker_launch(int type, bool fast, const DcLaunch &a, hipStream_t st);

// moving_average: n outputs from n + length - 1 inputs.  GENERIC restarts the sum every max_iter outputs (one reference
// work call each); FAST and the integer types form every window sum on its own.
struct MaLaunch {
    const void *in;
    void *out;
    long long n;
    int length, max_iter;
    float2 scale;                   // float: .x; complex: (.x, .y)
    int iscale;                     // short / int
};
int moving_average_launch(int type, bool fast, const MaLaunch &a, hipStream_t st);

// integrate: out[i] = sum of in[i decim .. i decim + decim - 1]
int integrate_launch(int type, bool fast, const void *in, void *out, long long n, int decim, hipStream_t st);

}  // namespace grhip
