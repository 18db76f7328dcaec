// logpwr_plan.h -- which calls of blks2.logpwrfft (logpwrfft.py:47-63) the fused FFT kernels can address (internal).
// Plain host arithmetic, no HIP: host/logpwr_plan_test.cc runs it on the CPU.
//
// fft16x_kernel (N = 32 ... 2048) carries VPG = 4096 / N vectors per workgroup step and loads them through ONE buffer
// descriptor: its base is the group's first kept frame, its range ends behind the group's last one, and a lane's 32-bit
// byte offset is the distance of its own frame from the first.  With a decimation n the frames of a group are n frames
// apart, and where a group runs over the end of a stream the next frame is a whole stream further on.  The fused path
// is taken while that range stays at or below LOGPWR_MAX_RANGE = 2^31 bytes (half of what the offset could hold: a lane
// past the last vector is given the range itself as its offset, and the instruction's own offsets come on top); beyond
// it the block runs keep_one_in_n, the transform, mag^2 and the averaging pass one after the other.
// For one stream the bound is exact: decimations up to (2^31 - N item) / ((VPG - 1) N item), which is 66 052 for complex
// and 132 104 for float items at N = 32, rising to 131 071 and 262 143 at N = 2048.
// fft4096_kernel and fft8192_kernel build a descriptor per vector from a 64-bit address: no such limit.
#pragma once

namespace grhip {

constexpr long long LOGPWR_MAX_RANGE = 1ll << 31;
constexpr long long LOGPWR_MAX_VECTORS = 0x7fffff00ll;      // streams x kept frames of one launch (an int in the kernels)

inline bool logpwr_native_size(long long N) { return N >= 32 && N <= 8192 && (N & (N - 1)) == 0; }

// upper bound of the descriptor range any group of the call needs, in bytes (exact for one stream); item = bytes per
// sample, n_frames = frames per stream in the input, n_out = kept frames per stream, n = decimation
inline long long logpwr_group_range(int N, int item, long long nstreams, long long n_frames, long long n_out, long long n)
{
    const long long vpg = N < 4096 ? 4096 / N : 1, frame = (long long)N * item;
    if (nstreams < 1 || n_out < 1) return 0;
    const long long total = nstreams * n_out;
    const long long j = vpg - 1 < total - 1 ? vpg - 1 : total - 1;        // vectors between a group's first and last
    long long cross = (n_out - 1 + j) / n_out;                          // stream ends between them, at most
    if (cross > nstreams - 1) cross = nstreams - 1;
    const long long inside = j < n_out - 1 ? j : n_out - 1;            // kept frames between them inside one stream, at most
    // first and last are at most cross n_frames + inside n frames apart; -1: far out of reach (and of 64 bits)
    if (n_frames > (1ll << 40) || n > (1ll << 40)) return -1;
    const long long span = cross * n_frames + inside * n;
    if (span > (1ll << 40)) return -1;
    return (span + 1) * frame;
}

inline bool logpwr_fused_ok(int N, int item, long long nstreams, long long n_frames, long long n_out, long long n)
{
    if (!logpwr_native_size(N) || nstreams < 1 || n_out < 0 || n < 1) return false;
    if (nstreams * n_out > LOGPWR_MAX_VECTORS) return false;
    if (N >= 4096) return true;
    const long long r = logpwr_group_range(N, item, nstreams, n_frames, n_out, n);
    return r >= 0 && r <= LOGPWR_MAX_RANGE;
}

}  // namespace grhip
