"""blks2.logpwrfft_c / logpwrfft_f on one GPU, device resident, beside the two things it is measured against, timed in the
same process before and after it (A, B, A: the two comparison figures give the run-to-run spread).

usage: python tools/bench_logpwrfft.py [--captures 64] [--samples 10000000] [--sizes 4096,1024] [--rate 30] [--reps 5]

`captures` successive work_device calls of `samples` samples each (rounded down to whole frames, and to a multiple of
the decimation so that every call keeps the same number of frames), one stream, FAST mode, state and countdown carried
from call to call.  Per size: decimation 1 and the one that gives `rate` frames per second at a sample rate of
`samples` per second (81 at 4096 points), averaging on and off, complex and float input.
  five blocks      keep_one_in_n -> fft_vcc | fft_vfc (windowed) -> complex_to_mag_squared -> single_pole_iir_filter_ff ->
                   nlog10_ff, the reference's order, every intermediate of every capture in a buffer of its own (nothing
                   is re-used out of the cache): 60 B of HBM traffic per kept complex sample (16 keep copy, 16 transform,
                   12, 8, 8), 48 for float input
  transform        the windowed forward fft_vcc | fft_vfc on the kept frames alone (contiguous): 16 (12) B per sample
  logpwrfft        8 B in + 4 B out per kept complex sample with averaging off (12), + 8 for the averaging pass (20);
                   4 + 4 (8) and 16 for float input
One JSON line per measurement: `kept_vectors_per_s`, `frac_of_hbm` = algorithmic bytes / time over 8 TB/s,
`vs_five_blocks` and `vs_transform` = the comparison's mean time over the block's (`vs_transform`, averaging off: the aim
is 1.0 or more; the margin is the A-to-B spread printed beside it).  Time: device events around `reps` passes on one
stream after a short ramp; kernel time alone comes from a separate rocprofv3 --kernel-trace --stats run."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import grhip_loader  # noqa: E402

g = grhip_loader.import_grhip()
HBM_BPS = 8.0e12

ap = argparse.ArgumentParser()
ap.add_argument("--captures", type=int, default=64)
ap.add_argument("--samples", type=int, default=10_000_000, help="samples per capture (and per second, for --rate)")
ap.add_argument("--sizes", default="4096,1024")
ap.add_argument("--rate", type=float, default=30.0, help="frames per second of the decimated case")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--seed", type=int, default=1234)
args = ap.parse_args()

dev = torch.device("cuda", 0)
st = torch.cuda.Stream(device=dev)
gen = torch.Generator(device=dev)
gen.manual_seed(args.seed)


def timeit(fn, reps, ramp_s=0.3):
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < ramp_s:
        fn()
        st.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(reps):
        fn()
    e1.record(st)
    st.synchronize()
    return e0.elapsed_time(e1) / reps


def line(block, N, kind, decim, average, ms, kept, bytes_per_sample, **extra):
    d = {"block": block, "fft_size": N, "input": kind, "decim": decim, "average": average, "captures": args.captures,
         "kept_vectors": kept, "ms": round(ms, 4), "kept_vectors_per_s": round(kept / (ms * 1e-3), 1),
         "kept_Gsamples_per_s": round(kept * N / ms / 1e6, 3), "bytes_per_kept_sample": bytes_per_sample,
         "GBps": round(bytes_per_sample * kept * N / ms / 1e6, 1),
         "frac_of_hbm": round(bytes_per_sample * kept * N / (ms * 1e-3) / HBM_BPS, 4)}
    d.update(extra)
    print(json.dumps(d), flush=True)


for N in (int(v) for v in args.sizes.split(",")):
    win = g.window_blackmanharris(N)
    w32 = win.astype(np.float32)
    d_rate = max(1, int(np.floor(args.samples / N / args.rate + 0.5)))
    for kind in ("c", "f"):
        item = 2 if kind == "c" else 1
        for decim in (1, d_rate):
            F = (args.samples // N // decim) * decim         # frames per capture
            K = F // decim                                   # kept per capture
            kept = K * args.captures
            x = torch.randn((args.captures * F * N * item,), device=dev, generator=gen)
            out = torch.empty((kept * N,), device=dev)
            t_keep = torch.empty((kept * N * item,), device=dev)
            t_spec = torch.empty((kept * N * 2,), device=dev)
            t_pow = torch.empty((kept * N,), device=dev)
            t_avg = torch.empty((kept * N,), device=dev)
            out2 = torch.empty((kept * N,), device=dev)
            mk_fft = (lambda: g.fft_vcc(N, True, w32)) if kind == "c" else (lambda: g.fft_vfc(N, True, w32))
            fft_alone = mk_fft()
            for average in (True, False):
                alpha = 0.2
                cls = g.logpwrfft_c if kind == "c" else g.logpwrfft_f
                blk = cls(float(args.samples), N, 2.0, args.samples / N / decim, alpha, average)
                assert blk.decimation() == decim, (blk.decimation(), decim)
                blk.set_mode(g.MODE_FAST)
                keep, fft = g.keep_one_in_n(N * 4 * item, decim), mk_fft()
                mag, iir = g.complex_to_mag_squared(N), g.single_pole_iir_filter_ff(alpha if average else 1.0, N)
                log = g.nlog10_ff(10, N, 0.0)
                for b in (mag, iir, log):
                    b.set_mode(g.MODE_FAST)
                torch.cuda.synchronize()

                def run_blk():
                    for c in range(args.captures):
                        blk.work_device(F, x[c * F * N * item:], out[c * K * N:], st)

                def run_five():
                    for c in range(args.captures):
                        o, oc = c * K * N, c * K * N * 2
                        keep.work_device(F, x[c * F * N * item:], t_keep[o * item:], st)
                        fft.work_device(K, t_keep[o * item:], t_spec[oc:], st)
                        mag.work_device(K, t_spec[oc:], t_pow[o:], st)
                        iir.work_device(K, t_pow[o:], t_avg[o:], st)
                        log.work_device(K, t_avg[o:], out2[o:], st)

                def run_fft():                               # the kept frames alone, contiguous
                    for c in range(args.captures):
                        fft_alone.work_device(K, x[c * K * N * item:], t_spec[c * K * N * 2:], st)

                b_in = 4.0 * item
                five_a, fft_a = timeit(run_five, args.reps), timeit(run_fft, args.reps)
                ms = timeit(run_blk, args.reps)
                five_b, fft_b = timeit(run_five, args.reps), timeit(run_fft, args.reps)
                for tag, t in (("A", five_a), ("B", five_b)):
                    line("five blocks " + tag, N, kind, decim, average, t, kept, 2 * b_in + (b_in + 8) + 12 + 8 + 8)
                for tag, t in (("A", fft_a), ("B", fft_b)):
                    line("transform alone (windowed fft_v%sc) %s" % (kind, tag), N, kind, decim, average, t, kept, b_in + 8)
                line("logpwrfft_" + kind, N, kind, decim, average, ms, kept, b_in + 4 + (8 if average else 0),
                     vs_five_blocks=round(0.5 * (five_a + five_b) / ms, 3), five_blocks_spread=round(abs(five_a - five_b) / min(five_a, five_b), 3),
                     vs_transform=round(0.5 * (fft_a + fft_b) / ms, 3), transform_spread=round(abs(fft_a - fft_b) / min(fft_a, fft_b), 3))
                del blk, keep, fft, mag, iir, log
            del x, out, t_keep, t_spec, t_pow, t_avg, out2, fft_alone
            torch.cuda.empty_cache()
