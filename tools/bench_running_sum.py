"""dc_blocker_ff / _cc, moving_average_ff and integrate_ff on one GPU, device resident.

usage: python tools/bench_running_sum.py [--captures 64] [--samples 10000000] [--reps 20] [--generic-samples 1000000]

One JSON line per measurement: the median of --reps timed runs (each between its own pair of events, after a ramp of
untimed runs).
  dc_blocker_ff / _cc FAST, D = 32 long form, all captures as streams of ONE work_device call, Gsamples/s and the
    fraction of 8 TB/s at 8 / 16 B per sample, beside fir_filter_fff / _ccf FAST with the equivalent 125 taps (delta at
    62 minus the 32-box convolved four times) on the same data in the same run, timed before and after;
    "speedup_vs_fir_filter" is the ratio.
  moving_average_ff(10, 0.1) FAST beside fir_filter_fff with ten 0.1 taps, the same way.
  dc_blocker GENERIC: `captures` streams of --generic-samples each in one call (one wavefront per stream).
  moving_average_ff GENERIC (max_iter 4096) and integrate_ff(10), both modes."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import grhip_loader  # noqa: E402

g = grhip_loader.import_grhip()

ap = argparse.ArgumentParser()
ap.add_argument("--captures", type=int, default=64)
ap.add_argument("--samples", type=int, default=10_000_000)
ap.add_argument("--generic-samples", type=int, default=1_000_000)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--seed", type=int, default=1234)
args = ap.parse_args()

dev = torch.device("cuda", 0)
st = torch.cuda.Stream(device=dev)


def timeit(fn, reps, ramp_s=0.3):
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < ramp_s:
        fn()
        st.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        fn()
        e1.record(st)
        st.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


def line(block, mode, ms, nsamp, bytes_per_sample, **kw):
    gs = nsamp / ms / 1e6
    d = {"block": block, "mode": mode, "ms_median": round(ms, 4), "Gsamples_per_s": round(gs, 2),
         "frac_of_8TBps": round(gs * bytes_per_sample / 8000.0, 4)}
    d.update(kw)
    print(json.dumps(d), flush=True)


def dc_taps(D):
    box = np.ones(D) / D
    h = np.convolve(np.convolve(box, box), np.convolve(box, box))
    t = -h
    t[2 * D - 2] += 1.0
    return t.astype(np.float32)


n, N = args.captures, args.samples
gen = torch.Generator(device=dev)
gen.manual_seed(args.seed)

for kind, width, bps in (("ff", 1, 8.0), ("cc", 2, 16.0)):
    x = torch.rand((n, N, width), device=dev, generator=gen) * 2 - 1 + 10
    y = torch.empty((n, N, width), device=dev)
    taps = dc_taps(32)
    fir = (g.fir_filter_fff if kind == "ff" else g.fir_filter_ccf)(1, taps)
    fir.set_mode(g.MODE_FAST)
    nf = N - len(taps) + 1

    def fn_fir():
        for c in range(n):
            fir.work_device(nf, x[c], y[c], stream=st)
    a = timeit(fn_fir, args.reps)
    blk = (g.dc_blocker_ff if kind == "ff" else g.dc_blocker_cc)(32, True)
    blk.set_streams(n)
    blk.set_mode(g.MODE_FAST)
    ms = timeit(lambda: blk.work_device(N, x, y, stream=st), args.reps)
    b = timeit(fn_fir, args.reps)
    fir_ms = 0.5 * (a + b) * (N / nf)
    line("fir_filter_%s 125 taps (delta - box^4)" % ("fff" if kind == "ff" else "ccf"), "FAST", fir_ms, n * N, bps,
         ms_before=round(a, 4), ms_after=round(b, 4))
    line("dc_blocker_%s D=32 long" % kind, "FAST", ms, n * N, bps, streams=n, speedup_vs_fir_filter=round(fir_ms / ms, 3))
    Ng = min(args.generic_samples, N)
    blk.set_mode(g.MODE_GENERIC)
    xg, yg = x[:, :Ng].contiguous(), torch.empty((n, Ng, width), device=dev)
    line("dc_blocker_%s D=32 long" % kind, "GENERIC", timeit(lambda: blk.work_device(Ng, xg, yg, stream=st), max(3, args.reps // 4)),
         n * Ng, bps, streams=n, samples_per_stream=Ng)
    del xg, yg
    if kind == "ff":
        fir = g.fir_filter_fff(1, np.full(10, 0.1, np.float32))
        fir.set_mode(g.MODE_FAST)
        nm = N - 9

        def fn_fir10():
            for c in range(n):
                fir.work_device(nm, x[c], y[c], stream=st)
        a = timeit(fn_fir10, args.reps)
        res = {}
        for mode in ("FAST", "GENERIC"):
            ma = g.moving_average_ff(10, 0.1)
            ma.set_mode(getattr(g, "MODE_" + mode))

            def fn_ma():
                for c in range(n):
                    ma.work_device(nm, x[c], y[c], stream=st)
            res[mode] = timeit(fn_ma, args.reps if mode == "FAST" else max(3, args.reps // 4))
        b = timeit(fn_fir10, args.reps)
        fir_ms = 0.5 * (a + b)
        line("fir_filter_fff ten 0.1 taps", "FAST", fir_ms, n * nm, 8.0, ms_before=round(a, 4), ms_after=round(b, 4))
        for mode in ("FAST", "GENERIC"):
            line("moving_average_ff(10, 0.1)", mode, res[mode], n * nm, 8.0, speedup_vs_fir_filter=round(fir_ms / res[mode], 3))
        for mode in ("FAST", "GENERIC"):
            it = g.integrate_ff(10)
            it.set_mode(getattr(g, "MODE_" + mode))

            def fn_it():
                for c in range(n):
                    it.work_device(N // 10, x[c], y[c], stream=st)
            line("integrate_ff(10)", mode, timeit(fn_it, args.reps), n * (N // 10) * 10, 4.4)
    del x, y
    torch.cuda.empty_cache()
