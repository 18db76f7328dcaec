"""agc_cc and agc2_cc on one GPU, device resident, beside pwr_squelch_cc on the same data.

usage: python tools/bench_agc.py [--captures 64] [--samples 10000000] [--reps 10] [--only NAME] [--no-yardstick]

Data: `captures` streams of `samples` complex items, Gaussian noise of 0.7 per component on every other stretch of
--burst samples and 0.035 between them, so the loop keeps moving.  agc_cc(1e-3, 1, 1, 1000): rate |x| stays far below 1,
no chunk is flagged.  agc2_cc(1e-2, 1e-3, 1, 1, 1000).

One JSON line per measurement: the median of --reps timed runs (each between its own pair of events, after a ramp of
untimed runs), all captures as streams of ONE work_device call, Gsamples/s and the fraction of 8 TB/s at 16 B per sample
(read 8, write 8: the least the block moves).
  agc_fast     agc_cc in MODE_FAST: the chunked form, three kernels
  agc_generic  agc_cc in MODE_GENERIC: the serial walk, one wavefront per stream
  agc2         agc2_cc: the serial walk in every mode
The yardstick, timed before and after every configuration (A-B-A): pwr_squelch_cc FAST, ramp 0, no gate, -20 dB,
alpha 0.01, one call over the same data; "ratio_vs_yardstick" is the configuration's time over the mean of the two
yardstick times.  The aim (at most 1) is agc_fast's; the two serial walks are reported only.
--only NAME runs one configuration and --no-yardstick drops the yardstick: for a kernel trace of one configuration alone
(the three kernels' shares of an agc_fast call come from there)."""
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

ap = argparse.ArgumentParser()
ap.add_argument("--captures", type=int, default=64)
ap.add_argument("--samples", type=int, default=10_000_000)
ap.add_argument("--burst", type=int, default=100_000)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--seed", type=int, default=1234)
ap.add_argument("--only", default=None)
ap.add_argument("--no-yardstick", action="store_true")
args = ap.parse_args()

if g.device_count() < 1:
    raise SystemExit("bench_agc: no HIP device visible; there is no CPU fallback")
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
    return float(np.median(ms)), float(np.min(ms))


n, N = args.captures, args.samples
gen = torch.Generator(device=dev)
gen.manual_seed(args.seed)
x = torch.randn((n, N, 2), device=dev, generator=gen)
level = torch.where((torch.arange(N, device=dev) // args.burst) % 2 == 1, 0.7, 0.035).to(torch.float32)
x *= level[None, :, None]
del level
y = torch.empty((n, N, 2), device=dev)
d_p = torch.zeros(n, dtype=torch.int32, device=dev)
torch.cuda.synchronize()

yard = None
if not args.no_yardstick:
    sq = g.pwr_squelch_cc(-20.0, 0.01, 0, False)
    sq.set_streams(n)
    sq.set_mode(g.MODE_FAST)

    def yard():
        sq.work_device(N, x, y, d_p, stream=st)

CONFIGS = (("agc_fast", lambda: g.agc_cc(1e-3, 1, 1, 1000), g.MODE_FAST),
           ("agc_generic", lambda: g.agc_cc(1e-3, 1, 1, 1000), g.MODE_GENERIC),
           ("agc2", lambda: g.agc2_cc(1e-2, 1e-3, 1, 1, 1000), g.MODE_FAST))
for name, make, mode in CONFIGS:
    if args.only and args.only != name:
        continue
    blk = make()
    blk.set_streams(n)
    blk.set_mode(mode)
    a = timeit(yard, args.reps) if yard else None
    ms, ms_min = timeit(lambda: blk.work_device(N, x, y, stream=st), args.reps)
    b = timeit(yard, args.reps) if yard else None
    gains = [float(blk.gain(s)) for s in (0, n - 1)]
    gs = n * N / ms / 1e6
    d = {"block": "agc2_cc" if name == "agc2" else "agc_cc", "config": name, "mode": "GENERIC" if mode == g.MODE_GENERIC else "FAST",
         "streams": n, "samples_per_stream": N, "ms_median": round(ms, 4), "ms_min": round(ms_min, 4),
         "Gsamples_per_s": round(gs, 2), "frac_of_8TBps_at_16B": round(gs * 16 / 8000.0, 4), "gain_first_last_stream": gains}
    if yard:
        ym = 0.5 * (a[0] + b[0])
        d.update(yardstick="pwr_squelch_cc FAST ramp 0 no gate", yardstick_ms_before=round(a[0], 4),
                 yardstick_ms_after=round(b[0], 4), ratio_vs_yardstick=round(ms / ym, 3))
        if name == "agc_fast":
            d.update(aim="met" if ms <= ym else "missed")
    print(json.dumps(d), flush=True)
