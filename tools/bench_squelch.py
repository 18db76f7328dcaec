"""pwr_squelch_cc on one GPU, device resident, beside its detector's nearest relatives.

usage: python tools/bench_squelch.py [--captures 64] [--samples 10000000] [--reps 10] [--only NAME] [--no-yardstick]

Data: `captures` streams of `samples` complex items, Gaussian noise of 0.01 per component with a unit tone at 0.05
cycles per sample on every other stretch of --burst samples (bursts cover half of each capture).  alpha 0.01, -20 dB.

One JSON line per measurement: the median of --reps timed runs (each between its own pair of events, after a ramp of
untimed runs).
  pwr_squelch_cc FAST, ramp 0 and 64, gate off and on, all captures as streams of ONE work_device call: Gsamples/s and
    the fraction of 8 TB/s at 16 B per sample (the least a squelch without gating moves: read 8, write 8).
  The yardstick, timed before and after every configuration (A-B-A): complex_to_mag_squared followed by
    single_pole_iir_filter_ff FAST on the same data, each one call over all captures; "ratio_vs_yardstick" is squelch
    time over the mean of the two yardstick times (at most 1: the aim is met).
--only NAME runs one configuration (ramp0, ramp0_gate, ramp64, ramp64_gate) and --no-yardstick drops the yardstick: for
a kernel trace of the squelch alone (the walk kernel's share of the total comes from there)."""
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
    raise SystemExit("bench_squelch: no HIP device visible; there is no CPU fallback")
dev = torch.device("cuda", 0)
st = torch.cuda.Stream(device=dev)
ALPHA, DB = 0.01, -20.0


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
x = torch.randn((n, N, 2), device=dev, generator=gen) * 0.01
t = torch.arange(N, device=dev, dtype=torch.float64)
on = ((torch.arange(N, device=dev) // args.burst) % 2 == 1).to(torch.float32)
ph = (2 * np.pi * 0.05) * t
x[:, :, 0] += (torch.cos(ph).to(torch.float32) * on)[None, :]
x[:, :, 1] += (torch.sin(ph).to(torch.float32) * on)[None, :]
del t, ph
y = torch.empty((n, N, 2), device=dev)
d_p = torch.zeros(n, dtype=torch.int32, device=dev)
torch.cuda.synchronize()

yard = None
if not args.no_yardstick:
    p = torch.empty((n, N), device=dev)
    q = torch.empty((n, N), device=dev)
    m2 = g.complex_to_mag_squared()
    m2.set_streams(n)
    iir = g.single_pole_iir_filter_ff(ALPHA)
    iir.set_streams(n)
    iir.set_mode(g.MODE_FAST)

    def yard():
        m2.work_device(N, x, p, stream=st)
        iir.work_device(N, p, q, stream=st)

for name, ramp, gate in (("ramp0", 0, False), ("ramp0_gate", 0, True), ("ramp64", 64, False), ("ramp64_gate", 64, True)):
    if args.only and args.only != name:
        continue
    blk = g.pwr_squelch_cc(DB, ALPHA, ramp, gate)
    blk.set_streams(n)
    blk.set_mode(g.MODE_FAST)
    a = timeit(yard, args.reps) if yard else None
    ms, ms_min = timeit(lambda: blk.work_device(N, x, y, d_p, stream=st), args.reps)
    b = timeit(yard, args.reps) if yard else None
    gs = n * N / ms / 1e6
    d = {"block": "pwr_squelch_cc", "config": name, "mode": "FAST", "streams": n, "samples_per_stream": N, "ms_median": round(ms, 4),
         "ms_min": round(ms_min, 4), "Gsamples_per_s": round(gs, 2), "frac_of_8TBps_at_16B": round(gs * 16 / 8000.0, 4),
         "produced_share": round(float(d_p.sum().item()) / (n * N), 4)}
    if yard:
        ym = 0.5 * (a[0] + b[0])
        d.update(yardstick="complex_to_mag_squared -> single_pole_iir_filter_ff FAST", yardstick_ms_before=round(a[0], 4),
                 yardstick_ms_after=round(b[0], 4), yardstick_Gsamples_per_s=round(n * N / ym / 1e6, 2),
                 ratio_vs_yardstick=round(ms / ym, 3), aim="met" if ms <= ym else "missed")
    print(json.dumps(d), flush=True)
