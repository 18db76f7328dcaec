"""ctcss_squelch_ff on one GPU, device resident, beside two yardsticks already in the library.

usage: python tools/bench_ctcss_squelch.py [--captures 64] [--samples 10000000] [--reps 10] [--only NAME] [--no-yardstick]

Data: `captures` streams of `samples` floats, Gaussian noise of 0.01 with a 100 Hz tone of 0.1 at rate 8000 on every
other stretch of --burst samples (bursts cover half of each capture).  freq 100.0, level 0.01, len 800.

One JSON line per measurement: the median of --reps timed runs (each between its own pair of events, after a ramp of
untimed runs).
  ctcss_squelch_ff FAST, (ramp 0, gate off) and (ramp 64, gate on), all captures as streams of ONE work_device call:
    Gsamples/s and the fraction of 8 TB/s at 8 B per sample (read 4, write 4: the least a squelch without gating moves).
  Two yardsticks, each timed before and after every configuration (A-B-A):
    (a) goertzel_fc FAST, len 800, one pass over the same data: what ONE of the three tones costs on its own.  The
        detector stage of the squelch reads the same bytes once for three tones; its own time comes from a kernel trace
        (--only NAME --no-yardstick under a tracer), not from this script.
    (b) pwr_squelch_ff FAST at the same ramp and gate (alpha 0.01, -30 dB: between the noise and the tone);
        "ratio_vs_pwr_squelch" is the squelch's time over the mean of (b)'s two (at most 1: the aim is met).
  "noise_floor" is the larger A-to-A spread of the two yardsticks, |before - after| / mean, in the same run: a ratio
  closer to 1 than that says nothing."""
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
    raise SystemExit("bench_ctcss_squelch: no HIP device visible; there is no CPU fallback")
dev = torch.device("cuda", 0)
st = torch.cuda.Stream(device=dev)
RATE, FREQ, LEVEL, LEN = 8000, 100.0, 0.01, 800
ALPHA, DB = 0.01, -30.0


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
if N % LEN:
    raise SystemExit("bench_ctcss_squelch: --samples must be a multiple of %d (yardstick (a) takes whole blocks)" % LEN)
gen = torch.Generator(device=dev)
gen.manual_seed(args.seed)
x = torch.randn((n, N), device=dev, generator=gen) * 0.01
t = torch.arange(N, device=dev, dtype=torch.float64)
on = ((torch.arange(N, device=dev) // args.burst) % 2 == 1).to(torch.float32)
x += (0.1 * torch.sin((2 * np.pi * FREQ / RATE) * t).to(torch.float32) * on)[None, :]
del t, on
y = torch.empty((n, N), device=dev)
d_p = torch.zeros(n, dtype=torch.int32, device=dev)
torch.cuda.synchronize()

for name, ramp, gate in (("ramp0", 0, False), ("ramp64_gate", 64, True)):
    if args.only and args.only != name:
        continue
    blk = g.ctcss_squelch_ff(RATE, FREQ, LEVEL, LEN, ramp, gate)
    blk.set_streams(n)
    blk.set_mode(g.MODE_FAST)
    yards = []
    if not args.no_yardstick:
        gz = g.goertzel_fc(RATE, LEN, FREQ)
        gz.set_mode(g.MODE_FAST)
        z = torch.empty((n * (N // LEN), 2), device=dev)
        pw = g.pwr_squelch_ff(DB, ALPHA, ramp, gate)
        pw.set_streams(n)
        pw.set_mode(g.MODE_FAST)
        yards = [lambda: gz.work_device(n * (N // LEN), x, z, stream=st), lambda: pw.work_device(N, x, y, d_p, stream=st)]
    before = [timeit(f, args.reps) for f in yards]
    ms, ms_min = timeit(lambda: blk.work_device(N, x, y, d_p, stream=st), args.reps)
    share = float(d_p.sum().item()) / (n * N)
    after = [timeit(f, args.reps) for f in yards]
    gs = n * N / ms / 1e6
    d = {"block": "ctcss_squelch_ff", "config": name, "mode": "FAST", "streams": n, "samples_per_stream": N, "len": LEN,
         "ms_median": round(ms, 4), "ms_min": round(ms_min, 4), "Gsamples_per_s": round(gs, 2),
         "frac_of_8TBps_at_8B": round(gs * 8 / 8000.0, 4), "produced_share": round(share, 4)}
    if yards:
        gm, pm = (0.5 * (before[i][0] + after[i][0]) for i in (0, 1))
        floor = max(abs(before[i][0] - after[i][0]) / (0.5 * (before[i][0] + after[i][0])) for i in (0, 1))
        d.update(goertzel_fc_ms_before=round(before[0][0], 4), goertzel_fc_ms_after=round(after[0][0], 4),
                 pwr_squelch_ff_ms_before=round(before[1][0], 4), pwr_squelch_ff_ms_after=round(after[1][0], 4),
                 ratio_vs_goertzel_fc=round(ms / gm, 3), ratio_vs_pwr_squelch=round(ms / pm, 3), noise_floor=round(floor, 4),
                 aim_whole_call="met" if ms <= pm else ("within the noise floor" if ms <= pm * (1 + floor) else "missed"))
    print(json.dumps(d), flush=True)
