"""costas_loop_cc and the three pll_* blocks on one GPU, device resident, beside agc2_cc on the same data.

usage: python tools/bench_carrier.py [--captures 64] [--samples 10000000] [--reps 3] [--only NAME] [--limit-s 300]

Data: `captures` streams of `samples` complex items.  For the PLLs a unit tone at 0.3 rad/sample from a start phase of
its own per stream, with noise of 0.05 per component; for Costas symbols of the order's constellation (order 8 at
amplitude 2) rotated by 0.2 rad plus 1e-3 rad/sample, with noise of 0.02.  pll_*(0.05, 1, -1), costas_loop_cc(0.05,
order).

One JSON line per configuration: the median of --reps timed runs (each between its own pair of events, after a ramp of
untimed runs), all captures as streams of ONE work_device call, Msamples/s over all streams.
  pll_freqdet_cf, pll_refout_cc, pll_carriertracking_cc   one engine in every mode: timed in GENERIC and in FAST
  costas2 / costas4 / costas8                             GENERIC (the float-rounded double NCO) and FAST (the float one)
The yardstick, timed before and after every configuration in the same process on the same data (A-B-A): agc2_cc(1e-2,
1e-3, 1, 1, 1000), the serial walk of the same shape; "ratio_vs_agc2" is the configuration's time over the mean of the
two yardstick times.  Aims (at most 1): pll_freqdet_cf, and costas_loop_cc FAST; everything else is reported only.
Without --only every configuration runs in a child process of its own under a time limit of --limit-s seconds; one
that does not end in time, or fails, is reported and the rest is not started."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--captures", type=int, default=64)
ap.add_argument("--samples", type=int, default=10_000_000)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--seed", type=int, default=1234)
ap.add_argument("--only", default=None)
ap.add_argument("--limit-s", type=float, default=300.0)
args = ap.parse_args()

NAMES = [b + "_" + m for b in ("pll_freqdet_cf", "pll_refout_cc", "pll_carriertracking_cc", "costas2", "costas4", "costas8")
         for m in ("generic", "fast")]

if args.only is None:
    for name in NAMES:
        cmd = [sys.executable, os.path.abspath(__file__), "--only", name, "--captures", str(args.captures), "--samples",
               str(args.samples), "--reps", str(args.reps), "--seed", str(args.seed)]
        try:
            r = subprocess.run(cmd, timeout=args.limit_s)
        except subprocess.TimeoutExpired:
            print(json.dumps({"config": name, "error": "not finished after %g s" % args.limit_s}), flush=True)
            raise SystemExit(1)
        if r.returncode != 0:
            print(json.dumps({"config": name, "error": "exit status %d" % r.returncode}), flush=True)
            raise SystemExit(1)
    raise SystemExit(0)

if args.only not in NAMES:
    raise SystemExit("bench_carrier: --only takes one of " + " ".join(NAMES))

import torch  # noqa: E402
import grhip_loader  # noqa: E402

g = grhip_loader.import_grhip()
if g.device_count() < 1:
    raise SystemExit("bench_carrier: no HIP device visible; there is no CPU fallback")
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


block, mode_name = args.only.rsplit("_", 1)
mode = g.MODE_GENERIC if mode_name == "generic" else g.MODE_FAST
n, N = args.captures, args.samples
gen = torch.Generator(device=dev)
gen.manual_seed(args.seed)
t = torch.arange(N, device=dev, dtype=torch.float64)
if block.startswith("costas"):
    order = int(block[6:])
    ph = torch.remainder(0.2 + 1e-3 * t, 2 * np.pi)
    noise, amp = 0.02, (2.0 if order == 8 else (2.0 ** 0.5 if order == 4 else 1.0))
else:
    order = 0
    ph = torch.remainder(0.3 * t, 2 * np.pi)
    noise, amp = 0.05, 1.0
del t
x = torch.randn((n, N, 2), device=dev, generator=gen) * noise
for s in range(n):
    if order:
        k = torch.randint(0, order, (N,), device=dev, generator=gen).to(torch.float64)
        a = ph + k * (2 * np.pi / order) + (np.pi / order if order > 2 else 0.0)
    else:
        a = ph + 0.1 * s
    x[s, :, 0] += (amp * torch.cos(a)).to(torch.float32)
    x[s, :, 1] += (amp * torch.sin(a)).to(torch.float32)
del ph, a
y = torch.empty((n, N, 2), device=dev)
torch.cuda.synchronize()

agc = g.agc2_cc(1e-2, 1e-3, 1, 1, 1000)
agc.set_streams(n)


def yard():
    agc.work_device(N, x, y, stream=st)


blk = g.costas_loop_cc(0.05, order) if order else getattr(g, block)(0.05, 1.0, -1.0)
blk.set_streams(n)
blk.set_mode(mode)
a = timeit(yard, args.reps)
ms, ms_min = timeit(lambda: blk.work_device(N, x, y, stream=st), args.reps)
b = timeit(yard, args.reps)
ym = 0.5 * (a[0] + b[0])
d = {"block": "costas_loop_cc" if order else block, "config": args.only, "mode": mode_name.upper(), "streams": n,
     "samples_per_stream": N, "ms_median": round(ms, 3), "ms_min": round(ms_min, 3),
     "Msamples_per_s": round(n * N / ms / 1e3, 1), "frequency_first_last_stream": [float(blk.get_frequency(s)) for s in (0, n - 1)],
     "yardstick": "agc2_cc", "yardstick_ms_before": round(a[0], 3), "yardstick_ms_after": round(b[0], 3),
     "ratio_vs_agc2": round(ms / ym, 3)}
if order:
    d["order"] = order
if block == "pll_freqdet_cf" or (order and mode_name == "fast"):
    d["aim"] = "met" if ms <= ym else "missed"
print(json.dumps(d), flush=True)
