"""fll_band_edge_cc on one GPU, device resident, beside costas_loop_cc on the same data.

usage: python tools/bench_fll_band_edge.py [--captures 64] [--samples 1000000] [--generic-samples 250000] [--reps 3]
                                           [--only NAME] [--limit-s 120]

Data: `captures` streams of complex items: QPSK symbols held for sps = 2 samples, spun by 0.05 rad/sample from a start
phase of its own per stream, with noise of 0.05 per component.  fll_band_edge_cc(2, 0.35, filter_size, 2 pi / 100) with
all four outputs.

One JSON line per configuration (fs55_fast, fs55_generic, fs129_fast, fs129_generic): the median of --reps timed runs
(each between its own pair of events, after a ramp of untimed runs), all captures as streams of ONE work_device call;
"ns_per_sample_and_stream" is the time of the call over the items of one stream (the streams run side by side, one
wavefront each, so this is the serial step's time).  GENERIC runs on --generic-samples items per stream.
The yardstick, timed before and after every configuration in the same process on the same data (A-B-A):
costas_loop_cc(0.05, 2) in FAST, the serial walk of the same shape without the filters; "ratio_vs_costas" is the
configuration's time over the mean of the two yardstick times.  Nothing is aimed at: nobody has measured this shape.
Without --only every configuration runs in a child process of its own under a time limit of --limit-s seconds; one
that does not end in time, or fails, is reported and the rest is not started."""
import argparse
import json
import math
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--captures", type=int, default=64)
ap.add_argument("--samples", type=int, default=1_000_000)
ap.add_argument("--generic-samples", type=int, default=250_000)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--seed", type=int, default=1234)
ap.add_argument("--only", default=None)
ap.add_argument("--limit-s", type=float, default=120.0)
args = ap.parse_args()

NAMES = ["fs%d_%s" % (fs, m) for fs in (55, 129) for m in ("fast", "generic")]

if args.only is None:
    for name in NAMES:
        cmd = [sys.executable, os.path.abspath(__file__), "--only", name, "--captures", str(args.captures), "--samples",
               str(args.samples), "--generic-samples", str(args.generic_samples), "--reps", str(args.reps), "--seed", str(args.seed)]
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
    raise SystemExit("bench_fll_band_edge: --only takes one of " + " ".join(NAMES))

import torch  # noqa: E402
import grhip_loader  # noqa: E402

g = grhip_loader.import_grhip()
if g.device_count() < 1:
    raise SystemExit("bench_fll_band_edge: no HIP device visible; there is no CPU fallback")
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


fs_name, mode_name = args.only.split("_")
fs = int(fs_name[2:])
mode = g.MODE_GENERIC if mode_name == "generic" else g.MODE_FAST
n, N, SPS = args.captures, (args.generic_samples if mode_name == "generic" else args.samples), 2
gen = torch.Generator(device=dev)
gen.manual_seed(args.seed)
t = torch.arange(N, device=dev, dtype=torch.float64)
x = torch.randn((n, N, 2), device=dev, generator=gen) * 0.05
for s in range(n):
    k = torch.randint(0, 4, ((N + SPS - 1) // SPS,), device=dev, generator=gen).repeat_interleave(SPS)[:N].to(torch.float64)
    a = torch.remainder(0.05 * t + 0.1 * s, 2 * np.pi) + k * (np.pi / 2) + np.pi / 4
    x[s, :, 0] += torch.cos(a).to(torch.float32)
    x[s, :, 1] += torch.sin(a).to(torch.float32)
del t, a, k
y = torch.empty((n, N, 2), device=dev)
aux = [torch.empty((n, N), device=dev) for _ in range(3)]
torch.cuda.synchronize()

costas = g.costas_loop_cc(0.05, 2)
costas.set_streams(n)
costas.set_mode(g.MODE_FAST)


def yard():
    costas.work_device(N, x, y, stream=st)


blk = g.fll_band_edge_cc(SPS, 0.35, fs, 2 * math.pi / 100)
blk.set_streams(n)
blk.set_mode(mode)
a = timeit(yard, args.reps)
ms, ms_min = timeit(lambda: blk.work_device(N, x, y, aux[0], aux[1], aux[2], stream=st), args.reps)
b = timeit(yard, args.reps)
ym = 0.5 * (a[0] + b[0])
print(json.dumps({"block": "fll_band_edge_cc", "config": args.only, "mode": mode_name.upper(), "filter_size": fs, "sps": SPS,
                  "streams": n, "samples_per_stream": N, "ms_median": round(ms, 3), "ms_min": round(ms_min, 3),
                  "ns_per_sample_and_stream": round(ms * 1e6 / N, 2), "Msamples_per_s": round(n * N / ms / 1e3, 2),
                  "frequency_first_last_stream": [float(blk.get_frequency(s)) for s in (0, n - 1)],
                  "yardstick": "costas_loop_cc order 2 FAST", "yardstick_ms_before": round(a[0], 3), "yardstick_ms_after": round(b[0], 3),
                  "yardstick_ns_per_sample_and_stream": round(ym * 1e6 / N, 2), "ratio_vs_costas": round(ms / ym, 2)}), flush=True)
