"""pfb_clock_sync_ccf on one GPU, device resident, beside fll_band_edge_cc on the same data.

usage: python tools/bench_pfb_clock_sync.py [--captures 64] [--samples 10000000] [--generic-samples 10000000] [--reps 3]
                                            [--only NAME] [--limit-s 240]

Data: `captures` streams of complex items at sps = 2: QPSK symbols through generic_demod's matched pulse
(root_raised_cosine(1, 2, 1, 0.35, 45)) at unit power, a start of its own per stream, noise of 0.02 per component.
pfb_clock_sync_ccf(2, 2 pi / 100, root_raised_cosine(32, 64, 1.0, 0.35, 704), 32, 16, 1.5, 1) with all four outputs.

One JSON line per configuration (fast, generic, one_stream): the median of --reps timed runs (each between its own pair
of events, after a ramp of untimed runs), all captures as streams of ONE work_device call; "ns_per_sample_and_stream" is the time of
the call over the INPUT items of one stream (the streams run side by side, one wavefront each, so this is the serial
walk's time per input sample).  GENERIC runs on --generic-samples items per stream.  The handle goes on from call to
call, as a stream does.
The yardstick, timed before and after every configuration in the same process on the same data (A-B-A):
fll_band_edge_cc(2, 0.35, 55, 2 pi / 100) in FAST with all four outputs; "ratio_vs_fll" is the configuration's time over
the mean of the two yardstick times.  The aim: per input sample no dearer than the yardstick.
one_stream: clock_recovery_mm_cc's device entry takes one stream per call, so the two timing loops are compared on ONE
stream of --samples items, which is like for like per sample since this walk is one wavefront per stream:
pfb_clock_sync_ccf FAST with all four outputs, and before and after it (A-B-A) clock_recovery_mm_cc(2, 0.25 * 0.175^2,
0.5, 0.175, 0.005) with its error output on the same stream, both timed by the host's clock around a call and a
synchronisation (general_work_device returns its counts, so it waits for the device itself); "ratio_vs_mm" is the time
per input sample over the mean of the two yardstick times.
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
ap.add_argument("--samples", type=int, default=10_000_000)
ap.add_argument("--generic-samples", type=int, default=10_000_000)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--seed", type=int, default=1234)
ap.add_argument("--only", default=None)
ap.add_argument("--limit-s", type=float, default=240.0)
args = ap.parse_args()

NAMES = ["fast", "generic", "one_stream"]

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
    raise SystemExit("bench_pfb_clock_sync: --only takes one of " + " ".join(NAMES))

import torch  # noqa: E402
import grhip_loader  # noqa: E402

g = grhip_loader.import_grhip()
if g.device_count() < 1:
    raise SystemExit("bench_pfb_clock_sync: no HIP device visible; there is no CPU fallback")
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
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


mode_name = args.only
mode = g.MODE_GENERIC if mode_name == "generic" else g.MODE_FAST
n, N, SPS, NF = args.captures, (args.generic_samples if mode_name == "generic" else args.samples), 2, 32
if mode_name == "one_stream":
    n = 1
gen = torch.Generator(device=dev)
gen.manual_seed(args.seed)
pulse = torch.from_numpy(g.firdes_root_raised_cosine(1.0, float(SPS), 1.0, 0.35, 45).astype(np.float32)).to(dev)
x = torch.randn((n, N, 2), device=dev, generator=gen) * 0.02
nsym = N // SPS + len(pulse)
for s in range(n):
    for c in range(2):
        up = torch.zeros(nsym * SPS, device=dev)
        up[::SPS] = (torch.randint(0, 2, (nsym,), device=dev, generator=gen).to(torch.float32) * 2 - 1) * (1 / math.sqrt(2))
        shaped = torch.nn.functional.conv1d(up.view(1, 1, -1), pulse.view(1, 1, -1), padding=len(pulse) - 1).view(-1)
        x[s, :, c] += shaped[len(pulse) + s % 7:][:N]
    x[s] /= torch.sqrt((x[s] ** 2).sum(dim=1).mean())
del up, shaped
taps = g.firdes_root_raised_cosine(float(NF), float(NF * SPS), 1.0, 0.35, 11 * SPS * NF)
blk = g.pfb_clock_sync_ccf(SPS, 2 * math.pi / 100, taps, NF, 16.0, 1.5, 1)
blk.set_streams(n)
blk.set_mode(mode)
cap = blk.max_produced(N)
y = torch.empty((n, cap, 2), device=dev)
aux = [torch.empty((n, cap), device=dev) for _ in range(3)]
prod = torch.zeros(n, dtype=torch.int32, device=dev)
yf = torch.empty((n, N, 2), device=dev)
auxf = [torch.empty((n, N), device=dev) for _ in range(3)]
torch.cuda.synchronize()


def wall(fn, reps, ramp_s=0.3):
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < ramp_s:
        fn()
        torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


if mode_name == "one_stream":
    mm_out = N // SPS - 64
    made = []
    mm = g.clock_recovery_mm_cc(float(SPS), 0.25 * 0.175 * 0.175, 0.5, 0.175, 0.005)           # goes on from call to call too

    def mm_run():
        made.append(mm.general_work_device(mm_out, N, x, yf, auxf[0], stream=st))

    a = wall(mm_run, args.reps)
    ms, ms_min, ms_max = wall(lambda: blk.work_device(N, x, cap, y, prod, aux[0], aux[1], aux[2], stream=st), args.reps)
    b = wall(mm_run, args.reps)
    ym = 0.5 * (a[0] + b[0])
    print(json.dumps({"block": "pfb_clock_sync_ccf", "config": args.only, "mode": "FAST", "nfilters": NF, "ntaps": int(len(taps)), "sps": SPS,
                      "streams": 1, "samples_per_stream": N, "ms_median": round(ms, 3), "ms_min": round(ms_min, 3), "ms_max": round(ms_max, 3),
                      "ns_per_sample": round(ms * 1e6 / N, 2), "produced": int(prod.cpu()[0]), "slips": int(blk.slips(0)),
                      "yardstick": "clock_recovery_mm_cc, one stream, with its error output", "yardstick_produced_consumed": list(made[-1]),
                      "yardstick_ms_before": round(a[0], 3), "yardstick_ms_after": round(b[0], 3),
                      "yardstick_ns_per_sample": round(ym * 1e6 / made[-1][1], 2),
                      "ratio_vs_mm": round((ms / N) / (ym / made[-1][1]), 3)}), flush=True)
    raise SystemExit(0)

fll = g.fll_band_edge_cc(SPS, 0.35, 55, 2 * math.pi / 100)
fll.set_streams(n)
fll.set_mode(g.MODE_FAST)


def yard():
    fll.work_device(N, x, yf, auxf[0], auxf[1], auxf[2], stream=st)


a = timeit(yard, args.reps)
ms, ms_min, ms_max = timeit(lambda: blk.work_device(N, x, cap, y, prod, aux[0], aux[1], aux[2], stream=st), args.reps)
b = timeit(yard, args.reps)
ym = 0.5 * (a[0] + b[0])
p = prod.cpu().numpy()
print(json.dumps({"block": "pfb_clock_sync_ccf", "config": args.only, "mode": mode_name.upper(), "nfilters": NF, "ntaps": int(len(taps)),
                  "sps": SPS, "streams": n, "samples_per_stream": N, "ms_median": round(ms, 3), "ms_min": round(ms_min, 3),
                  "ms_max": round(ms_max, 3), "ns_per_sample_and_stream": round(ms * 1e6 / N, 2),
                  "Msamples_per_s": round(n * N / ms / 1e3, 2), "produced_first_last_stream": [int(p[0]), int(p[-1])],
                  "slips": int(sum(blk.slips(s) for s in range(n))), "rate_first_last_stream": [float(blk.get_clock_rate(s)) for s in (0, n - 1)],
                  "yardstick": "fll_band_edge_cc 55 taps FAST", "yardstick_ms_before": round(a[0], 3), "yardstick_ms_after": round(b[0], 3),
                  "yardstick_ns_per_sample_and_stream": round(ym * 1e6 / N, 2), "ratio_vs_fll": round(ms / ym, 3),
                  "aim_no_dearer_than_fll": "met" if ms <= ym else "missed"}), flush=True)
