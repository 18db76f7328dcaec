"""constellation_receiver_cb, constellation_demod_cb and constellation_decoder_cb on one GPU, device resident, beside a
comparison block on the same data.

usage: python tools/bench_constellation.py [--captures 64] [--samples 10000000] [--reps 3] [--only NAME] [--limit-s 300]

Data: `captures` streams of `samples` complex items: seeded symbols of the configuration's constellation rotated by
0.2 rad plus 1e-3 rad/sample, with noise of 0.02 per component.  Loop bandwidth 2 pi / 100, limits +-0.25.

One JSON line per configuration: the median of --reps timed runs (each between its own pair of events, after a ramp of
untimed runs), all captures as streams of ONE work_device call, Msamples/s over all streams.  The comparison block is
timed before and after every configuration in the same process on the same data (A-B-A); "ratio" is the configuration's
time over the mean of the two.
  receiver_qpsk_fast      the angle form; compared with costas_loop_cc(order 4) FAST.  Aim: ratio at most 1.
  demod_qpsk_engine1      the whole tail from the walk (differential, Gray); compared with the receiver alone.  Aim: at
                          most the receiver's time plus the spread of its two timings.
  receiver_8psk_fast, receiver_psk16_fast (angle form, a sector table), receiver_rect16_fast, receiver_calcdist4_fast
  (cartesian form), receiver_qpsk_generic, receiver_qpsk_fast_floats (all four outputs), demod_qpsk_engine0: reported
  beside them against costas_loop_cc FAST, without an aim.
  decoder_qpsk            one lane per output; "share_of_8TBps" is 9 bytes per sample over the time at 8 TB/s.
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

NAMES = ["receiver_qpsk_fast", "demod_qpsk_engine1", "demod_qpsk_engine0", "receiver_qpsk_fast_floats", "receiver_8psk_fast",
         "receiver_psk16_fast", "receiver_rect16_fast", "receiver_calcdist4_fast", "receiver_qpsk_generic", "decoder_qpsk"]

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
    raise SystemExit("bench_constellation: --only takes one of " + " ".join(NAMES))

import torch  # noqa: E402
import grhip_loader  # noqa: E402

g = grhip_loader.import_grhip()
if g.device_count() < 1:
    raise SystemExit("bench_constellation: no HIP device visible; there is no CPU fallback")
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


parts = args.only.split("_")
what, kind, variant = parts[0], parts[1], (parts[2] if len(parts) > 2 else "")
floats = parts[-1] == "floats"
cons = {"qpsk": g.constellation_qpsk, "8psk": g.constellation_8psk, "psk16": lambda: g.psk_constellation(16),
        "rect16": lambda: g.qam_constellation(16),
        "calcdist4": lambda: g.constellation_calcdist([1 + 1j, -1 + 1j, -1 - 1j, 1 - 1j], [0, 1, 3, 2], 4, 1)}[kind]()
pts = torch.from_numpy(np.ascontiguousarray(cons.points().view(np.float32).reshape(-1, 2))).to(dev).to(torch.float64)
n, N = args.captures, args.samples
gen = torch.Generator(device=dev)
gen.manual_seed(args.seed)
rot = -torch.remainder(0.2 + 1e-3 * torch.arange(N, device=dev, dtype=torch.float64), 2 * np.pi)
cr, sr = torch.cos(rot), torch.sin(rot)
del rot
x = torch.randn((n, N, 2), device=dev, generator=gen) * 0.02
for s in range(n):
    k = torch.randint(0, cons.arity(), (N,), device=dev, generator=gen)
    pr, pi = pts[k, 0], pts[k, 1]
    x[s, :, 0] += (pr * cr - pi * sr).to(torch.float32)
    x[s, :, 1] += (pr * sr + pi * cr).to(torch.float32)
del cr, sr, pr, pi, k
LOOP = (2 * np.pi / 100, -0.25, 0.25)
y = torch.empty((n, N, 2), device=dev)                  # the comparison block's output
out = torch.empty((n, N * 4), device=dev, dtype=torch.uint8)
f3 = [torch.empty((n, N), device=dev) for _ in range(3)] if floats else [None] * 3
torch.cuda.synchronize()

if what == "demod":
    yard_blk = g.constellation_receiver_cb(cons, *LOOP)
    yard_blk.set_streams(n)
    yard_name = "constellation_receiver_cb FAST"

    def yard():
        yard_blk.work_device(N, x, out, stream=st)
else:
    yard_blk = g.costas_loop_cc(0.05, 4)
    yard_blk.set_streams(n)
    yard_name = "costas_loop_cc(order 4) FAST"

    def yard():
        yard_blk.work_device(N, x, y, stream=st)

if what == "receiver":
    blk = g.constellation_receiver_cb(cons, *LOOP)
    blk.set_mode(g.MODE_GENERIC if variant == "generic" else g.MODE_FAST)
    run = lambda: blk.work_device(N, x, out, f3[0], f3[1], f3[2], stream=st)        # noqa: E731
elif what == "demod":
    blk = g.constellation_demod_cb(cons, *LOOP, True, True)
    blk.set_engine(int(variant[-1]))
    run = lambda: blk.work_device(N, x, out, stream=st)                               # noqa: E731
else:
    blk = g.constellation_decoder_cb(cons)
    run = lambda: blk.work_device(N, x, out, stream=st)                               # noqa: E731
blk.set_streams(n)
a = timeit(yard, args.reps)
ms, ms_min = timeit(run, args.reps)
b = timeit(yard, args.reps)
ym = 0.5 * (a[0] + b[0])
d = {"block": "constellation_%s_cb" % what, "config": args.only, "streams": n, "samples_per_stream": N, "ms_median": round(ms, 3),
     "ms_min": round(ms_min, 3), "Msamples_per_s": round(n * N / ms / 1e3, 1), "compared_with": yard_name,
     "compared_ms_before": round(a[0], 3), "compared_ms_after": round(b[0], 3), "ratio": round(ms / ym, 3)}
if what != "decoder":
    d["form"] = blk.form()
    d["frequency_first_last_stream"] = [float(blk.get_frequency(s)) for s in (0, n - 1)]
else:
    d["share_of_8TBps"] = round(9.0 * n * N / 8e12 / (ms * 1e-3), 4)
if args.only == "receiver_qpsk_fast":
    d["aim"] = "met" if ms <= ym else "missed"
if args.only == "demod_qpsk_engine1":
    d["aim"] = "met" if ms <= ym + abs(a[0] - b[0]) else "missed"
print(json.dumps(d), flush=True)
