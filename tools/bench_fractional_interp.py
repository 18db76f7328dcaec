"""gr_fractional_interpolator_cc / _ff on one GPU, device resident: n fresh captures per run_captures_device call.

usage: python tools/bench_fractional_interp.py [--captures 64] [--samples 10000000] [--reps 20] [--check]
          [--ratios 0.5,1.08843537,2.0] [--phase 0] [--kinds cc,ff] [--modes FAST,GENERIC]

One JSON line per shape: the median of --reps timed calls (each between its own pair of events, after a ramp of
untimed calls), input Gsamples/s, outputs/s, and the algorithmic bytes ((8 + 8/ratio) B per input sample for cc,
(4 + 4/ratio) for ff: every input read once, every output written once) as a fraction of 8 TB/s.  "schedule" says
whether the kernel evaluated the closed form or read a walked schedule (the host's walk and its upload are inside
the timed call then).
--check compares the first outputs of capture 0 with the restatement in tests/fractional_interp_ref.py (GENERIC bit
for bit, FAST within 1e-5 of the output peak of the float64 evaluation)."""
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
import fractional_interp_ref as fr  # noqa: E402

g = grhip_loader.import_grhip()

ap = argparse.ArgumentParser()
ap.add_argument("--captures", type=int, default=64)
ap.add_argument("--samples", type=int, default=10_000_000)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--ratios", default="0.5,%r,2.0" % (160.0 / 147.0))
ap.add_argument("--phase", type=float, default=0.0)
ap.add_argument("--kinds", default="cc,ff")
ap.add_argument("--modes", default="FAST,GENERIC")
ap.add_argument("--seed", type=int, default=1234)
ap.add_argument("--check", action="store_true")
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
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def check(kind, mode, phase, ratio, x0, got0):
    M = 20000
    x = x0[:M].cpu().numpy()
    x = x.view(np.complex64).reshape(-1) if kind == "cc" else x.reshape(-1)
    ii, imu, _mu = fr.whole_stream_schedule(phase, ratio, M)
    got = got0[:len(ii)].cpu().numpy()
    got = got.view(np.complex64).reshape(-1) if kind == "cc" else got.reshape(-1)
    if mode == "GENERIC":
        ref = fr.eval_schedule(x, ii, imu)
        return bool(np.array_equal(got.view(np.uint32), ref.view(np.uint32)))
    ref = fr.eval_schedule(x, ii, imu, f64=True)
    return bool(np.abs(got - ref).max() / np.abs(ref).max() < 1e-5)


gen = torch.Generator(device=dev)
for kind in args.kinds.split(","):
    w = 2 if kind == "cc" else 1
    gen.manual_seed(args.seed)
    n, N = args.captures, args.samples
    x = torch.randn((n, N, w), device=dev, generator=gen)       # n captures, synthesised on the device
    for ratio in [float(np.float32(float(v))) for v in args.ratios.split(",")]:
        for mode in args.modes.split(","):
            blk = (g.fractional_interpolator_cc if kind == "cc" else g.fractional_interpolator_ff)(args.phase, ratio)
            blk.set_mode(getattr(g, "MODE_" + mode))
            n_out = blk.captures_nout(N)
            y = torch.empty((n, n_out, w), device=dev)
            torch.cuda.synchronize()
            fn = lambda: blk.run_captures_device(n, N, x, N, y, n_out, stream=st)  # noqa: E731
            ms, lo, hi = timeit(fn, args.reps)
            nin = n * N
            gbs = nin * 4 * w * (1.0 + 1.0 / ratio) / (ms * 1e-3) / 1e9
            line = {"block": "fractional_interpolator_" + kind, "mode": mode, "phase": args.phase, "ratio": ratio,
                    "schedule": "closed form" if fr.closed_form_ok(args.phase, ratio) else "walked",
                    "captures": n, "n_samples": N, "n_out": n_out, "reps": args.reps, "ms_median": round(ms, 4),
                    "ms_min": round(lo, 4), "ms_max": round(hi, 4),
                    "input_Gsamples_per_s": round(nin / ms / 1e6, 2),
                    "output_Gsamples_per_s": round(n * n_out / ms / 1e6, 2), "algorithmic_GBps": round(gbs, 1),
                    "frac_of_8TBps": round(gbs / 8000.0, 4)}
            if args.check:
                st.synchronize()
                line["check"] = check(kind, mode, np.float32(args.phase), np.float32(ratio), x[0], y[0])
            print(json.dumps(line), flush=True)
            del y
    del x
    torch.cuda.empty_cache()
