"""gr_interp_fir_filter_XXX / gr_rational_resampler_base_XXX on one GPU, device resident: n fresh captures per
run_captures_device call.

usage: python tools/bench_resampler.py [--captures 64] [--samples 10000000] [--reps 10] [--check]
          [--shapes interp4,3/2,2/3,160/147] [--kinds ccf,fff] [--modes FAST,GENERIC]

Shapes: interp4 is gr_interp_fir_filter with I = 4 and a 64-tap prototype (nt 16); I/D is
gr_rational_resampler_base with blks2 design_filter's default taps (fractional_bw 0.4: nt 101).
One JSON line per shape: the algorithmic bytes (every input item read once, every output written once: 8 B each for
ccf/ccc, 4 B for fff) and flops (4 per tap and output for ccf, 2 for fff, 8 for ccc), and the share of the governing
bound max(bytes / 8 TB/s, flops / 157.3 TF/s) that the measured time reaches.  Time: CUDA events around `reps`
launches on one stream after a short ramp; kernel time alone comes from a separate rocprofv3 --kernel-trace --stats
run of this script.  --check compares the first outputs of capture 0 with tests/resampler_ref.py (GENERIC bit for
bit, FAST within 1e-5 of the output peak)."""
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
HBM_BPS, VALU_FLOPS = 8.0e12, 157.3e12

ap = argparse.ArgumentParser()
ap.add_argument("--captures", type=int, default=64)
ap.add_argument("--samples", type=int, default=10_000_000)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--shapes", default="interp4,3/2,2/3,160/147")
ap.add_argument("--kinds", default="ccf,fff")
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
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(reps):
        fn()
    e1.record(st)
    st.synchronize()
    return e0.elapsed_time(e1) / reps


def make(kind, shape, mode):
    if shape.startswith("interp"):
        I = int(shape[len("interp"):])
        taps = np.hanning(16 * I).astype(np.float32) / 8          # a 64-tap prototype at I = 4
        if kind == "ccc":
            taps = taps.astype(np.complex64)
        blk = getattr(g, "interp_fir_filter_" + kind)(I, taps)
        D = 1
    else:
        I, D = (int(v) for v in shape.split("/"))
        blk = getattr(g, "rational_resampler_" + kind)(I, D)       # design_filter(I, D, 0.4)
        taps = blk.taps
    blk.set_mode(getattr(g, "MODE_" + mode))
    return blk, I, D, taps


def check(kind, mode, shape, I, D, taps, x0, y0):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import resampler_ref as rr
    po = grhip_loader.import_oracle()
    M = 20000
    x = x0[:M].cpu().numpy()
    x = x.view(np.complex64).reshape(-1) if kind != "fff" else x.reshape(-1)
    ref = rr.whole_interp(po, I, taps, x) if shape.startswith("interp") else rr.whole_rational(po, I, D, taps, x)
    got = y0[:len(ref)].cpu().numpy()
    got = got.view(np.complex64).reshape(-1) if kind != "fff" else got.reshape(-1)
    if mode == "GENERIC":
        return bool(np.array_equal(got.view(np.uint32), ref.view(np.uint32)))
    return bool(np.abs(got - ref).max() / np.abs(ref).max() < 1e-5)


gen = torch.Generator(device=dev)
for kind in args.kinds.split(","):
    w = 1 if kind == "fff" else 2
    item = 4 * w
    gen.manual_seed(args.seed)
    n, N = args.captures, args.samples
    x = torch.randn((n, N, w), device=dev, generator=gen)       # n captures, synthesised on the device
    for shape in args.shapes.split(","):
        for mode in args.modes.split(","):
            blk, I, D, taps = make(kind, shape, mode)
            nt = blk.history()
            n_out = blk.captures_nout(N)
            y = torch.empty((n, n_out, w), device=dev)
            torch.cuda.synchronize()
            fn = lambda: blk.run_captures_device(n, N, x, N, y, n_out, stream=st)  # noqa: E731
            ms = timeit(fn, args.reps)
            s = ms * 1e-3
            nbytes = float(n) * (N + n_out) * item
            flops = float(n) * n_out * nt * {"ccf": 4, "fff": 2, "ccc": 8}[kind]
            t_bound = max(nbytes / HBM_BPS, flops / VALU_FLOPS)
            line = {"block": ("interp_fir_filter_" if shape.startswith("interp") else "rational_resampler_") + kind,
                    "mode": mode, "I": I, "D": D, "nt": nt, "captures": n, "n_samples": N, "n_out": n_out,
                    "ms": round(ms, 4), "input_Gsamples_per_s": round(n * N / s / 1e9, 2),
                    "flop_per_byte": round(flops / nbytes, 2), "GBps": round(nbytes / s / 1e9, 1),
                    "TFLOPs": round(flops / s / 1e12, 2),
                    "governing": "HBM" if nbytes / HBM_BPS >= flops / VALU_FLOPS else "VALU",
                    "frac_of_bound": round(t_bound / s, 4)}
            if args.check:
                st.synchronize()
                line["check"] = check(kind, mode, shape, I, D, taps, x[0], y[0])
            print(json.dumps(line), flush=True)
            del y
    del x
    torch.cuda.empty_cache()
