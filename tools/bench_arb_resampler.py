"""gr_pfb_arb_resampler_ccf / _fff on one GPU, device resident: n fresh captures per run_captures_device call.

usage: python tools/bench_arb_resampler.py [--captures 64] [--samples 10000000] [--reps 10] [--check]
          [--tpf 8,16,32] [--rates 0.0192,0.5,1.25] [--kinds ccf,fff] [--modes FAST,GENERIC]

One JSON line per shape: input Gsamples/s, the algorithmic bytes ((8 + 8*rate) B per input sample for ccf,
(4 + 4*rate) for fff: every input read once, every output written once) as a fraction of 8 TB/s, and the
rate-bound flops (8*tpf + 4 per ccf output, 4*tpf + 2 per fff output: two dot products and the blend).
--check compares the first outputs of capture 0 with the restatement in tests/arb_resampler_ref.py (GENERIC bit for
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
wl = g.workload

ap = argparse.ArgumentParser()
ap.add_argument("--captures", type=int, default=64)
ap.add_argument("--samples", type=int, default=10_000_000)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--R", type=int, default=32)
ap.add_argument("--tpf", default="8,16,32")
ap.add_argument("--rates", default="0.0192,0.5,1.25")
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


def check(kind, mode, rate, taps, R, x0, got0):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import arb_resampler_ref as ar
    M = 20000
    x = x0[:M].cpu().numpy()
    x = x.view(np.complex64).reshape(-1) if kind == "ccf" else x.reshape(-1)
    tpf, fwd, dfwd = ar.banks(taps, R)
    counts, js, accs = ar.whole_stream_schedule(R, rate, M)
    ref = ar.eval_schedule(fwd, dfwd, np.concatenate([np.zeros(tpf, x.dtype), x]), counts, js, accs)
    got = got0[:len(ref)].cpu().numpy()
    got = got.view(np.complex64).reshape(-1) if kind == "ccf" else got.reshape(-1)
    if mode == "GENERIC":
        return bool(np.array_equal(got.view(np.uint32), ref.view(np.uint32)))
    return bool(np.abs(got - ref).max() / np.abs(ref).max() < 1e-5)


gen = torch.Generator(device=dev)
for kind in args.kinds.split(","):
    w = 2 if kind == "ccf" else 1
    gen.manual_seed(args.seed)
    n, N = args.captures, args.samples
    x = torch.randn((n, N, w), device=dev, generator=gen)       # n captures, synthesised on the device
    for tpf in [int(v) for v in args.tpf.split(",")]:
        R = args.R
        taps = wl.lowpass_taps(R * tpf, 0.4, float(R))
        for rate in [float(v) for v in args.rates.split(",")]:
            for mode in args.modes.split(","):
                blk = (g.pfb_arb_resampler_ccf if kind == "ccf" else g.pfb_arb_resampler_fff)(rate, taps, R)
                blk.set_mode(getattr(g, "MODE_" + mode))
                n_out = blk.captures_nout(N)
                y = torch.empty((n, n_out, w), device=dev)
                torch.cuda.synchronize()
                fn = lambda: blk.run_captures_device(n, N, x, N, y, n_out, stream=st)  # noqa: E731
                ms = timeit(fn, args.reps)
                nin = n * N
                bytes_in = 4 * w * (1.0 + rate)
                gbs = nin * bytes_in / (ms * 1e-3) / 1e9
                flops = n * n_out * ((8 * tpf + 4) if kind == "ccf" else (4 * tpf + 2))
                line = {"block": "pfb_arb_resampler_" + kind, "mode": mode, "R": R, "tpf": tpf, "rate": rate,
                        "captures": n, "n_samples": N, "n_out": n_out, "ms": round(ms, 4),
                        "input_Gsamples_per_s": round(nin / ms / 1e6, 2), "algorithmic_GBps": round(gbs, 1),
                        "frac_of_8TBps": round(gbs / 8000.0, 4), "TFLOPs": round(flops / (ms * 1e-3) / 1e12, 2)}
                if args.check:
                    st.synchronize()
                    line["check"] = check(kind, mode, rate, taps, R, x[0], y[0])
                print(json.dumps(line), flush=True)
                del y
    del x
    torch.cuda.empty_cache()
