"""gr_pfb_synthesis_filterbank_ccf and gr_pfb_interpolator_ccf on one GPU, device resident, beside the channeliser of
the same shape measured in the same process.

usage: python tools/bench_pfb_synth.py [--samples 67108864] [--reps 20] [--modes FAST,GENERIC] [--shapes ...]

Shapes: M:tpf[:numsigs] for the synthesis bank (default list below), interpR:tpf for the interpolator.
One JSON line per shape and mode.  Algorithmic bytes per output sample: 8*numsigs/M read + 8 written (16 with all
streams connected); flops: 4*tpf per output sample for the branches plus the DFT (5 M log2 M per vector for powers of
two, 8 M^2 for the direct sum).  `frac_of_hbm` is bytes / time over 8 TB/s.  For shapes the channeliser's fused kernel
also takes (all streams connected), the channeliser is timed before and after the bank (A, B, A): its two figures
give the run-to-run spread, and `vs_channelizer` is the bank's rate over their mean.  Time: device events around
`reps` launches on one stream after a short ramp; kernel time alone comes from a separate
rocprofv3 --kernel-trace --stats run of this script."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import grhip_loader  # noqa: E402

g = grhip_loader.import_grhip()
HBM_BPS = 8.0e12

ap = argparse.ArgumentParser()
ap.add_argument("--samples", type=int, default=1 << 26, help="output samples per launch")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--modes", default="FAST,GENERIC")
ap.add_argument("--shapes", default="2:32,4:32,8:32,16:32,8:16,8:64,7:32:5,32:31,64:63,interp4:16")
ap.add_argument("--seed", type=int, default=1234)
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


def traffic(M, tpf, numsigs):
    """(bytes, flops) per output sample"""
    dft = 5.0 * math.log2(M) if M & (M - 1) == 0 else 8.0 * M
    return 8.0 * numsigs / M + 8.0, 4.0 * tpf + dft


def proto(M, tpf):
    return (g.workload.lowpass_taps(M * tpf, 0.8 / (2 * M), 1.0) * M).astype(np.float32)


def bench_channelizer(M, tpf, nvec, x):
    ch = g.pfb_channelizer_ccf(M, proto(M, tpf) / M)
    out = torch.empty((nvec, M, 2), device=dev)
    torch.cuda.synchronize()
    ch.general_work_device(nvec, x, x.shape[1], out, st)            # the first call only takes the new taps
    return timeit(lambda: ch.general_work_device(nvec, x, x.shape[1], out, st), args.reps)


gen = torch.Generator(device=dev)
gen.manual_seed(args.seed)
for shape in args.shapes.split(","):
    if shape.startswith("interp"):
        R, tpf = (int(v) for v in shape[len("interp"):].split(":"))
        n_in = args.samples // R
        x = torch.randn((n_in + tpf, 2), device=dev, generator=gen)
        y = torch.empty((n_in * R, 2), device=dev)
        taps = proto(R, tpf)
        for mode in args.modes.split(","):
            lines = []
            for name, blk in (("pfb_interpolator_ccf", g.pfb_interpolator_ccf(R, taps)),
                              ("interp_fir_filter_ccf", g.interp_fir_filter_ccf(R, taps))):
                blk.set_mode(getattr(g, "MODE_" + mode))
                torch.cuda.synchronize()
                ms = timeit(lambda: blk.work_device(n_in * R, x, y, st), args.reps)
                nbytes = 8.0 * n_in + 8.0 * n_in * R
                print(json.dumps({"block": name, "mode": mode, "R": R, "tpf": tpf, "n_out": n_in * R, "ms": round(ms, 4),
                                  "GBps": round(nbytes / ms / 1e6, 1), "frac_of_hbm": round(nbytes / (ms * 1e-3) / HBM_BPS, 4),
                                  "TFLOPs": round(4.0 * tpf * n_in * R / ms / 1e9, 2)}), flush=True)
        del x, y
        continue
    f = [int(v) for v in shape.split(":")]
    M, tpf = f[0], f[1]
    numsigs = f[2] if len(f) > 2 else M
    nvec = args.samples // M
    stride = nvec + tpf + 1
    x = torch.randn((M, stride, 2), device=dev, generator=gen)
    y = torch.empty((nvec * M, 2), device=dev)
    bps, fps = traffic(M, tpf, numsigs)
    with_ch = numsigs == M and 2 <= M <= 16
    for mode in args.modes.split(","):
        blk = g.pfb_synthesis_filterbank_ccf(M, proto(M, tpf))
        blk.set_mode(getattr(g, "MODE_" + mode))
        torch.cuda.synchronize()
        ch_a = bench_channelizer(M, tpf, nvec, x) if with_ch else None
        ms = timeit(lambda: blk.work_device(nvec * M, x, stride, numsigs, y, st), args.reps)
        ch_b = bench_channelizer(M, tpf, nvec, x) if with_ch else None
        nbytes = bps * nvec * M
        line = {"block": "pfb_synthesis_filterbank_ccf", "mode": mode, "M": M, "tpf": tpf, "numsigs": numsigs,
                "n_out": nvec * M, "ms": round(ms, 4), "Gsamples_per_s": round(nvec * M / ms / 1e6, 2),
                "bytes_per_sample": round(bps, 2), "flop_per_byte": round(fps / bps, 2),
                "GBps": round(nbytes / ms / 1e6, 1), "frac_of_hbm": round(nbytes / (ms * 1e-3) / HBM_BPS, 4),
                "TFLOPs": round(fps * nvec * M / ms / 1e9, 2)}
        if with_ch:
            cb = 16.0 * nvec * M
            line["channelizer_ms"] = [round(ch_a, 4), round(ch_b, 4)]
            line["channelizer_frac_of_hbm"] = [round(cb / (t * 1e-3) / HBM_BPS, 4) for t in (ch_a, ch_b)]
            line["vs_channelizer"] = round(0.5 * (ch_a + ch_b) / ms, 3)
        print(json.dumps(line), flush=True)
    del x, y
    torch.cuda.empty_cache()
