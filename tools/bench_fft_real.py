"""gr_fft_filter_fff and gr_fft_vfc on one GPU, device resident, beside their nearest siblings measured in the same
process.

usage: python tools/bench_fft_real.py [--captures 64] [--samples 10000000] [--ntaps 256] [--decims 1,4] [--reps 5]

fft_filter_fff: `captures` successive work_device calls of `samples` floats each (rounded down to the output
multiple), one stream, the history carried from call to call.  Algorithmic bytes per input sample: 4 read + 4/D
written.  Two comparison figures per decimation, timed before and after the block (A, B, A: the two figures give the
run-to-run spread):
  fir_filter_fff FAST   the same taps and decimation: at 256 taps (D = 1: more than 176 taps per phase; D = 4: no tiled
                        float kernel above D = 2) its dispatch is the single-block real overlap-save kernel, one real
                        block per 4096-point transform
  fft_filter_ccc        the same taps given as complex, on complex noise: one complex block per transform, 8 + 8/D B/sample
`blocks_per_s` is engine blocks (4096-point transforms' worth of input: L = ((4096 - ntaps + 1) / D) D samples) per second;
`transforms_per_s` is 4096-point transforms per second: blocks_per_s for the two single-block kernels, half of it for
the paired one.  The aim of the paired kernel is fft_filter_ccc's transforms_per_s (then twice fir_filter_fff's samples per
second); `vs_fft_filter_ccc_transforms` is that ratio (aim 1.0), `vs_fir_filter_fff` the ratio of samples per second.
fft_vfc: 4096 points x 4096 vectors against fft_vcc of the same size (12 against 16 B/sample).
One JSON line per measurement.  `frac_of_hbm` is bytes / time over 8 TB/s.  Time: device events around `reps` passes on
one stream after a short ramp; kernel time alone comes from a separate rocprofv3 --kernel-trace --stats run."""
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
HBM_BPS = 8.0e12

ap = argparse.ArgumentParser()
ap.add_argument("--captures", type=int, default=64)
ap.add_argument("--samples", type=int, default=10_000_000, help="floats per capture")
ap.add_argument("--ntaps", type=int, default=256)
ap.add_argument("--decims", default="1,4")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--seed", type=int, default=1234)
args = ap.parse_args()

dev = torch.device("cuda", 0)
st = torch.cuda.Stream(device=dev)
gen = torch.Generator(device=dev)
gen.manual_seed(args.seed)


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


def line(block, decim, ms, n_in, bytes_per_sample, L, per_transform=1, **extra):
    d = {"transforms_per_s": round(n_in / L / per_transform / (ms * 1e-3), 1),
         "block": block, "ntaps": args.ntaps, "decim": decim, "captures": args.captures, "n_in": n_in, "ms": round(ms, 4),
         "Gsamples_per_s": round(n_in / ms / 1e6, 2), "blocks_per_s": round(n_in / L / (ms * 1e-3), 1),
         "bytes_per_sample": bytes_per_sample, "GBps": round(bytes_per_sample * n_in / ms / 1e6, 1),
         "frac_of_hbm": round(bytes_per_sample * n_in / (ms * 1e-3) / HBM_BPS, 4)}
    d.update(extra)
    print(json.dumps(d), flush=True)
    return d


taps = g.workload.lowpass_taps(args.ntaps, 0.1, 1.0).astype(np.float32)
H = args.ntaps - 1
for decim in (int(v) for v in args.decims.split(",")):
    blk = g.fft_filter_fff(decim, taps)
    ns = blk.nsamples()
    L = ((4096 - H) // decim) * decim
    nout = (args.samples // (ns * decim)) * ns            # outputs per capture
    nin = nout * decim
    tot = nin * args.captures
    x = torch.randn((H + tot,), device=dev, generator=gen)
    y = torch.empty((nout * args.captures,), device=dev)
    fir = g.fir_filter_fff(decim, taps)
    ccc = g.fft_filter_ccc(decim, taps.astype(np.complex64))
    xc = torch.randn((tot, 2), device=dev, generator=gen)
    yc = torch.empty((nout * args.captures, 2), device=dev)
    torch.cuda.synchronize()

    def run_fff():
        for c in range(args.captures):
            blk.work_device(nout, x[H + c * nin:], y[c * nout:], st)

    def run_fir():                                       # history in front of every call's input
        for c in range(args.captures):
            fir.work_device(nout, x[c * nin:], y[c * nout:], st)

    def run_ccc():
        for c in range(args.captures):
            ccc.work_device(nout, xc[c * nin:], yc[c * nout:], st)

    bps_r, bps_c = 4.0 + 4.0 / decim, 8.0 + 8.0 / decim
    fir_a = timeit(run_fir, args.reps)
    ccc_a = timeit(run_ccc, args.reps)
    ms = timeit(run_fff, args.reps)
    fir_b = timeit(run_fir, args.reps)
    ccc_b = timeit(run_ccc, args.reps)
    for tag, t in (("A", fir_a), ("B", fir_b)):
        line("fir_filter_fff FAST (single-block real engine) " + tag, decim, t, tot, bps_r, L)
    for tag, t in (("A", ccc_a), ("B", ccc_b)):
        line("fft_filter_ccc (taps as complex) " + tag, decim, t, tot, bps_c, L)
    line("fft_filter_fff (paired blocks)", decim, ms, tot, bps_r, L, per_transform=2,
         vs_fir_filter_fff=round(0.5 * (fir_a + fir_b) / ms, 3), vs_fft_filter_ccc_transforms=round(0.5 * (ccc_a + ccc_b) / ms / 2, 3))
    del x, y, xc, yc, blk, fir, ccc
    torch.cuda.empty_cache()

# ---- fft_vfc against fft_vcc, 4096 points
N, nvec = 4096, 4096
xr = torch.randn((N * nvec,), device=dev, generator=gen)
xv = torch.randn((N * nvec, 2), device=dev, generator=gen)
yv = torch.empty((N * nvec, 2), device=dev)
vfc, vcc = g.fft_vfc(N, True, []), g.fft_vcc(N, True, [], False)
torch.cuda.synchronize()
vcc_a = timeit(lambda: vcc.work_device(nvec, xv, yv, st), 20)
ms = timeit(lambda: vfc.work_device(nvec, xr, yv, st), 20)
vcc_b = timeit(lambda: vcc.work_device(nvec, xv, yv, st), 20)
for name, t, b in (("fft_vcc 4096 A", vcc_a, 16.0), ("fft_vcc 4096 B", vcc_b, 16.0), ("fft_vfc 4096", ms, 12.0)):
    print(json.dumps({"block": name, "nvec": nvec, "ms": round(t, 4), "Gsamples_per_s": round(N * nvec / t / 1e6, 2),
                      "bytes_per_sample": b, "GBps": round(b * N * nvec / t / 1e6, 1),
                      "frac_of_hbm": round(b * N * nvec / (t * 1e-3) / HBM_BPS, 4)}), flush=True)
print(json.dumps({"fft_vfc_vs_fft_vcc_samples_per_s": round(0.5 * (vcc_a + vcc_b) / ms, 3)}), flush=True)
