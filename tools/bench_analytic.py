"""hilbert_fc, filter_delay_fc and goertzel_fc on one GPU, device resident.

usage: python tools/bench_analytic.py [--captures 64] [--samples 10000000] [--reps 20] [--ntaps 19,63,255]
          [--dense 64,255] [--skip-generic]

One JSON line per measurement: the median of --reps timed runs (each between its own pair of events, after a ramp of
untimed runs) of `captures` work_device calls of `samples` floats each.
  hilbert_fc FAST / GENERIC at each --ntaps, Gsamples/s and the fraction of 8 TB/s at 12 B per sample (4 in, 8 out),
    beside fir_filter_fcc FAST with taps delta(h) + j hilbert(ntaps) on the same data in the same run -- how an
    analytic signal was made before this block -- timed before and after; "speedup_vs_fir_filter_fcc" is the ratio.
  filter_delay_fc FAST with random taps (the dense kernel) at each --dense length.
  goertzel_fc, both modes: len 400 on all captures (many blocks) and len 8000 on ONE capture (1250 blocks at the
    default size: the shape the FAST split exists for), as a fraction of 8 TB/s at 4 B per sample."""
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
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--ntaps", default="19,63,255")
ap.add_argument("--dense", default="64,255")
ap.add_argument("--seed", type=int, default=1234)
ap.add_argument("--skip-generic", action="store_true")
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
    return float(np.median(ms))


def line(block, mode, ms, nsamp, bytes_per_sample, **kw):
    gs = nsamp / ms / 1e6
    d = {"block": block, "mode": mode, "ms_median": round(ms, 4), "Gsamples_per_s": round(gs, 2),
         "frac_of_8TBps": round(gs * bytes_per_sample / 8000.0, 4)}
    d.update(kw)
    print(json.dumps(d), flush=True)
    return gs


n, N = args.captures, args.samples
gen = torch.Generator(device=dev)
gen.manual_seed(args.seed)
x = torch.randn((n, N), device=dev, generator=gen)
y = torch.empty((n, N, 2), device=dev)
modes = ["FAST"] + ([] if args.skip_generic else ["GENERIC"])


def sync_runner(blk, nt, delay_form=False):
    nout = N - nt + 1

    def fn():
        for c in range(n):
            if delay_form:        # filter_delay_fc: (in0, in1 = none, out)
                blk.work_device(nout, x[c], None, y[c], stream=st)
            else:
                blk.work_device(nout, x[c], y[c], stream=st)
    return fn, nout * n


for nt in [int(v) for v in args.ntaps.split(",")]:
    hil = g.firdes_hilbert(nt)
    ct = (1j * hil).astype(np.complex64)
    ct[nt // 2] += 1.0
    fcc = g.fir_filter_fcc(1, ct)
    fcc.set_mode(g.MODE_FAST)
    fn_fcc, tot = sync_runner(fcc, nt)
    fcc_a = timeit(fn_fcc, args.reps)
    res = {}
    for mode in modes:
        blk = g.hilbert_fc(nt)
        blk.set_mode(getattr(g, "MODE_" + mode))
        fn, tot = sync_runner(blk, nt)
        res[mode] = timeit(fn, args.reps)
    fcc_b = timeit(fn_fcc, args.reps)
    fcc_ms = 0.5 * (fcc_a + fcc_b)
    line("fir_filter_fcc delta+j*hilbert", "FAST", fcc_ms, tot, 12.0, ntaps=nt, ms_before=round(fcc_a, 4), ms_after=round(fcc_b, 4))
    for mode in modes:
        line("hilbert_fc", mode, res[mode], tot, 12.0, ntaps=nt, speedup_vs_fir_filter_fcc=round(fcc_ms / res[mode], 3))

for nt in [int(v) for v in args.dense.split(",") if v]:
    taps = np.random.default_rng(args.seed).standard_normal(nt).astype(np.float32)
    blk = g.filter_delay_fc(taps)
    blk.set_mode(g.MODE_FAST)
    fn, tot = sync_runner(blk, nt, delay_form=True)
    line("filter_delay_fc (dense)", "FAST", timeit(fn, args.reps), tot, 12.0, ntaps=nt)

del y
torch.cuda.empty_cache()
for ln, caps in ((400, n), (8000, 1)):
    nb = N // ln
    out = torch.empty((caps, nb, 2), device=dev)
    res = {}
    for mode in modes:
        blk = g.goertzel_fc(8000, ln, 100.0)
        blk.set_mode(getattr(g, "MODE_" + mode))

        def fn():
            for c in range(caps):
                blk.work_device(nb, x[c], out[c], stream=st)
        res[mode] = timeit(fn, args.reps)
    for mode in modes:
        extra = {"fast_vs_generic": round(res["GENERIC"] / res["FAST"], 3)} if mode == "FAST" and "GENERIC" in res else {}
        line("goertzel_fc", mode, res[mode], caps * nb * ln, 4.0, len=ln, captures=caps, blocks_per_call=nb, **extra)
    del out
