"""Real-input FIR kinds on one GPU, device resident: freq_xlating_fir_filter_fcf / _scf (256 taps, D = 4),
fir_filter_fcc (64 taps, D = 1) and fir_filter_fsf (64 taps, D = 1).

usage: python tools/bench_realin.py [--samples 40000000] [--reps 10] [--shapes xlating_fcf,xlating_scf,fir_fcc,fir_fsf]
          [--modes FAST]

One JSON line per shape and mode.  Algorithmic bytes: every input item read once (4 B float, 2 B int16), every output
written once (8 B complex, 2 B short), plus 8 B per output for the rotator phase table of the xlating kinds.  Flops: 4
per tap and output for complex taps, 2 for fsf.  The governing bound is max(bytes / 8 TB/s, flops / 157.3 TF/s); the
line carries the measured share of it.  fsf is reported only (its FAST form is fff's engines + a conversion pass).
For the xlating shapes the same run times what a user would otherwise build: widen the items to complex on the device,
then the _ccc block.  Each timed call follows reset(), so the rotator table (built on the host at ~3 ns per output, as
for _ccc) is already there; the first, untimed call builds it.  Time: CUDA events around `reps` calls on one stream."""
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
ap.add_argument("--samples", type=int, default=40_000_000)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--shapes", default="xlating_fcf,xlating_scf,fir_fcc,fir_fsf")
ap.add_argument("--modes", default="FAST")
args = ap.parse_args()

dev = torch.device("cuda", 0)
st = torch.cuda.Stream(device=dev)
SHAPES = {  # name: (class, ntaps, decim, item dtype, complex taps?, xlating?)
    "xlating_fcf": ("freq_xlating_fir_filter_fcf", 256, 4, np.float32, False, True),
    "xlating_scf": ("freq_xlating_fir_filter_scf", 256, 4, np.int16, False, True),
    "fir_fcc": ("fir_filter_fcc", 64, 1, np.float32, True, False),
    "fir_fsf": ("fir_filter_fsf", 64, 1, np.float32, False, False),
}


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


rng = np.random.default_rng(7)
for name in args.shapes.split(","):
    cname, T, D, dt, ctaps, xl = SHAPES[name]
    proto = (np.sinc(0.05 * (np.arange(T) - (T - 1) / 2)) * 0.05).astype(np.float32)
    taps = (proto * np.exp(0.2j * np.arange(T))).astype(np.complex64) if ctaps else proto
    nout = args.samples // D
    n_in = (nout - 1) * D + T
    if dt == np.int16:
        x = rng.integers(-32768, 32768, n_in).astype(np.int16)
    else:
        x = rng.standard_normal(n_in).astype(np.float32)
    dx = torch.from_numpy(x).to(dev)
    out_dt = torch.int16 if name == "fir_fsf" else torch.complex64
    dy = torch.empty(nout, dtype=out_dt, device=dev)
    in_b, out_b = x.itemsize, (2 if name == "fir_fsf" else 8)
    bytes_ = n_in * in_b + nout * out_b + (nout * 8 if xl else 0)
    flops = float(nout) * T * (2 if name == "fir_fsf" else 4)
    for mode in args.modes.split(","):
        blk = getattr(g, cname)(D, taps, 2500.0, 48000.0) if xl else getattr(g, cname)(D, taps)
        blk.set_mode(getattr(g, "MODE_" + mode))
        if xl:
            def call():
                blk.reset()
                blk.work_device(nout, dx.data_ptr(), dy.data_ptr(), st)
        else:
            def call():
                blk.work_device(nout, dx.data_ptr(), dy.data_ptr(), st)
        with torch.cuda.stream(st):
            call()
            st.synchronize()
            ms = timeit(call, args.reps)
        t_hbm, t_valu = bytes_ / HBM_BPS, flops / VALU_FLOPS
        bound = "HBM" if t_hbm >= t_valu else "VALU"
        rec = {"shape": name, "mode": mode, "ntaps": T, "decim": D, "n_in": n_in, "n_out": nout, "ms": round(ms, 4),
               "gsamples_per_s": round(n_in / ms / 1e6, 1), "bytes": bytes_, "flops": flops,
               "hbm_bound_gsps": round(n_in / t_hbm / 1e9, 1), "valu_bound_gsps": round(n_in / t_valu / 1e9, 1),
               "governs": bound, "fraction_of_bound": round(max(t_hbm, t_valu) * 1e3 / ms, 3)}
        if name == "fir_fsf":
            rec["governs"], rec["note"] = "reported only", "fff engines + conversion pass"
        if xl:
            base = g.freq_xlating_fir_filter_ccc(D, proto.astype(np.complex64), 2500.0, 48000.0)
            base.set_mode(getattr(g, "MODE_" + mode))
            wide = torch.empty(n_in, dtype=torch.complex64, device=dev)
            dyb = torch.empty(nout, dtype=torch.complex64, device=dev)

            def bcall():
                wide.copy_(dx)                  # widen to complex on the device (imaginary part 0)
                base.reset()
                base.work_device(nout, wide.data_ptr(), dyb.data_ptr(), st)
            with torch.cuda.stream(st):
                bcall()
                st.synchronize()
                bms = timeit(bcall, args.reps)
            rec["baseline_widen_ccc_ms"] = round(bms, 4)
            rec["speedup_vs_baseline"] = round(bms / ms, 3)
        print(json.dumps(rec), flush=True)
