#!/usr/bin/env python
"""Speed of the AM demodulator hier block: demod_10k0a3e_cf(16e3, 1) in FAST mode (the fused kernel, 83 taps, no
decimation) against
  (a) the two handles it replaces run one after the other on the same device data -- complex_to_mag and
      fir_filter_fff(1, taps) FAST (the add of -1 is left out: it would only add a pass to this side), and
  (b) fir_filter_fff(1, taps) FAST alone with the same taps on the same number of samples.

    python tools/bench_am_demod.py [--captures 64] [--samples 10000000] [--reps 5]

Two aims.  The fused kernel is no slower than (b): its FIR step is then not bound by LDS reads; the margin is the
spread of the two A legs.  The fused kernel is faster than (a), which moves 20 bytes per sample where it moves 12.

Ordering is A-B-A (fused, the yardstick, fused again) for each yardstick, so that a drift of the clocks shows as a
difference between the A legs; every leg is the median of --reps timed calls after one untimed call.  Times come from
device events around work_device calls on one (non-default) stream; nothing is copied to the host inside a timed
region.  Prints one line per figure and a JSON summary last."""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import grhip_loader  # noqa: E402

HBM_BYTES_PER_S = 8e12


def timed(torch, stream, fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--captures", type=int, default=64)
    ap.add_argument("--samples", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    g = grhip_loader.import_grhip()
    if g.device_count() < 1:
        raise SystemExit("bench_am_demod: no HIP device visible")
    S, n = args.captures, args.samples
    total = S * n

    # one capture: a carrier with 50 % tone modulation; every capture gets it
    t = torch.arange(n, device="cuda", dtype=torch.float64)
    env = 1.0 + 0.5 * torch.sin(2 * math.pi * 0.013 * t)
    one = torch.polar(env, 0.31 * t).to(torch.complex64)
    del t, env
    x = one.repeat(S)
    del one

    rx = g.demod_10k0a3e_cf(16e3, 1)
    rx.set_mode(g.MODE_FAST)
    rx.set_streams(S)
    taps = rx.audio_taps
    assert rx.engine() == 1 and len(taps) == 83 and rx.produced(n) == n
    H = len(taps) - 1
    out = torch.zeros(total, dtype=torch.float32, device="cuda")
    # a stream of its own: the default stream's handle is 0, which the library reads as "the handle's own stream"
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()

    def fused():
        rx.work_device(n, x, out, None, stream)

    mag = g.complex_to_mag()
    fir = g.fir_filter_fff(1, taps)
    fir.set_mode(g.MODE_FAST)
    m = torch.zeros(total + H, dtype=torch.float32, device="cuda")      # the FIR's history in front
    out2 = torch.zeros(total, dtype=torch.float32, device="cuda")

    # both take the captures as one long stream (the seams cost nothing); the FIR takes at most 2 GiB of input per call
    piece = max(1, (1 << 28) // n) * n
    pieces = [(c, min(piece, total - c)) for c in range(0, total, piece)]

    def fir_alone():
        for c, k in pieces:
            fir.work_device(k, m[c:], out2[c:], stream)

    def two():
        mag.work_device(total, x, m[H:], stream)
        fir_alone()

    res = {"captures": S, "samples": n, "decim": 1, "ntaps": H + 1}
    res["fused_ms_a1"] = timed(torch, stream, fused, args.reps)
    res["two_handles_ms"] = timed(torch, stream, two, args.reps)
    res["fused_ms_a2"] = timed(torch, stream, fused, args.reps)
    res["fir_alone_ms"] = timed(torch, stream, fir_alone, args.reps)
    res["fused_ms_a3"] = timed(torch, stream, fused, args.reps)
    res["complex_to_mag_ms"] = timed(torch, stream, lambda: mag.work_device(total, x, m[H:], stream), args.reps)
    legs = [res["fused_ms_a1"], res["fused_ms_a2"], res["fused_ms_a3"]]
    fused_ms, spread = max(legs), (max(legs) - min(legs)) / min(legs)
    res["fused_spread"] = spread
    res["fused_over_two_handles"] = fused_ms / res["two_handles_ms"]
    res["fused_over_fir_alone"] = fused_ms / res["fir_alone_ms"]
    res["fused_fraction_of_8TBps"] = total * 12.0 / (fused_ms * 1e-3) / HBM_BYTES_PER_S
    res["fused_Msamples_per_s"] = total / (fused_ms * 1e-3) / 1e6

    print("fused demod_10k0a3e_cf(16e3, 1), %d x %d samples: %.2f, %.2f and %.2f ms (A legs, spread %.1f %%)"
          % (S, n, legs[0], legs[1], legs[2], 100 * spread))
    print("  (a) complex_to_mag -> fir_filter_fff FAST: %.2f ms (complex_to_mag alone %.2f ms)"
          % (res["two_handles_ms"], res["complex_to_mag_ms"]))
    print("  (b) fir_filter_fff FAST alone: %.2f ms" % res["fir_alone_ms"])
    print("  fused / (b) = %.3f (aim: at most 1 within the spread): %s"
          % (res["fused_over_fir_alone"], "met" if res["fused_over_fir_alone"] <= 1.0 + spread else "missed"))
    print("  fused / (a) = %.3f (aim: below 1): %s"
          % (res["fused_over_two_handles"], "met" if res["fused_over_two_handles"] < 1.0 else "missed"))
    print("  fused: %.0f Msamples/s, %.1f %% of 8 TB/s at 12 bytes per sample"
          % (res["fused_Msamples_per_s"], 100 * res["fused_fraction_of_8TBps"]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
