#!/usr/bin/env python
"""Speed of the FM demodulator hier block: nbfm_rx(8000, 32000) in FAST mode (the fused kernel) against the three
handles it replaces run one after the other on the same device data -- quadrature_demod_cf, iir_filter_ffd (FAST, the
chunked form) and fir_filter_fff(4, taps) (FAST) -- and iir_filter_ffd FAST against GENERIC on one stream.

    python tools/bench_fm_demod.py [--captures 64] [--samples 10000000] [--reps 5]

Ordering is A-B-A (fused, three handles, fused again) so that a drift of the clocks shows as a difference between the
two A legs; every leg is the median of --reps timed calls after one untimed call.  Times come from device events
around work_device calls on one (non-default) stream; nothing is copied to the host inside a timed region.  Prints one line per
figure and a JSON summary last."""
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
    return float(np.median(ms)), ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--captures", type=int, default=64)
    ap.add_argument("--samples", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    g = grhip_loader.import_grhip()
    if g.device_count() < 1:
        raise SystemExit("bench_fm_demod: no HIP device visible")
    S, n, D = args.captures, args.samples, 4
    total = S * n

    # one capture: a frequency-modulated carrier; every capture gets it
    t = torch.arange(n, device="cuda", dtype=torch.float64)
    audio = 0.6 * torch.sin(2 * math.pi * 0.011 * t) + 0.3 * torch.sin(2 * math.pi * 0.037 * t)
    phase = torch.cumsum(0.9 * audio, 0)
    one = torch.polar(torch.ones_like(phase), phase).to(torch.complex64)
    del t, audio, phase
    # one history item in front for the stand-alone demodulator
    buf = torch.zeros(total + 1, dtype=torch.complex64, device="cuda")
    buf[1:] = one.repeat(S)
    x = buf[1:]
    del one

    rx = g.nbfm_rx(8000, 32000)
    rx.set_mode(g.MODE_FAST)
    rx.set_streams(S)
    assert rx.engine() == 1 and rx.audio_decim == D
    n_out = rx.produced(n)
    out = torch.zeros(S * n_out, dtype=torch.float32, device="cuda")
    # a stream of its own: the default stream's handle is 0, which the library reads as "the handle's own stream"
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()

    def fused():
        rx.work_device(n, x, out, None, stream)

    qd = g.quadrature_demod_cf(rx.k)
    b, a = g.fm_deemph_taps(32000, 75e-6)
    iir = g.iir_filter_ffd(b, a)
    iir.set_mode(g.MODE_FAST)
    iir.set_streams(S)
    assert iir.chunked()
    fir = g.fir_filter_fff(D, rx.audio_taps)
    fir.set_mode(g.MODE_FAST)
    H = len(rx.audio_taps) - 1
    q = torch.zeros(total, dtype=torch.float32, device="cuda")
    y = torch.zeros(total + H, dtype=torch.float32, device="cuda")      # the FIR's history in front
    out3 = torch.zeros((total // D), dtype=torch.float32, device="cuda")

    def three():
        # the demodulator and the FIR take the captures as one long stream: the seams cost nothing
        qd.work_device(total, buf, q, stream)
        iir.work_device(n, q, y[H:], stream)
        fir.work_device(total // D, y, out3, stream)

    res = {"captures": S, "samples": n, "decim": D, "ntaps": H + 1}
    res["fused_ms_a1"], _ = timed(torch, stream, fused, args.reps)
    res["three_ms"], _ = timed(torch, stream, three, args.reps)
    res["fused_ms_a2"], _ = timed(torch, stream, fused, args.reps)
    parts = {}
    parts["quadrature_demod_cf"], _ = timed(torch, stream, lambda: qd.work_device(total, buf, q, stream), args.reps)
    parts["iir_filter_ffd FAST"], _ = timed(torch, stream, lambda: iir.work_device(n, q, y[H:], stream), args.reps)
    parts["fir_filter_fff FAST"], _ = timed(torch, stream, lambda: fir.work_device(total // D, y, out3, stream), args.reps)
    res["parts_ms"] = parts
    fused_ms = max(res["fused_ms_a1"], res["fused_ms_a2"])
    res["fused_over_three"] = fused_ms / res["three_ms"]
    bytes_moved = total * (8 + 4.0 / D)
    res["fused_fraction_of_8TBps"] = bytes_moved / (fused_ms * 1e-3) / HBM_BYTES_PER_S
    res["fused_Msamples_per_s"] = total / (fused_ms * 1e-3) / 1e6

    # iir_filter_ffd on one stream: the chunked form against the serial walk
    one_n = min(n, total)
    i1 = g.iir_filter_ffd(b, a)
    o1 = torch.zeros(one_n, dtype=torch.float32, device="cuda")
    for name, mode in (("iir_one_stream_fast_ms", g.MODE_FAST), ("iir_one_stream_generic_ms", g.MODE_GENERIC)):
        i1.set_mode(mode)
        res[name], _ = timed(torch, stream, lambda: i1.work_device(one_n, q, o1, stream), max(2, args.reps // 2))
    res["iir_generic_over_fast"] = res["iir_one_stream_generic_ms"] / res["iir_one_stream_fast_ms"]

    print("fused nbfm_rx(8000, 32000), %d x %d samples: %.2f ms and %.2f ms (A legs), three handles %.2f ms (B)"
          % (S, n, res["fused_ms_a1"], res["fused_ms_a2"], res["three_ms"]))
    print("  the three handles alone: " + ", ".join("%s %.2f ms" % kv for kv in parts.items()))
    print("  fused / three = %.3f (aim: at most 0.5): %s" % (res["fused_over_three"], "met" if res["fused_over_three"] <= 0.5 else "missed"))
    print("  fused: %.0f Msamples/s, %.1f %% of 8 TB/s at %.2f bytes per sample"
          % (res["fused_Msamples_per_s"], 100 * res["fused_fraction_of_8TBps"], 8 + 4.0 / D))
    print("iir_filter_ffd, one stream of %d: FAST %.3f ms, GENERIC %.3f ms (x %.1f)"
          % (one_n, res["iir_one_stream_fast_ms"], res["iir_one_stream_generic_ms"], res["iir_generic_over_fast"]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
