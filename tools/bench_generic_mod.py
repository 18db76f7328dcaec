"""generic_mod on one GPU, device resident: S streams of bytes per work_device call, FAST mode.

usage: python tools/bench_generic_mod.py [--streams 64] [--out-mib 1024] [--reps 10] [--cases dqpsk,qam16] [--sps 2,2.5,4]

Per case one JSON line with the time of a call for engine 1 (the fused kernel), engine 0 (the five blocks in a row) and
pfb_arb_resampler_ccf alone on ready-made symbols with the same taps and rate (run_captures_device, FAST), all in the
same run: legs A (engine 1), B (engine 0), R (the resampler), A again; `spread` is the two A legs' difference over their
mean.  The batch is sized by its output (--out-mib, which dominates).  `frac_of_8TBps` is engine 1's algorithmic
traffic, k/8 bytes in and 8 * sps out per symbol, over 8 TB/s.  Two aims, reported as met or missed, never asserted:
  (a) engine 1 is no slower than the resampler alone (it writes the same bytes and reads 8 per symbol fewer);
  (b) engine 1 takes at most half of engine 0's time."""
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
ap.add_argument("--streams", type=int, default=64)
ap.add_argument("--out-mib", type=int, default=1024)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--cases", default="dqpsk,qam16")
ap.add_argument("--sps", default="2,2.5,4")
ap.add_argument("--seed", type=int, default=1234)
args = ap.parse_args()

dev = torch.device("cuda", 0)
st = torch.cuda.Stream(device=dev)
CONS = {"dqpsk": lambda: g.constellation_dqpsk(), "qam16": lambda: g.qam_constellation(16), "bpsk": lambda: g.constellation_bpsk(),
        "8psk": lambda: g.constellation_8psk(), "qam64": lambda: g.qam_constellation(64)}


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


gen = torch.Generator(device=dev)
gen.manual_seed(args.seed)
S = args.streams
for name in args.cases.split(","):
    for sps in [float(v) for v in args.sps.split(",")]:
        c = CONS[name]()
        k = c.bits_per_symbol()
        nsym = int(args.out_mib * 2 ** 20 / 8 / sps / S) // 8 * 8
        n_bytes = nsym * k // 8
        d_in = torch.randint(0, 256, (S, n_bytes), device=dev, dtype=torch.uint8, generator=gen)
        mods = []
        for engine in (1, 0):
            m = g.generic_mod(c, sps, True)
            m.set_mode(g.MODE_FAST)
            m.set_streams(S)
            m.set_engine(engine)
            mods.append(m)
        n_out = mods[0].max_produced(n_bytes)
        d_out = torch.empty((S, n_out), device=dev, dtype=torch.complex64)
        arb = g.pfb_arb_resampler_ccf(sps, mods[0].taps(), 32)
        arb.set_mode(g.MODE_FAST)
        d_sym = torch.randn((S, nsym, 2), device=dev, generator=gen)
        n_arb = arb.captures_nout(nsym)
        torch.cuda.synchronize()
        legs = {}
        for leg, fn in (("A1", lambda: mods[0].work_device(n_bytes, d_in, d_out, n_out, n_out, stream=st)),
                        ("B", lambda: mods[1].work_device(n_bytes, d_in, d_out, n_out, n_out, stream=st)),
                        ("R", lambda: arb.run_captures_device(S, nsym, d_sym, nsym, d_out, n_out, stream=st)),
                        ("A2", lambda: mods[0].work_device(n_bytes, d_in, d_out, n_out, n_out, stream=st))):
            legs[leg] = timeit(fn, args.reps)
        e1 = 0.5 * (legs["A1"] + legs["A2"])
        spread = abs(legs["A1"] - legs["A2"]) / e1
        gbs = S * nsym * (k / 8.0 + 8.0 * sps) / (e1 * 1e-3) / 1e9
        line = {"block": "generic_mod", "constellation": name, "bits_per_symbol": k, "sps": sps, "mode": "FAST", "streams": S,
                "n_bytes": n_bytes, "symbols": nsym, "n_out": n_out, "resampler_n_out": n_arb,
                "engine1_ms": round(e1, 4), "engine1_legs_ms": [round(legs["A1"], 4), round(legs["A2"], 4)], "spread": round(spread, 4),
                "engine0_ms": round(legs["B"], 4), "resampler_alone_ms": round(legs["R"], 4),
                "engine1_Gsymbols_per_s": round(S * nsym / e1 / 1e6, 2), "algorithmic_GBps": round(gbs, 1),
                "frac_of_8TBps": round(gbs / 8000.0, 4),
                "engine1_over_resampler": round(e1 / legs["R"], 3), "aim_a_no_slower_than_resampler": "met" if e1 <= legs["R"] * (1 + spread) else "missed",
                "engine1_over_engine0": round(e1 / legs["B"], 3), "aim_b_at_most_half_of_engine0": "met" if e1 <= 0.5 * legs["B"] else "missed"}
        print(json.dumps(line), flush=True)
        del d_in, d_out, d_sym, mods, arb
        torch.cuda.empty_cache()
