"""The continuous-phase transmitter on one GPU, device resident, A-B-A in one run.

usage: python tools/bench_cpm_mod.py [--streams 64] [--items 10000000] [--generic-items 1000000] [--reps 5]

One JSON line per measurement; every aim is reported as met or missed, never asserted.  --items is outputs per stream
and call; it is rounded down to a multiple of 32 (gmsk_mod at sps 4 makes 32 outputs per byte).
  (1) frequency_modulator_fc FAST, --streams x --items floats in one work_device call, beside quadrature_demod_cf on the
      same number of items (legs: modulator, demodulator, modulator).  Aim: no longer than the demodulator -- the
      inverse block, the same 12 bytes per item.  The scan reads its input twice: the 16 bytes per item over 8 TB/s is
      reported too.
  (2) gmsk_mod(sps 4) and cpmmod_bc(GAUSSIAN, sps 4, L 4), engine 1, for the same output count, beside
      frequency_modulator_fc alone on ready-made frequency samples (legs: handle, modulator, handle) and beside their
      engine 0.  Aims: no longer than the modulator alone; at most half of engine 0.
  (3) frequency_modulator_fc GENERIC beside agc2_cc GENERIC, --streams x --generic-items: both one wavefront per stream;
      reported, not targeted."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import grhip_loader  # noqa: E402

g = grhip_loader.import_grhip()

ap = argparse.ArgumentParser()
ap.add_argument("--streams", type=int, default=64)
ap.add_argument("--items", type=int, default=10_000_000)
ap.add_argument("--generic-items", type=int, default=1_000_000)
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()

dev = torch.device("cuda", 0)
st = torch.cuda.Stream(device=dev)
gen = torch.Generator(device=dev)
gen.manual_seed(1234)
S, n = args.streams, args.items // 32 * 32


def timeit(fn, reps, ramp_s=0.3):
    """ms per call on the stream's clock (the calls do not wait)"""
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


def aba(a, b, reps):
    a1, bb, a2 = timeit(a, reps), timeit(b, reps), timeit(a, reps)
    mean = 0.5 * (a1 + a2)
    return mean, bb, [round(a1, 4), round(a2, 4)], abs(a1 - a2) / mean


def verdict(ok):
    return "met" if ok else "missed"


# ---- (1) ------------------------------------------------------------------------------------------------------------
d_f = torch.randn((S, n), device=dev, dtype=torch.float32, generator=gen)
d_c = torch.empty((S * n + 1,), device=dev, dtype=torch.complex64)
d_y = torch.empty((S * n,), device=dev, dtype=torch.float32)
fm = g.frequency_modulator_fc(0.37)
fm.set_mode(g.MODE_FAST)
fm.set_streams(S)
qd = g.quadrature_demod_cf(1.0)
torch.cuda.synchronize()
run_fm = lambda: fm.work_device(n, d_f, d_c, stream=st)           # noqa: E731
run_qd = lambda: qd.work_device(S * n, d_c, d_y, stream=st)       # noqa: E731
t_fm, t_qd, legs, spread = aba(run_fm, run_qd, args.reps)
print(json.dumps({"measure": "1_frequency_modulator_fc", "streams": S, "items": n, "tile": g.frequency_modulator_fc_tile(),
                  "modulator_ms": round(t_fm, 4), "modulator_legs_ms": legs, "spread": round(spread, 4), "quadrature_demod_ms": round(t_qd, 4),
                  "modulator_over_demod": round(t_fm / t_qd, 3), "aim_no_longer_than_the_demodulator": verdict(t_fm <= t_qd * (1 + spread)),
                  "modulator_frac_of_8TBps_at_16_bytes": round(16.0 * S * n / t_fm / 1e6 / 8000.0, 4),
                  "demod_frac_of_8TBps_at_12_bytes": round(12.0 * S * n / t_qd / 1e6 / 8000.0, 4)}), flush=True)
del d_y, qd

# ---- (2) ------------------------------------------------------------------------------------------------------------
handles = {"gmsk_mod": (lambda: g.gmsk_mod(4, 0.35), n // 32), "cpmmod_bc": (lambda: g.cpmmod_bc(g.CPM_GAUSSIAN, 0.5, 4, 4, 0.3), n // 4)}
for name, (make, n_in) in handles.items():
    d_in = torch.randint(0, 256, (S, n_in), device=dev, dtype=torch.uint8, generator=gen)
    if name == "cpmmod_bc":
        d_in = (d_in & 2) + 255                                     # symbols -1 / +1 as signed chars
    line = {"measure": "2_" + name, "streams": S, "outputs": n, "inputs": n_in}
    t = {}
    for engine in (1, 0):
        blk = make()
        blk.set_mode(g.MODE_FAST)
        blk.set_engine(engine)
        blk.set_streams(S)
        torch.cuda.synchronize()
        run = lambda blk=blk: blk.work_device(n_in, d_in, d_c, stream=st)          # noqa: E731
        if engine == 1:
            t[1], t_alone, legs, spread = aba(run, run_fm, args.reps)
            line.update({"engine1_ms": round(t[1], 4), "engine1_legs_ms": legs, "spread": round(spread, 4), "modulator_alone_ms": round(t_alone, 4)})
        else:
            t[0] = timeit(run, args.reps)
            line["engine0_ms"] = round(t[0], 4)
        del blk, run
        torch.cuda.empty_cache()
    line.update({"engine1_over_modulator": round(t[1] / t_alone, 3), "aim_no_longer_than_the_modulator_alone": verdict(t[1] <= t_alone * (1 + spread)),
                 "engine1_over_engine0": round(t[1] / t[0], 3), "aim_at_most_half_of_engine0": verdict(t[1] <= 0.5 * t[0]),
                 "engine1_frac_of_8TBps": round((S * n_in + 8.0 * S * n) / t[1] / 1e6 / 8000.0, 4)})
    print(json.dumps(line), flush=True)
    del d_in
del d_f, d_c, fm
torch.cuda.empty_cache()

# ---- (3) ------------------------------------------------------------------------------------------------------------
m = args.generic_items
d_f = torch.randn((S, m), device=dev, dtype=torch.float32, generator=gen)
d_c = torch.empty((S, m), device=dev, dtype=torch.complex64)
d_x = torch.view_as_complex(torch.randn((S, m, 2), device=dev, dtype=torch.float32, generator=gen))
d_a = torch.empty_like(d_x)
fm = g.frequency_modulator_fc(0.37)
agc = g.agc2_cc(1e-2, 1e-3, 1, 1, 1000)
for b in (fm, agc):
    b.set_mode(g.MODE_GENERIC)
    b.set_streams(S)
torch.cuda.synchronize()
t_fm, t_agc, legs, spread = aba(lambda: fm.work_device(m, d_f, d_c, stream=st), lambda: agc.work_device(m, d_x, d_a, stream=st), max(2, args.reps // 2))
print(json.dumps({"measure": "3_generic", "streams": S, "items": m, "modulator_ms": round(t_fm, 4), "modulator_legs_ms": legs, "spread": round(spread, 4),
                  "agc2_cc_ms": round(t_agc, 4), "modulator_ns_per_item_and_stream": round(t_fm * 1e6 / m, 2),
                  "agc2_ns_per_item_and_stream": round(t_agc * 1e6 / m, 2)}), flush=True)
