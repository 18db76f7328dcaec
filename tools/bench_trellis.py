"""trellis_viterbi_b on one GPU, device resident, A-B-A in one run.

usage: python tools/bench_trellis.py [--K 1024] [--rounds 2] [--reps 5] [--agc-items 1000000]

One JSON line per measurement; nothing is asserted.
  (1) Decode rate of trellis_viterbi_b for awgn1o2_4 (4 states, 16 blocks per wavefront), the 64-state (133, 171) code
      (one block per wavefront) and awgn1o2_128 (two wavefronts per block): blocks of --K steps, --rounds times the
      handle's resident_blocks(), so that every persistent wavefront walks --rounds blocks (groups of blocks) one after
      the other.  Legs: FAST, GENERIC, FAST.  Reported: trellis steps per second (steps x blocks over the time) and
      nanoseconds per step and wavefront (the time over the K x rounds steps a wavefront walks serially), for both modes.
  (2) trellis_viterbi_combined_fb(D = 1) on awgn1o2_4 and the 64-state code, the same shape: engine 1 (the metrics formed
      in the decoder's LDS window from the raw floats), engine 0 (metrics kernel into a scratch buffer, then the decoder),
      engine 1; beside trellis_viterbi_b on ready metrics from (1).  A step moves 4 bytes in engine 1 and writes and reads
      16 more in engine 0.
  (3) agc2_cc GENERIC on 64 streams, one wavefront per stream walking its items serially: nanoseconds per item and
      wavefront, the library's other serial float recurrence, measured in the same run for comparison."""
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
ap.add_argument("--K", type=int, default=1024)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--agc-items", type=int, default=1_000_000)
args = ap.parse_args()

dev = torch.device("cuda", 0)
st = torch.cuda.Stream(device=dev)
gen = torch.Generator(device=dev)
gen.manual_seed(1234)
FSM_DIR = os.path.join(ROOT, "tests", "golden", "fsm")


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


codes = (("awgn1o2_4", lambda: g.fsm(os.path.join(FSM_DIR, "awgn1o2_4.fsm"))),
         ("gen_133_171", lambda: g.fsm(1, 2, [0o133, 0o171])),
         ("awgn1o2_128", lambda: g.fsm(os.path.join(FSM_DIR, "awgn1o2_128.fsm"))))
K = args.K
viterbi_ms = {}
for name, make in codes:
    f = make()
    blk = g.trellis_viterbi_b(f, K, 0, -1)
    blocks = blk.resident_blocks() * args.rounds
    n = blocks * K
    # metrics of a noisy signal's kind: non-negative floats, no ties to speak of
    d_m = torch.rand((n * f.O(),), device=dev, dtype=torch.float32, generator=gen) * 4
    d_out = torch.empty((n,), device=dev, dtype=torch.uint8)
    torch.cuda.synchronize()

    def run(mode):
        blk.set_mode(mode)
        blk.work_device(n, d_m, d_out, stream=st)
    t_fast, t_gen, legs, spread = aba(lambda: run(g.MODE_FAST), lambda: run(g.MODE_GENERIC), args.reps)
    serial_steps = K * args.rounds
    print(json.dumps({"measure": "1_viterbi_b_" + name, "S": f.S(), "O": f.O(), "K": K, "blocks": blocks,
                      "blocks_per_wavefront": blk.blocks_per_wavefront(), "resident_blocks": blk.resident_blocks(),
                      "trace_window": blk.trace_window(), "workspace_bytes": blk.workspace_bytes(),
                      "fast_ms": round(t_fast, 4), "fast_legs_ms": legs, "spread": round(spread, 4), "generic_ms": round(t_gen, 4),
                      "fast_steps_per_s": round(n / t_fast * 1e3, 0), "generic_steps_per_s": round(n / t_gen * 1e3, 0),
                      "fast_ns_per_step_and_wavefront": round(t_fast * 1e6 / serial_steps, 2),
                      "generic_ns_per_step_and_wavefront": round(t_gen * 1e6 / serial_steps, 2),
                      "fast_input_GBps": round(4.0 * n * f.O() / t_fast / 1e6, 1)}), flush=True)
    viterbi_ms[name] = t_fast
    del blk, d_m, d_out
    torch.cuda.empty_cache()

for name, make in codes[:2]:
    f = make()
    table = torch.linspace(-1.5, 1.5, f.O()).numpy()
    blk = g.trellis_viterbi_combined_fb(f, K, 0, -1, 1, table, g.TRELLIS_EUCLIDEAN)
    blocks = blk.resident_blocks() * args.rounds
    n = blocks * K
    d_x = torch.randn((n,), device=dev, dtype=torch.float32, generator=gen)
    d_out = torch.empty((n,), device=dev, dtype=torch.uint8)
    torch.cuda.synchronize()

    def run_engine(engine):
        blk.set_engine(engine)
        blk.work_device(n, d_x, d_out, stream=st)
    t1, t0, legs, spread = aba(lambda: run_engine(1), lambda: run_engine(0), args.reps)
    print(json.dumps({"measure": "2_viterbi_combined_fb_" + name, "S": f.S(), "O": f.O(), "D": 1, "K": K, "blocks": blocks,
                      "engine1_ms": round(t1, 4), "engine1_legs_ms": legs, "spread": round(spread, 4), "engine0_ms": round(t0, 4),
                      "engine1_over_engine0": round(t1 / t0, 3), "viterbi_b_on_ready_metrics_ms": round(viterbi_ms[name], 4),
                      "engine1_over_viterbi_b": round(t1 / viterbi_ms[name], 3),
                      "engine1_steps_per_s": round(n / t1 * 1e3, 0)}), flush=True)
    del blk, d_x, d_out
    torch.cuda.empty_cache()

m = args.agc_items
S = 64
d_x = torch.view_as_complex(torch.randn((S, m, 2), device=dev, dtype=torch.float32, generator=gen))
d_a = torch.empty_like(d_x)
agc = g.agc2_cc(1e-2, 1e-3, 1, 1, 1000)
agc.set_mode(g.MODE_GENERIC)
agc.set_streams(S)
torch.cuda.synchronize()
t_agc = timeit(lambda: agc.work_device(m, d_x, d_a, stream=st), max(2, args.reps // 2))
print(json.dumps({"measure": "3_agc2_cc_generic", "streams": S, "items": m, "agc2_cc_ms": round(t_agc, 4),
                  "agc2_ns_per_item_and_wavefront": round(t_agc * 1e6 / m, 2)}), flush=True)
