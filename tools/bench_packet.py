"""The packet layer and the scramblers on one GPU, device resident, FAST mode, A-B-A in one run.

usage: python tools/bench_packet.py [--crc-mib 1024] [--streams 64] [--items 10000000] [--packets 65536] [--payload 1500] [--reps 10]

One JSON line per measurement; every aim is reported as met or missed, never asserted.
  (a) crc32_device over --crc-mib MiB beside torch's device-to-device copy of the same buffer (legs: CRC, copy, CRC).  The
      CRC call returns its value, so it waits for the stream: both legs are timed on the host around calls that wait.
      Aim: no slower than the copy -- the CRC reads every byte once and writes nothing.
  (b) scrambler_bb(0x8a, 0x7f, 7), --streams x --items bytes in one work_device call, beside diff_encoder_bb(2) on the same
      items (legs: scrambler, encoder, scrambler); descrambler_bb and additive_scrambler_bb are timed alongside.  Aim: at
      most the encoder's time -- the passes are the same, the state a word instead of a byte.
  (c) packet_maker and packet_check for --packets packets of --payload bytes: the bytes read and written over 8 TB/s."""
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
ap.add_argument("--crc-mib", type=int, default=1024)
ap.add_argument("--streams", type=int, default=64)
ap.add_argument("--items", type=int, default=10_000_000)
ap.add_argument("--packets", type=int, default=65536)
ap.add_argument("--payload", type=int, default=1500)
ap.add_argument("--reps", type=int, default=10)
args = ap.parse_args()

dev = torch.device("cuda", 0)
st = torch.cuda.Stream(device=dev)
gen = torch.Generator(device=dev)
gen.manual_seed(1234)


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


def timeit_host(fn, reps, ramp_s=0.3):
    """ms per call on the host's clock, for calls that wait for their result"""
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < ramp_s:
        fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) * 1e3 / reps


def aba(a, b, timer, reps):
    a1, bb, a2 = timer(a, reps), timer(b, reps), timer(a, reps)
    mean = 0.5 * (a1 + a2)
    return mean, bb, [round(a1, 4), round(a2, 4)], abs(a1 - a2) / mean


# ---- (a) ------------------------------------------------------------------------------------------------------------
nbytes = args.crc_mib << 20
d_a = torch.randint(0, 256, (nbytes,), device=dev, dtype=torch.uint8, generator=gen)
d_b = torch.empty_like(d_a)
crc = g.crc32()


def copy():
    with torch.cuda.stream(st):
        d_b.copy_(d_a)
    st.synchronize()


t_crc, t_copy, legs, spread = aba(lambda: crc.crc32_device(d_a, nbytes, stream=st), copy, timeit_host, args.reps)
print(json.dumps({"measure": "a_crc32", "bytes": nbytes, "crc_ms": round(t_crc, 4), "crc_legs_ms": legs, "spread": round(spread, 4),
                  "copy_ms": round(t_copy, 4), "crc_GBps": round(nbytes / t_crc / 1e6, 1), "copy_GBps_read_plus_write": round(2 * nbytes / t_copy / 1e6, 1),
                  "crc_over_copy": round(t_crc / t_copy, 3), "aim_no_slower_than_the_copy": "met" if t_crc <= t_copy * (1 + spread) else "missed"}),
      flush=True)
del d_a, d_b
torch.cuda.empty_cache()

# ---- (b) ------------------------------------------------------------------------------------------------------------
S, n = args.streams, args.items
d_in = torch.randint(0, 2, (S, n), device=dev, dtype=torch.uint8, generator=gen)
d_out = torch.empty_like(d_in)
blocks = {"scrambler_bb": g.scrambler_bb(0x8a, 0x7f, 7), "descrambler_bb": g.descrambler_bb(0x8a, 0x7f, 7),
          "additive_scrambler_bb": g.additive_scrambler_bb(0x8a, 0x7f, 7, 0), "diff_encoder_bb": g.diff_encoder_bb(2)}
for b in blocks.values():
    b.set_mode(g.MODE_FAST)
    b.set_streams(S)
torch.cuda.synchronize()
run = {k: (lambda b=b: b.work_device(n, d_in, d_out, stream=st)) for k, b in blocks.items()}
t_s, t_e, legs, spread = aba(run["scrambler_bb"], run["diff_encoder_bb"], timeit, args.reps)
line = {"measure": "b_scrambler", "streams": S, "items": n, "scrambler_ms": round(t_s, 4), "scrambler_legs_ms": legs, "spread": round(spread, 4),
        "diff_encoder_ms": round(t_e, 4), "scrambler_over_encoder": round(t_s / t_e, 3),
        "aim_at_most_the_encoders_time": "met" if t_s <= t_e * (1 + spread) else "missed",
        "scrambler_GBps_in_plus_out": round(2.0 * S * n / t_s / 1e6, 1)}
for k in ("descrambler_bb", "additive_scrambler_bb"):
    line[k + "_ms"] = round(timeit(run[k], args.reps), 4)
print(json.dumps(line), flush=True)
del d_in, d_out, blocks, run
torch.cuda.empty_cache()

# ---- (c) ------------------------------------------------------------------------------------------------------------
P, L = args.packets, args.payload
mk = g.packet_maker(2, 1)
jobs, tin, tout = mk.plan([L] * P, [i % 16 for i in range(P)])
d_jobs = torch.from_numpy(jobs.view(np.uint32).reshape(-1).copy().view(np.int32)).to(dev)
d_pay = torch.randint(0, 256, (tin,), device=dev, dtype=torch.uint8, generator=gen)
d_pkt = torch.empty(tout, device=dev, dtype=torch.uint8)
t_make = timeit(lambda: mk.work_device(P, d_jobs, d_pay, d_pkt, stream=st), args.reps)
# the messages as a framer leaves them: every packet's whitened payload + CRC, back to back in one stream's pool
size = mk.packet_bytes(L)
body = d_pkt.view(P, size)[:, 14:14 + L + 4].contiguous().view(-1)
recs = np.zeros(P, g.PACKET_REC)
recs["whitener_offset"] = np.arange(P) % 16
recs["length"] = L + 4
recs["offset"] = np.arange(P, dtype=np.int64) * (L + 4)
d_recs = torch.from_numpy(recs.view(np.uint32).reshape(-1).copy().view(np.int32)).to(dev)
d_plain = torch.empty_like(body)
d_ok = torch.zeros(P, device=dev, dtype=torch.uint8)
chk = g.packet_check()
t_check = timeit(lambda: chk.work_device(1, P, d_recs, P, None, 0, body, body.numel(), True, d_plain, d_ok, stream=st), args.reps)
all_ok = bool((d_ok == 1).all().item())
print(json.dumps({"measure": "c_packets", "packets": P, "payload": L, "packet_bytes": size, "maker_ms": round(t_make, 4),
                  "maker_frac_of_8TBps": round((tin + tout) / t_make / 1e6 / 8000.0, 4), "check_ms": round(t_check, 4),
                  "check_frac_of_8TBps": round(2.0 * body.numel() / t_check / 1e6 / 8000.0, 4), "every_packet_ok": all_ok}), flush=True)
