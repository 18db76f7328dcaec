#!/usr/bin/env python3
"""bench.py -- headline benchmark of the MI355X-native DMR demodulation hot path.

Metric (BASELINE.json): Msamples/s of complex input through the FIR->demod chain
@256 taps, with the fraction of the HBM roofline, at 1/2/4/8 GPUs.

Workload (config.workload = BASELINE.json configs[1]):
  freq_xlating_fir_filter_ccc (256 taps, decim 4) -> quadrature_demod_cf on
  synthetic 10 MS/s 4FSK IQ captures of 10 M samples each.  One "step" = one
  pass of the fused hot-path kernel over a batch of `--captures` independent
  captures that are already resident in HBM; every capture starts from fresh
  block state (rotator phase 1, demod history 0), exactly like a fresh
  flowgraph per capture.

Multi-GPU: one process per GPU (torch.distributed, backend nccl == RCCL).  The
streams are independent units, so ranks shard captures with no data-path
collective ("scaling": "weak": per-GPU work is fixed); the only collective is
the RCCL broadcast of the shared taps from rank 0 at set-up.

A plain run sets up, ramps the clock, warms up, times --steps steps, writes
their outputs if --dump-outputs is given, and prints the line.  --full adds the
other engines on the same step, the CPU baselines and the full-chain batch.

Prints ONE JSON line on rank 0.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
import grhip_loader  # noqa: E402

HBM_PEAK_GBS = 8000.0          # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
FP32_VALU_PEAK_TFLOPS = 157.3  # spec, vector fp32
DUMP_MAX_BYTES = 60 * 10**6    # --dump-outputs: payload bound (the files stay under 64 MB)
DUMP_SEED = 0x444D5200


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--captures", type=int, default=64, help="captures per GPU per step")
    ap.add_argument("--ramp-ms", type=float, default=400.0,
                    help="untimed launches before the W warm-up steps until this much GPU time has passed: the "
                         "shader clock of an idle MI355X takes tens of ms of load to reach its steady state "
                         "(the same step measures 0.72 ms in the first 10 ms and 0.59 ms later)")
    ap.add_argument("--samples", type=int, default=10_000_000, help="complex samples per capture")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline does not need: the same step on the vector-FMA, reference-tap and "
                         "bit-exact engines, the CPU baselines and the full-chain batch (the last two trimmed by "
                         "--no-cpu-baseline / --chain-captures)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps, write what the last of them computed (rank 0) as DIR/<name>.npy: "
                         "demod_out.npy, float32, the demodulator output of every capture (captures x outputs), or a "
                         "fixed seeded sample of its columns (and rows) when the whole would exceed %d MB"
                         % (DUMP_MAX_BYTES // 10**6))
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--per-capture-launch", action="store_true",
                    help="one work_device() call per capture (block API) instead of one batched launch")
    ap.add_argument("--cpu-samples", type=int, default=10_000_000)
    ap.add_argument("--engine", choices=["fast", "fast_valu"], default="fast",
                    help="fast: GRHIP_MODE_FAST (matrix-core FIR engine); fast_valu: f32 vector FMAs only")
    ap.add_argument("--chain-captures", type=int, default=2048,
                    help="captures of the full-chain (configs[3]) measurement that --full adds to the line at N=1 (0: skip); "
                         "reduced automatically to what fits the device")
    ap.add_argument("--launcher-selftest", action="store_true",
                    help="CPU-only self-test of the N-rank launch path (gloo, a stub step that touches no GPU): "
                         "used by tests/test_bench_launcher.py; the line it prints is labelled as a stub")
    return ap.parse_args()


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def launch_ranks(a):
    """`python bench.py --gpus N` without a launcher around it: start N copies of this
    script, one rank per GPU, as CHILD processes (never os.exec*), before this process has
    imported torch or touched HIP.  Rank 0's JSON line is forwarded; any child failing
    fails the run."""
    import subprocess
    port = os.environ.get("MASTER_PORT") or str(_free_port())
    procs = []
    for r in range(a.gpus):
        env = dict(os.environ)
        env.update({"RANK": str(r), "LOCAL_RANK": str(r), "WORLD_SIZE": str(a.gpus),
                    "LOCAL_WORLD_SIZE": str(a.gpus), "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": port})
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL))
    # Poll every child: as soon as one exits non-zero the others are ended (terminate, then kill after a grace period)
    # -- a rank that dies before or during the rendezvous would otherwise leave its siblings waiting in
    # init_process_group / the broadcast until the distributed timeout.  Rank 0's stdout is read by a thread so that a
    # full pipe can never block it.
    import threading
    chunks = []
    rd = threading.Thread(target=lambda: chunks.append(procs[0].stdout.read()), daemon=True)
    rd.start()
    codes = [None] * a.gpus
    failed = False
    while any(c is None for c in codes):
        for r, p in enumerate(procs):
            if codes[r] is None:
                codes[r] = p.poll()
        if not failed and any(c not in (None, 0) for c in codes):
            failed = True
            for r, p in enumerate(procs):
                if codes[r] is None:
                    p.terminate()
            deadline = time.time() + 10.0
            while time.time() < deadline and any(p.poll() is None for p in procs):
                time.sleep(0.05)
            for p in procs:
                if p.poll() is None:
                    p.kill()
        time.sleep(0.02)
    rd.join(timeout=5.0)
    sys.stdout.write(b"".join(c for c in chunks if c).decode())
    sys.stdout.flush()
    bad = [(r, c) for r, c in enumerate(codes) if c != 0]
    if bad:
        raise SystemExit("bench.py: rank(s) failed: %s" % bad)


def launcher_selftest(a):
    """world_size ranks on gloo, a stub step (no GPU, no kernel): exercises exactly the
    launch / rendezvous / sharding / max-over-ranks / rank-0-prints path of the real run."""
    import torch
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if os.environ.get("GRHIP_SELFTEST_FAIL_RANK") == str(rank):      # tests: this rank dies before the rendezvous
        raise SystemExit(7)
    os.environ["GRHIP_NO_TORCH_PRELOAD"] = "1"
    if world > 1:
        dist.init_process_group(backend="gloo", rank=rank, world_size=world)
    g = grhip_loader.import_grhip()
    from grhip import dist as gd
    proto = gd.broadcast_taps(g.workload.cfg2_proto_taps() if rank == 0 else np.zeros(1, np.complex64), dist)
    mine = gd.shard_streams(world * a.captures, rank, world)
    t0 = time.perf_counter()
    for _ in range(a.steps):
        time.sleep(0.001 * (1 + rank))
    elapsed = gd.max_over_ranks(time.perf_counter() - t0, dist)
    seen = [None] * world
    if world > 1:
        dist.all_gather_object(seen, (rank, int(os.environ.get("LOCAL_RANK", "-1")), mine, os.getpid(), len(proto)))
    else:
        seen = [(rank, 0, mine, os.getpid(), len(proto))]
    if rank == 0:
        print(json.dumps({"metric": "STUB launcher self-test (gloo, no GPU work; not a measurement)",
                          "value": 0.0, "unit": "Msamples/s", "n_gpus": world, "steps": a.steps,
                          "warmup": a.warmup, "ms_per_step": elapsed / max(a.steps, 1) * 1e3,
                          "ranks": seen}), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def synth_captures(torch, wl, n_caps, n_samples, first_stream_id, device):
    """4FSK captures synthesised on the device with torch (workload generation is
    not on the measured path).  Same modulation as workload.fsk4_capture.
    Deterministic: the same arguments give the same bits on every run.  A
    floating-point torch.cumsum on the device is not (its scan may add in a
    different order each time), so the phase is the exact int64 running sum of
    the instantaneous frequencies, which are whole numbers of Hz, scaled once."""
    c = wl.CFG2
    sps = int(round(c["fs"] / c["sym_rate"]))
    n_syms = (n_samples + sps - 1) // sps + 1
    out = torch.empty((n_caps, n_samples, 2), dtype=torch.float32, device=device)
    n0 = sps / (10.0 ** (c["esn0_db"] / 10.0))
    sigma = math.sqrt(n0 / 2.0)
    for k in range(n_caps):
        sid = first_stream_id + k
        f_sym = c["carrier"] + c["deviation"] * wl.fsk4_symbols(n_syms, wl.SEED_BASE + sid)
        if not np.array_equal(f_sym, np.round(f_sym)):
            raise ValueError("synth_captures: the 4FSK frequencies must be whole numbers of Hz")
        f_inst = torch.from_numpy(f_sym.astype(np.int64)).to(device).repeat_interleave(sps)[:n_samples]
        ph = torch.cumsum(f_inst, 0).double() * (2 * math.pi / c["fs"])
        ph = torch.remainder(ph, 2 * math.pi)
        gen = torch.Generator(device=device)
        gen.manual_seed(wl.SEED_BASE + sid)
        noise = torch.randn((n_samples, 2), generator=gen, device=device, dtype=torch.float32) * sigma
        out[k, :, 0] = torch.cos(ph).float() + noise[:, 0]
        out[k, :, 1] = torch.sin(ph).float() + noise[:, 1]
        del ph, f_inst, noise
    return out


def cpu_baseline(wl, x_host, proto, repeats=2):
    """CPU path on the host cores of this box, rank 0 only.  Prefers the
    reference's own SSE dot-product + rotator + atan code (oracle/_ref, kind
    "reference"); falls back to this repo's generic-order port (kind "port")."""
    po = grhip_loader.import_oracle()
    c = wl.CFG2
    lib = "ref" if po.have_ref() else "oracle"
    best = None
    for _ in range(repeats):
        t0 = time.perf_counter()
        po.chain_xlating_demod(c["decim"], proto, c["center_freq"], c["fs"], c["demod_gain"], x_host, lib=lib)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    res = {
        "value": len(x_host) / best / 1e6, "unit": "Msamples/s", "cores": 1,
        "kind": "reference" if lib == "ref" else "port",
        "sample": "%d-sample capture, best of %d, single thread; %s" % (
            len(x_host), repeats,
            "reference ccomplex_dotprod_sse64.S + gr_rotator.h + gr_fast_atan2f.cc (oracle/_ref)"
            if lib == "ref" else "generic-order C port (oracle/liboracle.so)"),
    }
    # all host cores, one independent stream per thread (ctypes releases the GIL)
    try:
        import threading
        ncpu = os.cpu_count() or 1
        sub = x_host[: max(len(x_host) // 4, 1_000_000)]
        t0 = time.perf_counter()
        ths = [threading.Thread(target=po.chain_xlating_demod,
                                args=(c["decim"], proto, c["center_freq"], c["fs"], c["demod_gain"], sub),
                                kwargs={"lib": lib}) for _ in range(ncpu)]
        [t.start() for t in ths]
        [t.join() for t in ths]
        dt = time.perf_counter() - t0
        res["all_cores"] = {"value": ncpu * len(sub) / dt / 1e6, "cores": ncpu,
                            "sample": "%d streams x %d samples" % (ncpu, len(sub))}
    except Exception as e:  # pragma: no cover
        res["all_cores"] = {"error": str(e)}
    try:
        res["chain"] = cpu_chain_baseline(wl, x_host, proto, lib)
    except Exception as e:  # pragma: no cover
        res["chain"] = {"error": str(e)}
    return res


def cpu_chain_baseline(wl, x_host, proto, lib):
    """SURVEY 8(d) CPU legs for the full chain (config 4): xlating FIR + demodulator -> M&M clock recovery -> slicer ->
    access-code correlator on this box's host cores.  (i) one thread, stage after stage; (ii) one thread per block over
    64 k-item chunks, the shape of the reference's thread-per-block scheduler (gr_scheduler_tpb.cc:70-77: the slowest
    block sets the rate); (iii) one independent capture per host thread.  Stages are the oracle's C (the reference's
    SSE dot product where oracle/_ref is built, leg (i) and (iii) only -- the chunked leg needs the stateful port)."""
    import queue
    import threading
    po = grhip_loader.import_oracle()
    c, c4 = wl.CFG2, wl.CFG4
    code = wl.access_code_string()
    x = x_host[: min(len(x_host), 2_000_000)]

    def serial(xs, which):
        d = po.chain_xlating_demod(c["decim"], proto, c["center_freq"], c["fs"], c["demod_gain"], xs, lib=which)
        sym, _ = po.chain_mm(c4["omega"], c4["gain_omega"], c4["mu"], c4["gain_mu"], c4["omega_relative_limit"], d)
        return po.CorrelateAccessCode(code, c4["threshold"]).work(po.binary_slicer_fb(sym))

    t0 = time.perf_counter()
    flags = serial(x, lib)
    t_serial = time.perf_counter() - t0
    out = {"unit": "Msamples/s of complex input",
           "serial_1_thread": {"value": len(x) / t_serial / 1e6, "cores": 1, "kind": "reference" if lib == "ref" else "port",
                               "sync_flags": int((flags >> 1).sum()), "sample": "%d samples" % len(x)}}

    # (ii) thread per block
    D, nt = c["decim"], len(proto)
    CH = 65536                                   # output items of the FIR per chunk
    xin = wl.with_history(x, nt - 1)
    nout = len(x) // D
    q1, q2, q3, q4 = (queue.Queue(maxsize=4) for _ in range(4))

    def t_fir():
        f = po.Xlating(D, proto, c["center_freq"], c["fs"])
        for pos in range(0, nout, CH):
            m = min(CH, nout - pos)
            q1.put(f.work(xin[pos * D: pos * D + (m - 1) * D + nt], m))
        q1.put(None)

    def t_demod():
        last = np.zeros(1, np.complex64)
        while True:
            y = q1.get()
            if y is None:
                break
            yh = np.concatenate([last, y])
            q2.put(po.quad_demod_cf(c["demod_gain"], yh, len(y)))
            last = y[-1:]
        q2.put(None)

    def t_mm():
        mm = po.ClockRecoveryMM(c4["omega"], c4["gain_omega"], c4["mu"], c4["gain_mu"], c4["omega_relative_limit"])
        left = np.zeros(0, np.float32)
        while True:
            d = q2.get()
            if d is None:
                break
            buf = np.concatenate([left, d])
            o_, used = mm.general_work(len(buf), buf)
            left = buf[used:]
            q3.put(o_)
        q3.put(None)

    def t_slice():
        while True:
            s_ = q3.get()
            if s_ is None:
                break
            q4.put(po.binary_slicer_fb(s_))
        q4.put(None)

    nflags = [0]

    def t_corr():
        corr = po.CorrelateAccessCode(code, c4["threshold"])
        while True:
            b = q4.get()
            if b is None:
                break
            nflags[0] += int((corr.work(b) >> 1).sum())

    ths = [threading.Thread(target=f) for f in (t_fir, t_demod, t_mm, t_slice, t_corr)]
    t0 = time.perf_counter()
    [t.start() for t in ths]
    [t.join() for t in ths]
    t_tpb = time.perf_counter() - t0
    out["thread_per_block"] = {"value": len(x) / t_tpb / 1e6, "cores": len(ths), "kind": "port",
                               "sync_flags": nflags[0], "sample": "%d samples in %d-item chunks, 5 block threads" % (len(x), CH)}

    # (iii) one capture per host thread
    ncpu = os.cpu_count() or 1
    sub = x[: 1_000_000]
    ths = [threading.Thread(target=serial, args=(sub, lib)) for _ in range(ncpu)]
    t0 = time.perf_counter()
    [t.start() for t in ths]
    [t.join() for t in ths]
    dt = time.perf_counter() - t0
    out["all_cores"] = {"value": ncpu * len(sub) / dt / 1e6, "cores": ncpu, "kind": "reference" if lib == "ref" else "port",
                        "sample": "%d captures x %d samples" % (ncpu, len(sub))}
    return out


def chain_bench(torch, g, wl, dev, proto, n, want_caps, reps=3):
    """BASELINE configs[3] / north_star's target shape, driver-visible: the full DMR chain (xlating FIR -> quad demod ->
    clock_recovery_mm_ff -> slicer -> correlate_access_code, and the 4FSK tail pager_slicer_fb -> unpack_k_bits(2) ->
    correlator) over a batch of DISTINCT captures (one stream id each, synthesised like the headline's), resident in
    HBM.  Checked: three captures (first, middle, last) go through the CPU oracle chain -- same symbol count, same number
    of access-code flags, bit decisions equal but for the few symbols FAST mode may flip (the chain's own parity tests
    allow 8 per 70 k symbols); the access-code flags of the WHOLE batch are counted on the device against the sync words
    the generator planted."""
    c, c4 = wl.CFG2, wl.CFG4
    free_b, _total = torch.cuda.mem_get_info(dev)
    nout = n // c["decim"]
    per_cap = n * 8 + nout * (4 + 4 + 1 + 2 + 1 + 2) + 4096       # input, demod, soft, bits, 4FSK symbols / dibits / bits
    S = int(min(want_caps, (free_b - (6 << 30)) // per_cap))
    if S < 1:
        return {"skipped": "not enough device memory for one capture"}
    t0 = time.perf_counter()
    d_in = torch.empty((S, n, 2), dtype=torch.float32, device=dev)
    first_id = 1000                                               # stream ids 1000 ... 1000 + S - 1
    CH = 64
    for k0 in range(0, S, CH):
        kk = min(CH, S - k0)
        d_in[k0:k0 + kk] = synth_captures(torch, wl, kk, n, first_id + k0, dev)
    torch.cuda.synchronize()
    t_synth = time.perf_counter() - t0
    ch = g.dmr_chain(c["decim"], proto, c["center_freq"], c["fs"], c["demod_gain"], c4["omega"], c4["gain_omega"],
                     c4["mu"], c4["gain_mu"], c4["omega_relative_limit"], wl.access_code_string(), c4["threshold"], S, n)
    st = torch.cuda.Stream(device=dev)
    d_n = torch.zeros(S, dtype=torch.int32, device=dev)
    out = {"workload": "full DMR chain: freq_xlating_fir_filter_ccc 256-tap decim 4 -> quadrature_demod_cf -> "
                       "clock_recovery_mm_ff -> binary_slicer_fb -> correlate_access_code_bb, 10 M-sample captures",
           "captures": S, "distinct_stream_ids": S, "samples_per_capture": n, "synthesis_s": t_synth,
           "algorithmic_bytes_per_sample": 8.0 + 1.0 / (c["decim"] * c4["omega"])}

    def timed(bits, stride):
        for _ in range(2):
            ch.run_device(d_in, n, n, bits, stride, d_n, st)
        st.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(reps):
            ch.run_device(d_in, n, n, bits, stride, d_n, st)
        e1.record(st)
        st.synchronize()
        ms = e0.elapsed_time(e1) / reps
        rate = S * n / ms / 1e3
        return {"ms_per_batch": ms, "Msamples_per_s": rate,
                "frac": out["algorithmic_bytes_per_sample"] * rate * 1e6 / 1e9 / HBM_PEAK_GBS}

    d_bits = torch.zeros((S, nout), dtype=torch.uint8, device=dev)
    out["binary"] = timed(d_bits, nout)
    # ---- check ----
    nb = d_n.cpu().numpy()
    flags_dev = sum(int(torch.count_nonzero(d_bits[r0:r0 + 64] & 2).item()) for r0 in range(0, d_bits.shape[0], 64))
    n_syms_nominal = nout / c4["omega"]
    planted = len(range(100, int(n_syms_nominal) - 48, c4["sync_period_syms"]))
    chk = {"access_code_flags_on_device": flags_dev, "sync_words_planted": planted * S,
           "symbols_min_max": [int(nb.min()), int(nb.max())]}
    try:
        po = grhip_loader.import_oracle()
        lib = "ref" if po.have_ref() else "oracle"
        worst_flips, caps_checked = 0, []
        for k in sorted({0, S // 2, S - 1}):
            xh = d_in[k].cpu().numpy().reshape(-1).view(np.complex64)
            dem = po.chain_xlating_demod(c["decim"], proto, c["center_freq"], c["fs"], c["demod_gain"], xh, lib=lib)
            sym, _ = po.chain_mm(c4["omega"], c4["gain_omega"], c4["mu"], c4["gain_mu"], c4["omega_relative_limit"], dem)
            ref = po.CorrelateAccessCode(wl.access_code_string(), c4["threshold"]).work(po.binary_slicer_fb(sym))
            got = d_bits[k, :int(nb[k])].cpu().numpy()
            same_len = int(nb[k]) == len(ref)
            flips = int(np.count_nonzero((got ^ ref[:len(got)]) & 1)) if same_len else -1
            flags_ok = same_len and int((got >> 1).sum()) == int((ref >> 1).sum())
            caps_checked.append({"stream_id": first_id + k, "symbols": int(nb[k]), "symbols_oracle": len(ref),
                                 "bit_flips_vs_oracle": flips, "access_code_flags_equal": bool(flags_ok)})
            worst_flips = max(worst_flips, flips if flips >= 0 else 1 << 30)
        chk["captures_through_the_cpu_oracle"] = caps_checked
        chk["oracle_kind"] = "reference SSE dot product + rotator + atan (oracle/_ref)" if lib == "ref" else "generic-order port"
        chk["ok"] = bool(all(cc["symbols"] == cc["symbols_oracle"] and cc["access_code_flags_equal"] for cc in caps_checked)
                         and worst_flips <= 32 and abs(flags_dev - planted * S) <= 2 * S)
    except Exception as e:  # pragma: no cover
        chk["error"] = str(e)
        chk["ok"] = False
    out["check"] = chk
    del d_bits
    # ---- 4FSK tail ----
    ch.set_four_level(True, 0.001)
    d_bits2 = torch.zeros((S, 2 * nout), dtype=torch.uint8, device=dev)
    out["four_level"] = timed(d_bits2, 2 * nout)
    out["four_level"]["tail"] = "pager_slicer_fb(alpha 0.001) -> unpack_k_bits_bb(2) -> correlate_access_code_bb, two items per symbol"
    del ch, d_bits2, d_in
    torch.cuda.synchronize()
    return out


def measured_traffic(kernel, captures, samples, launches_per_step):
    """HBM bytes per launch of the dominant kernel from the committed rocprofv3 PMC
    passes (profiles/traffic.json: FETCH_SIZE doubled per the gfx950 correction for
    16-byte coalesced streaming reads, + WRITE_SIZE).  PMC counters cannot be read from
    inside this process, so the figure is a committed measurement: it is reported only when
    it was collected for this exact kernel and configuration (its provenance goes into
    `traffic_source`); otherwise null."""
    try:
        with open(os.path.join(ROOT, "profiles", "traffic.json")) as f:
            t = json.load(f)
        if (t.get("kernel") == kernel and t["captures"] == captures and t["samples"] == samples
                and launches_per_step == 1):
            return t["hbm_bytes_per_launch"], "profiles/traffic.json (%s)" % t.get("collected", "?")
    except Exception:
        pass
    return None, None


def dump_outputs(dirname, y):
    """--dump-outputs: the demodulator output of the last timed step, `y` (captures x outputs, float32, on the device),
    -> DIR/demod_out.npy.  Beyond DUMP_MAX_BYTES it is a fixed sample drawn with DUMP_SEED, so that the same arguments
    always pick the same elements: the same sorted columns of every capture (and sorted captures only if one column
    of each would not fit)."""
    import torch
    rows, cols = y.shape
    cap = DUMP_MAX_BYTES // y.element_size()
    rng = np.random.default_rng(DUMP_SEED)
    ri = np.arange(rows) if rows <= cap else np.sort(rng.choice(rows, cap, replace=False))
    kc = min(cols, cap // len(ri))
    ci = np.arange(cols) if kc == cols else np.sort(rng.choice(cols, kc, replace=False))
    if len(ri) < rows:
        y = y.index_select(0, torch.from_numpy(ri).to(y.device))
    if len(ci) < cols:
        y = y.index_select(1, torch.from_numpy(ci).to(y.device))
    os.makedirs(dirname, exist_ok=True)
    np.save(os.path.join(dirname, "demod_out.npy"), y.cpu().numpy().astype(np.float32, copy=False))


def main():
    a = parse()
    if a.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if a.steps < 1:
        raise SystemExit("--steps must be >= 1")
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # no torchrun around us: be the launcher (before torch / HIP are touched in this process)
        return launch_ranks(a)
    if "WORLD_SIZE" in os.environ and int(os.environ["WORLD_SIZE"]) != a.gpus:
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%s" % (a.gpus, os.environ["WORLD_SIZE"]))
    if a.launcher_selftest:
        return launcher_selftest(a)
    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the hot path has no CPU fallback")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend="nccl", device_id=dev)

    g = grhip_loader.import_grhip()
    wl = g.workload
    c = wl.CFG2

    from grhip import dist as gd
    # shared taps: built on rank 0 only, RCCL-broadcast over xGMI to the other ranks
    # (the only collective on this path; captures are independent units)
    proto = gd.broadcast_taps(wl.cfg2_proto_taps() if rank == 0 else np.zeros(1, np.complex64), dist, dev)
    my_streams = gd.shard_streams(world * a.captures, rank, world)     # weak scaling: B captures per rank

    n = a.samples
    B = a.captures
    hist = len(proto) - 1
    nout = n // c["decim"]
    # B captures resident in HBM, back to back rows (no history in front: the
    # kernel supplies the ntaps-1 zeros a fresh flowgraph preloads,
    # runtime/gr_flat_flowgraph.cc:150)
    row = ((n + 63) // 64) * 64
    buf = torch.zeros((B, row, 2), dtype=torch.float32, device=dev)
    caps = synth_captures(torch, wl, B, n, my_streams[0], dev)
    buf[:, :n, :] = caps
    want_cpu_baseline = a.full and world == 1 and not a.no_cpu_baseline
    x0_host = caps[0].cpu().numpy().reshape(-1).view(np.complex64).copy() if want_cpu_baseline else None
    del caps
    orow = ((nout + 63) // 64) * 64
    out = torch.empty((B, orow), dtype=torch.float32, device=dev)

    blk = g.xlating_demod(c["decim"], proto, c["center_freq"], c["fs"], c["demod_gain"], device=local_rank)
    blk.set_mode(g.MODE_FAST if a.engine == "fast" else g.MODE_FAST_VALU)
    # a real (non-null) stream: the kernels, and the events that time them, all go here
    stream = torch.cuda.Stream(device=dev)
    launches_per_step = 1 if not a.per_capture_launch else B

    def step():
        if a.per_capture_launch:
            hist_buf = step.hist_buf
            for b in range(B):
                blk.reset()
                blk.work_device(nout, hist_buf[b], out[b], stream)
        else:
            # one launch of the fused kernel over the whole batch of captures
            blk.run_captures_device(B, n, buf, row, out, orow, stream)

    if a.per_capture_launch:   # block-API form: history zeros materialised in front of each capture
        hrow = ((hist + n + 63) // 64) * 64
        step.hist_buf = torch.zeros((B, hrow, 2), dtype=torch.float32, device=dev)
        step.hist_buf[:, hist:hist + n, :] = buf[:, :n, :]

    torch.cuda.synchronize()
    # clock ramp (untimed, not counted as steps), then the W warm-up steps
    t_ramp = time.perf_counter()
    while (time.perf_counter() - t_ramp) * 1e3 < a.ramp_ms:
        step()
        stream.synchronize()
    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    ev0 = torch.cuda.Event(enable_timing=True)
    ev1 = torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    ev0.record(stream)
    for _ in range(a.steps):
        step()
    ev1.record(stream)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    dev_ms = ev0.elapsed_time(ev1)
    my_elapsed = elapsed
    elapsed = gd.max_over_ranks(elapsed, dist, dev)
    per_rank_ms = [my_elapsed / a.steps * 1e3]
    if world > 1:                                   # a straggler shows in the line (every rank's own clock)
        allr = [None] * world
        dist.all_gather_object(allr, my_elapsed / a.steps * 1e3)
        per_rank_ms = allr
    if a.dump_outputs and rank == 0:      # before anything else reuses `out`
        dump_outputs(a.dump_outputs, out[:, :nout])

    # --full: the same step on the vector-FMA engine (the north star's "no MFMA" form), reported beside the headline: a
    # few untimed steps for the clocks, then the same K steps under HIP events
    valu_ms = None
    reftaps_ms = None
    if a.full and a.engine == "fast" and not a.per_capture_launch:
        blk.set_mode(g.MODE_FAST_VALU)
        for _ in range(max(a.warmup, 3)):
            step()
        torch.cuda.synchronize()
        ev2 = torch.cuda.Event(enable_timing=True)
        ev3 = torch.cuda.Event(enable_timing=True)
        ev2.record(stream)
        for _ in range(a.steps):
            step()
        ev3.record(stream)
        torch.cuda.synchronize()
        valu_ms = ev2.elapsed_time(ev3) / a.steps
        # ... and on GRHIP_MODE_FAST_REFTAPS (the matrix-core engine + the reference's tap-angle quantisation)
        blk.set_mode(g.MODE_FAST_REFTAPS)
        for _ in range(max(a.warmup, 3)):
            step()
        torch.cuda.synchronize()
        ev4 = torch.cuda.Event(enable_timing=True)
        ev5 = torch.cuda.Event(enable_timing=True)
        ev4.record(stream)
        for _ in range(a.steps):
            step()
        ev5.record(stream)
        torch.cuda.synchronize()
        reftaps_ms = ev4.elapsed_time(ev5) / a.steps
        blk.set_mode(g.MODE_FAST)
    # ... and in the bit-exact mode (GRHIP_MODE_GENERIC: the reference's generic order, every operation unfused; the fused
    # generic-order kernel takes the batch in one launch like the fast engines)
    generic_ms = None
    if a.full and a.engine == "fast" and not a.per_capture_launch and rank == 0:
        blk.set_mode(g.MODE_GENERIC)
        for _ in range(2):
            step()
        torch.cuda.synchronize()
        ev6 = torch.cuda.Event(enable_timing=True)
        ev7 = torch.cuda.Event(enable_timing=True)
        gsteps = max(1, min(a.steps, 5))
        ev6.record(stream)
        for _ in range(gsteps):
            step()
        ev7.record(stream)
        torch.cuda.synchronize()
        generic_ms = ev6.elapsed_time(ev7) / gsteps
        blk.set_mode(g.MODE_FAST)

    if rank == 0:
        total_samples = float(world) * B * n * a.steps
        value = total_samples / elapsed / 1e6
        launches = launches_per_step * a.steps
        k_ms = dev_ms / launches                      # the only kernel in the timed region
        # 9 B per input sample (8 in + 4/decim out), fused; x samples per launch
        alg_bytes = (8.0 + 4.0 / c["decim"]) * n * (B / launches_per_step)
        achieved = alg_bytes / (k_ms * 1e-3) / 1e9
        flops = (2.0 * 2.0 * c["ntaps"] / c["decim"] + 8.0) * n * (B / launches_per_step)   # pre-mix + real-tap MACs
        if a.engine == "fast":
            kname = "fir_mfma_kernel<D=4,KS=10,premix,demod>"
            # matrix engine: 30 v_mfma_f32_16x16x32_f16 (16384 flop each) per 16 outputs x 8 segments = 512 input samples
            mfma_flops = 30 * 16384.0 / 512.0 * n * (B / launches_per_step)
        else:
            kname = "fir_tiled_kernel<D=4,premix,demod>"
            mfma_flops = 0.0
        traffic, traffic_src = measured_traffic(kname, B, n, launches_per_step)
        res = {
            "metric": "Msamples/s through FIR->demod chain @256 taps",
            "value": value, "unit": "Msamples/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": elapsed / a.steps * 1e3, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None,
            "dtype": ("f32 (FIR operands split into two binary16 halves on the matrix cores, f32 accumulation; demodulator f32)"
                      if a.engine == "fast" else "f32"),
            "data": "synthetic", "per_rank_ms_per_step": per_rank_ms,
            "config": {"workload": "freq_xlating_fir_filter_ccc 256-tap decim=4 + quadrature_demod_cf, "
                                   "10 MS/s synthetic 4FSK IQ", "captures_per_gpu_per_step": B,
                       "samples_per_capture": n, "sharding": "independent captures per rank, "
                       "RCCL broadcast of taps only", "clock_ramp_ms_untimed": a.ramp_ms,
                       "engine": "GRHIP_MODE_FAST (banded-Toeplitz FIR on the matrix cores, split binary16, f32 "
                                 "accumulation)" if a.engine == "fast" else "GRHIP_MODE_FAST_VALU (f32 vector FMAs)"},
            "roofline": {"bound": "hbm", "kernel": kname,
                         "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": traffic_src,
                         "kernel_ms": k_ms, "algorithmic_bytes_per_launch": alg_bytes,
                         "fir_equivalent_f32_tflops": flops / (k_ms * 1e-3) / 1e12,
                         "mfma_f16_tflops": mfma_flops / (k_ms * 1e-3) / 1e12,
                         "frac_of_f16_mfma_peak": mfma_flops / (k_ms * 1e-3) / 1e12 / 2500.0},
        }
        if valu_ms is not None:
            res["vector_engine"] = {"engine": "GRHIP_MODE_FAST_VALU (f32 vector FMAs, no matrix cores), same step, rank 0",
                                    "kernel": "fir_tiled_kernel<D=4,premix,demod>", "kernel_ms": valu_ms,
                                    "Msamples_per_s_per_gpu": B * n / valu_ms / 1e3,
                                    "frac": alg_bytes / (valu_ms * 1e-3) / 1e9 / HBM_PEAK_GBS}
        if reftaps_ms is not None:
            res["reference_taps_engine"] = {
                "engine": "GRHIP_MODE_FAST_REFTAPS (matrix-core engine + the reference's tap-angle quantisation: demodulator per "
                          "element 1.16e-5 against the reference's generic build, 8.9e-6 against its SSE build; FAST 1.80e-5), "
                          "same step, rank 0",
                "kernel": "fir_mfma_kernel<D=4,KS=10,premix,demod,tapq>", "kernel_ms": reftaps_ms,
                "Msamples_per_s_per_gpu": B * n / reftaps_ms / 1e3,
                "frac": alg_bytes / (reftaps_ms * 1e-3) / 1e9 / HBM_PEAK_GBS}
        if generic_ms is not None:
            res["bit_exact_engine"] = {
                "engine": "GRHIP_MODE_GENERIC (gr_fir_ccc_generic order, rotator and demodulator with the reference's operations: "
                          "bit-exact against the oracle), same step, rank 0",
                "kernel": "fir_generic_win_kernel<ccc,D=4,demod>", "kernel_ms": generic_ms,
                "Msamples_per_s_per_gpu": B * n / generic_ms / 1e3,
                "bound": "vector pipes: 256 unfused packed instructions per input sample"}
        if want_cpu_baseline:
            res["cpu_baseline"] = cpu_baseline(wl, x0_host[: a.cpu_samples], proto)
            res["gpu_over_cpu"] = value / res["cpu_baseline"]["value"]
        if a.full and world == 1 and a.chain_captures > 0 and not a.per_capture_launch:
            del buf, out
            torch.cuda.empty_cache()
            try:
                res["chain"] = chain_bench(torch, g, wl, dev, proto, n, a.chain_captures)
                cb = res.get("cpu_baseline", {}).get("chain", {}).get("serial_1_thread", {}).get("value")
                if cb and "binary" in res["chain"]:
                    res["chain"]["gpu_over_cpu_1_thread"] = res["chain"]["binary"]["Msamples_per_s"] / cb
            except Exception as e:  # pragma: no cover
                res["chain"] = {"error": str(e)}
        print(json.dumps(res), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
