#!/usr/bin/env python3
"""bench.py -- headline benchmark: Msamples/s demodulated by the fused HIP FSK demodulator.

One "step" = one pass of the hot path (fskhip_demodulate_device: AGC -> band-pass -> I/Q mix -> low-pass ->
discriminator -> slicer -> sync -> UART framing) over ONE batch of synthetic 48 kHz streams already resident in HBM.

Default workload = BASELINE.json's metric configuration, configs[2] as SURVEY.md section 8 defines it (C3):
65 536 Bell-202 1200-baud streams x 480 000 samples (10 s) per GPU = 126 GB resident.  Streams shard across GPUs with
no collective.

  python bench.py --gpus N --steps K --warmup W [--full] [--dump-outputs DIR]

A plain run does what the headline needs and no more: set-up, W warm-ups, K timed steps, one JSON line.  --full adds what
is measured or checked beyond it (the CPU baseline and its oracle check, the shader-clock probe, the strong-scaling pass,
the side measurements, the c5 quality score).  --dump-outputs DIR writes, after the timed steps, what the last of them
returned (rank 0) as DIR/<name>.npy in float32 / float64: for the demodulator every stream's byte and 'eod' counts and the
bytes of a fixed, seeded sample of streams; for --workload mod the signal of such a sample and every stream's output length.
With the same arguments the inputs are the same from run to run (seeded synthesis on the device).

N > 1 without a launcher (no WORLD_SIZE in the environment): this process starts its own N ranks -- BEFORE anything
touches the GPU -- as a child `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ...
bench.py <same arguments>`, relays rank 0's JSON line and exits with the child's code.  Under a launcher (the driver's
own torch.distributed.run) RANK / LOCAL_RANK / WORLD_SIZE come from the environment as usual.

With N > 1 and --full ONE line carries both shapes:
  value                    weak scaling: every rank holds its own --streams streams (65 536 per GPU)
  config.strong_scaling    BASELINE config #3 as written: --streams streams IN TOTAL, a contiguous block per rank
                           (sharding.stream_shard: 8 192 per GPU at 8), measured right after the weak pass
(--total-streams T measures only the strong shape of T streams and reports it as `value`, scaling "strong").

Prints ONE JSON line on rank 0 (driver contract) with the extra objects
  roofline      achieved algorithmic HBM GB/s of the demod kernel (4 B per input sample) from HIP events
                around every launch on the launch stream, against the 8 TB/s peak; `kernel` is what the library says it
                launched (fskhip_last_kernel).  `binding_bound` names the ceiling that actually binds and
                `valu_issue` is the same run against it: vector instructions issued per second (committed PMC
                instruction mix x this run's rate) against 1024 SIMDs x one wave64 instruction per 2 cycles at 2.4 GHz
  cpu_baseline  (--full; null otherwise) the CPU oracle (scalar fp64 C port of the reference, oracle/) timed on one host
                core on a bounded sample of the same buffers; doubles as a parity check of that sample (GPU bytes ==
                oracle bytes): a mismatch sets parity_ok false and the exit code of EVERY rank to 3
and, with --full at N = 1, side measurements in `config` (never the headline): the fp64 parity path on the same shape, a
large batch (262 144 streams), and the PCIe-inclusive rate through fskhip_demodulate_host.  Without --full the clock in
`roofline.valu_issue` is the part's maximum (the probe that measures it runs with --full).

--workload c5 is BASELINE config #5 as BASELINE.md defines it: every stream's frames come from fskhip_modulate_device
(FSKCore.modulateData), Gaussian noise at 10 dB with the reference tests' power definition (mean square over the whole
buffer incl. padding, fsk-demodulation.node.test.ts:1184-1205), and with --full besides the throughput the line carries
config.c5_quality: frame success rate, BER against the transmitted payloads, and the oracle comparison of a stream sample.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec (MI355X_MICROARCH.md: 8.0 TB/s spec, 6.29 TB/s measured copy)
SIMDS = 1024           # 256 CUs x 4 SIMD-32
CLOCK_GHZ = 2.4        # max clock (MI355X_MICROARCH.md); one wave64 vector instruction per 2 cycles per SIMD

WORKLOADS = {
    # BASELINE.json configs[2] (the one the metric is quoted on): Bell-202, 1200 baud
    "c3": dict(cfg=dict(baudRate=1200, markFrequency=1200, spaceFrequency=2200), payload=100, snr=None, num="3",
               desc="Bell-202 1200 baud (1200/2200 Hz) @48 kHz"),
    # BASELINE.json configs[1]: 300 baud V.21 tones in the polarity the reference decodes
    "c2": dict(cfg=dict(baudRate=300, markFrequency=1070, spaceFrequency=1270), payload=32, snr=None, num="2",
               desc="V.21 300 baud (1070/1270 Hz) @48 kHz"),
    # BASELINE.json configs[4]: FSKCore.modulate -> AWGN 10 dB -> demodulate (TX through fskhip_modulate_device)
    "c5": dict(cfg=dict(baudRate=1200, markFrequency=1200, spaceFrequency=2200), payload=100, snr=10.0, num="5",
               desc="Bell-202 1200 baud @48 kHz, modulateData frames + AWGN 10 dB", roundtrip=True),
    # BASELINE.json configs[3]: per-stream tone pairs (mark_s = 1000 + 10 (s mod 100), space_s = mark_s + 200), 300 baud
    "c4": dict(cfg=dict(baudRate=300, markFrequency=1000, spaceFrequency=1200), payload=16, snr=None, num="4",
               desc="300 baud, per-stream mark/space tone pairs @48 kHz", per_stream=True),
    "default": dict(cfg=dict(), payload=100, snr=None, num="-", desc="default 1650/1850 Hz 1200 baud @48 kHz"),
    # VERDICT r03 #3 -- what a receiver bank does most of its life.  idle: ONE frame per stream, then a Gaussian floor 30 dB
    # under it for the rest of the 10 s: after the frame every stream fires 'eod' each samplesForEOD decimated samples and
    # resets (fsk.ts:285-295), with independent timing per stream.
    "idle": dict(cfg=dict(baudRate=1200, markFrequency=1200, spaceFrequency=2200), payload=100, snr=None, num="3 (idle variant)",
                 desc="Bell-202 1200 baud @48 kHz, ONE frame per stream then a noise floor 30 dB under it", idle_db=30.0),
    # idle4 (round 5): the same idle regime with per-stream tone pairs (config #4's kind: per-lane NCO in the block path with resets)
    "idle4": dict(cfg=dict(baudRate=1200, markFrequency=1200, spaceFrequency=2200), payload=100, snr=None, num="4 (idle variant, 1200 baud)",
                  desc="1200 baud @48 kHz, per-stream tone pairs, ONE frame per stream then a noise floor 30 dB under it", idle_db=30.0,
                  per_stream=True, tones1200=True),
    # c1x: BASELINE config #1's tone pair as written (mark 1270 / space 1070: the polarity the reference does not decode) at
    # config #3's stream count: a bank that searches for a preamble all the time and never finds one (fsk.ts:297-328)
    "c1x": dict(cfg=dict(baudRate=300, markFrequency=1270, spaceFrequency=1070), payload=32, snr=None, num="1 (x 65 536)",
                desc="V.21 300 baud with config #1's polarity (mark 1270 / space 1070 Hz: never syncs) @48 kHz"),
}


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", default="c3", choices=sorted(WORKLOADS) + ["mod"],
                    help="mod = FSKCore.modulateData, BASELINE config #5's TX leg (16 384 streams x 11 frames of 100 bytes unless --streams / --seconds say otherwise)")
    ap.add_argument("--streams", type=int, default=65536, help="streams per GPU (weak scaling); with N > 1 also the TOTAL of the strong-scaling pass")
    ap.add_argument("--total-streams", type=int, default=0,
                    help="strong scaling only: this many streams in total, sharded over the ranks (0 = weak + strong in one line)")
    ap.add_argument("--seconds", type=float, default=10.0, help="audio seconds per stream per step")
    ap.add_argument("--precision", default="f32", choices=["f32", "f64"])
    ap.add_argument("--cpu-seconds", type=float, default=12.0, help="budget for the cpu_baseline leg of --full (0 = skip)")
    ap.add_argument("--no-side", action="store_true", help="with --full: skip the side measurements (fp64 path, large batch, PCIe)")
    ap.add_argument("--probe-reads", type=int, default=0,
                    help="also launch the read-pattern probe kernel this many times (FETCH_SIZE calibration)")
    ap.add_argument("--pitch-pad", type=int, default=0, help="extra floats of row pitch (experiments)")
    ap.add_argument("--snr-db", type=float, default=None, help="add AWGN at this SNR (overrides the workload's)")
    ap.add_argument("--lead-max", type=int, default=None,
                    help="every stream's first frame starts at a random offset below this many samples (default: ten bit cells, so "
                         "that the streams' frames -- and their resets -- nearly line up; a frame length = streams that do not)")
    ap.add_argument("--no-clock-probe", action="store_true",
                    help="with --full: skip the shader-clock probe and its extra steps (profiler passes: their kernel statistics then hold the timed launches only)")
    ap.add_argument("--opt", action="append", default=[], metavar="NAME=VALUE",
                    help="fskhip_set_option for every engine of this run (measurements: kernel=two-wave, blk_y_slots=12, ...)")
    ap.add_argument("--dry-engine", action="store_true",
                    help="launcher / aggregation test without a GPU: gloo backend and a stand-in engine that only sleeps "
                         "(tests/test_bench_launcher_cpu.py); the line says so in `data`")
    ap.add_argument("--full", action="store_true",
                    help="also everything beyond the headline: the CPU oracle baseline and its parity check of a sample, the "
                         "shader-clock probe, the strong-scaling pass (N > 1) and the side measurements (N = 1)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one returned (rank 0) as DIR/<name>.npy")
    return ap


def check_args(ap, args):
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    if args.dump_outputs and args.dry_engine:
        ap.error("--dump-outputs needs the real engine")


DUMP_ROWS_BUDGET = 32 << 20     # bytes of per-sample rows one --dump-outputs writes at most (64 MB in all with the rest)
DUMP_SEED = 0xD0E5


def dump_rows(n_rows, row_bytes):
    """the fixed sample of rows a dump holds when all of them would not fit: a function of the shape alone"""
    k = int(max(1, min(n_rows, DUMP_ROWS_BUDGET // max(1, row_bytes))))
    if k == n_rows:
        return list(range(n_rows))
    import numpy as np
    return sorted(np.random.RandomState(DUMP_SEED).choice(n_rows, k, replace=False).tolist())


def write_dump(dirname, arrays):
    """arrays: name -> float32 / float64 numpy array, written as dirname/<name>.npy"""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    for name, a in arrays.items():
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
        np.save(os.path.join(dirname, name + ".npy"), a)


# ---------------------------------------------------------------------------------------------------------------------
# N > 1 without a launcher: start the ranks ourselves (fresh child processes; this process never touches the GPU)
# ---------------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def self_launch(args, argv):
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env["MASTER_ADDR"] = "127.0.0.1"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + argv
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
    lines = [l for l in p.stdout.splitlines() if l.startswith("{") and '"metric"' in l]
    for l in p.stdout.splitlines():
        if l not in lines:
            print(l, file=sys.stderr)
    if lines:
        print(lines[-1])
    elif p.returncode == 0:
        print("bench.py: the ranks exited 0 without a JSON line", file=sys.stderr)
        return 4
    return p.returncode


# ---------------------------------------------------------------------------------------------------------------------
class DryEngine:
    """--dry-engine: the engine's surface as far as the timed loop uses it; a step sleeps in proportion to its streams."""

    def __init__(self, n_streams):
        self.n_streams, self._n, self._ms = n_streams, 0, 0.0

    def max_bytes(self, n):
        return n // 400 + 8

    def last_kernel(self):
        return "dry_engine"

    def blk_lanes(self):
        return 0

    def demodulate_device(self, *a, **k):
        dt = 1e-3 * (1 + self.n_streams / 65536.0)
        time.sleep(dt)
        self._n += 1
        self._ms += dt * 1e3

    def timing_begin(self):
        self._n, self._ms = 0, 0.0

    def timing_end(self):
        return self._n, self._ms

    def close(self):
        pass


def timed_steps(sync, eng, step, steps):
    """kernel-only time of `steps` calls: HIP events recorded by the library around every launch"""
    sync()
    eng.timing_begin()
    for _ in range(steps):
        step()
    sync()
    return eng.timing_end()


def measure(sync, dist, eng, step, steps, warmup, dev):
    """the contract's timed region: W warm-ups, then K steps between barrier + synchronize on both sides, MAX over ranks"""
    from webaudio_modem_amd.sharding import max_over_ranks
    for _ in range(warmup):
        step()
    sync()
    if dist is not None:
        dist.barrier()
    sync()
    eng.timing_begin()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    sync()
    if dist is not None:
        dist.barrier()
    sync()
    elapsed = time.perf_counter() - t0
    n_launch, kernel_ms = eng.timing_end()
    return max_over_ranks(elapsed, dist, dev), n_launch, kernel_ms


def c5_build_and_score(torch, np, wm, eng, cfg, x, N, pitch, snr, seed, payload_len, stream, oracle_seconds, first_stream, score):
    """BASELINE config #5: fill x with FSKCore.modulateData frames (fskhip_modulate_device), one per time slot, add AWGN
    with the reference tests' power definition; with `score` (--full), demodulate slot by slot (the engine is a streaming
    state machine: any cut of a stream gives the same bytes) so that every frame's bytes are attributed to it, and score
    them against the transmitted payloads; a strided sample of streams is demodulated by the CPU oracle with the same cuts."""
    S = x.shape[0]
    frame_len = eng.modulated_length(payload_len)
    slot = (frame_len + 1952 + 15) // 16 * 16           # frame + 1 952 samples of silence, whole 16-sample tiles
    F = max(1, N // slot)
    rng = np.random.RandomState((seed ^ 0xC5) & 0x7FFFFFFF)
    payloads = rng.randint(0, 256, size=(F, S, payload_len)).astype(np.uint8)
    x.zero_()
    d_lens = torch.full((S,), payload_len, dtype=torch.int32, device="cuda")
    d_olens = torch.empty(S, dtype=torch.int32, device="cuda")
    t0 = time.perf_counter()
    for f in range(F):
        d_pay = torch.as_tensor(payloads[f], device="cuda")
        eng.modulate_device(d_pay.data_ptr(), d_lens.data_ptr(), payload_len, x.data_ptr() + 4 * f * slot, pitch,
                            d_olens.data_ptr(), stream)
        torch.cuda.synchronize()
    t_mod = time.perf_counter() - t0
    eng.add_awgn_device(x.data_ptr(), N, pitch, snr, seed ^ 0xA36, stream)
    torch.cuda.synchronize()
    if not score:
        return None
    # ---- demodulate slot by slot
    eng.reset()
    op = eng.max_bytes(slot + N - F * slot)
    out = torch.zeros((S, op), dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(S, dtype=torch.int32, device="cuda")
    got, got_n = [], []
    for f in range(F):
        n_f = slot if f + 1 < F else N - f * slot
        eng.demodulate_device(x.data_ptr() + 4 * f * slot, n_f, pitch, out.data_ptr(), op, cnt.data_ptr(), 0, 0, stream)
        torch.cuda.synchronize()
        got.append(out.cpu().numpy().copy())
        got_n.append(cnt.cpu().numpy().astype(np.int64))
    eng.reset()
    frames = F * S
    ok = 0
    len_match = 0
    bit_err = 0
    delivered = 0
    for f in range(F):
        n_ok_len = got_n[f] == payload_len
        len_match += int(n_ok_len.sum())
        rx = got[f][:, :payload_len]
        diff = np.bitwise_xor(rx[n_ok_len], payloads[f][n_ok_len])
        errs = np.unpackbits(diff, axis=1).sum(axis=1)
        bit_err += int(errs.sum())
        ok += int((errs == 0).sum())
        # a slot with more (or fewer) bytes than the payload: noise in the gaps decoded as extra bytes (a false sync) or a
        # frame cut short -- the reference's own behaviour at this SNR; the payload may still have come through whole
        exact = np.zeros(S, bool)
        exact[np.nonzero(n_ok_len)[0][errs == 0]] = True
        delivered += int(exact.sum())
        for s in np.nonzero(~exact)[0]:
            delivered += payloads[f][s].tobytes() in got[f][s, :got_n[f][s]].tobytes()
    q = {
        "tx": "fskhip_modulate_device (FSKCore.modulateData), %d frames of %d payload bytes per stream, one per %d-sample slot" % (F, payload_len, slot),
        "noise": "Gaussian, sigma^2 = mean square of the stream's whole buffer (padding included) / 10^(SNR/10), SNR %.1f dB "
                 "(power definition of fsk-demodulation.node.test.ts:1184-1205)" % snr,
        "frames": frames, "frame_success_rate": round(ok / frames, 6),
        "frame_success_definition": "the slot's decoded bytes are exactly the payload (nothing lost, nothing extra)",
        "frame_delivery_rate": round(delivered / frames, 6),
        "frame_delivery_definition": "the payload appears whole and in order among the slot's decoded bytes",
        "frames_with_payload_length": len_match,
        "ber_on_length_matched_frames": (bit_err / (8.0 * payload_len * len_match)) if len_match else None,
        "bit_errors": bit_err,
        "modulate_Msamples_per_s": round(F * S * frame_len / t_mod / 1e6, 1),
    }
    # ---- oracle on a strided sample, same cuts
    if oracle_seconds > 0:
        from oracle import pyoracle as po
        n_cpu = int(max(1, min(S, oracle_seconds * 7.0e6 // N)))
        rows = np.unique(np.linspace(0, S - 1, n_cpu).astype(np.int64))
        xs = x.index_select(0, torch.as_tensor(rows, device="cuda"))[:, :N].cpu().numpy()
        t0 = time.perf_counter()
        same = 0
        for j, s in enumerate(rows):
            o = po.OracleCore(cfg)
            good = True
            for f in range(F):
                n_f = slot if f + 1 < F else N - f * slot
                ob, _ = o.demodulate(xs[j, f * slot:f * slot + n_f])
                if ob != got[f][s, :got_n[f][s]].tobytes():
                    good = False
            same += good
        dt = time.perf_counter() - t0
        q.update({"oracle_streams_checked": int(len(rows)), "oracle_streams_byte_identical": int(same),
                  "oracle_Msamples_per_s": round(len(rows) * N / dt / 1e6, 3)})
    return q


def measure_modulate(torch, np, wm, eng, S, N, pitch, payload_len, seed, stream, steps, warmup, sync):
    """FSKCore.modulateData on the GPU (fskhip_modulate_device): every stream's 10 s buffer filled with back-to-back frames, one
    modulate call per frame slot (what --workload c5 transmits).  Returns (samples written per step, kernel ms per step from the
    library's HIP events, launches per step, the device buffer and output lengths, payloads, slot)."""
    frame_len = eng.modulated_length(payload_len)
    slot = (frame_len + 1952 + 15) // 16 * 16
    F = max(1, N // slot)
    rng = np.random.RandomState((seed ^ 0x30D) & 0x7FFFFFFF)
    payloads = rng.randint(0, 256, size=(F, S, payload_len)).astype(np.uint8)
    x = torch.zeros((S, pitch), dtype=torch.float32, device="cuda")
    d_pay = [torch.as_tensor(payloads[f], device="cuda") for f in range(F)]
    d_lens = torch.full((S,), payload_len, dtype=torch.int32, device="cuda")
    d_olens = torch.empty(S, dtype=torch.int32, device="cuda")

    def step():
        for f in range(F):
            eng.modulate_device(d_pay[f].data_ptr(), d_lens.data_ptr(), payload_len, x.data_ptr() + 4 * f * slot, pitch,
                                d_olens.data_ptr(), stream)
    for _ in range(max(1, warmup)):
        step()
    sync()
    eng.timing_begin()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    sync()
    wall = time.perf_counter() - t0
    nl, ms = eng.timing_end()
    return dict(samples_per_step=float(S) * F * frame_len, kernel_ms_per_step=ms / steps, launches_per_step=nl // steps,
                wall_s_per_step=wall / steps, x=x, olens=d_olens, payloads=payloads, slot=slot, frames=F, frame_len=frame_len)


def worker_mod(args):
    """--workload mod: one line for modulateData (VERDICT r04 "missing" #2): Msamples/s written, against the HBM WRITE roofline
    (4 B written per output sample), kernel time from the library's HIP events; a strided sample of streams is
    compared with the oracle's modulateData (fp64 engines: bit for bit; fp32 engines: at most one float ulp on at most 1e-4 of
    the samples -- the bound tests/test_gpu_parity.py holds them to)."""
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    import numpy as np
    import torch
    import __graft_entry__ as ge
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (the engine has no CPU fallback)")
    torch.cuda.set_device(local_rank)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
    if rank == 0:
        ge.build()
    if dist is not None:
        dist.barrier()
    import webaudio_modem_amd as wm
    from webaudio_modem_amd.sharding import max_over_ranks
    cfg = WORKLOADS["c5"]["cfg"]
    payload_len = WORKLOADS["c5"]["payload"]
    S = args.streams if args.streams != 65536 else 16384      # (config #5: 16 384 streams unless --streams is given)
    N = (int(round(args.seconds * 48000)) + 31) // 32 * 32
    pitch = (N + 63) // 64 * 64
    prec = wm.PRECISION_F32 if args.precision == "f32" else wm.PRECISION_F64
    eng = wm.FSKEngine(S, cfg, device=local_rank, precision=prec)
    stream = torch.cuda.current_stream().cuda_stream
    sync = torch.cuda.synchronize
    if dist is not None:
        dist.barrier()
    m = measure_modulate(torch, np, wm, eng, S, N, pitch, payload_len, 0xF5C0DE + 0x1000 * rank, stream, args.steps, args.warmup, sync)
    elapsed = max_over_ranks(m["wall_s_per_step"] * args.steps, dist, "cuda")
    if rank == 0 and args.dump_outputs:
        # the last step's signal (a fixed sample of streams, whole rows) and every stream's output length (that of the last frame slot)
        rows = dump_rows(S, 4 * pitch)
        write_dump(args.dump_outputs, {
            "signal": m["x"].index_select(0, torch.as_tensor(rows, device="cuda")).cpu().numpy(),
            "signal_rows": np.asarray(rows, np.float64),
            "out_lengths": m["olens"].cpu().numpy().astype(np.float64)})
    # ---- parity + cpu baseline on a strided sample (rank 0): frame 0 of each sampled stream against the oracle's modulateData
    cpu_obj, parity_ok = None, True
    if rank == 0 and args.full and args.cpu_seconds > 0:
        from oracle import pyoracle as po
        rows = np.unique(np.linspace(0, S - 1, 64).astype(np.int64))
        xs = m["x"].index_select(0, torch.as_tensor(rows, device="cuda"))[:, :m["frame_len"]].cpu().numpy()
        o = po.OracleCore(cfg)
        t0 = time.perf_counter()
        refs = [o.modulate(bytes(m["payloads"][0][int(s_)])) for s_ in rows]
        dt = time.perf_counter() - t0
        n_diff = sum(int(np.count_nonzero(xs[j] != refs[j])) for j in range(len(rows)))
        worst = max(float(np.max(np.abs(xs[j].astype(np.float64) - refs[j].astype(np.float64)))) for j in range(len(rows)))
        total = len(rows) * m["frame_len"]
        parity_ok = (n_diff == 0) if args.precision == "f64" else (worst <= 1.2e-7 and n_diff <= max(1, total // 10000))
        cpu_obj = {"value": round(total / dt / 1e6, 3), "unit": "Msamples/s", "cores": 1, "kind": "port",
                   "sample": "%d streams x one %d-sample frame, oracle/fsk_oracle.c modulateData (scalar fp64 C port, V8's Math.sin restated, 1 thread)" % (len(rows), m["frame_len"]),
                   "parity_ok": parity_ok, "samples_checked": total, "samples_differing": n_diff, "max_abs_difference": worst,
                   "host_cpus": os.cpu_count()}
    value = float(world) * m["samples_per_step"] * args.steps / elapsed / 1e6
    alg = 4.0 * m["samples_per_step"]
    ksec = m["kernel_ms_per_step"] / 1e3
    achieved = alg / ksec / 1e9
    if rank == 0:
        print(json.dumps({
            "metric": "Msamples/s modulated (FSKCore.modulateData, outputs written to HBM)", "value": round(value, 1), "unit": "Msamples/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 3),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64",
            "dtype_note": "phase accumulation and sine in doubles, Float32Array store (fsk.ts:398-406); --precision %s engine: %s" % (
                args.precision, "Math.sin by V8's operation sequence, bit-identical signal" if args.precision == "f64" else
                "sine carried as a rotated phasor corrected by the exactly known phase rounding, refreshed every 32 samples"),
            "data": "synthetic",
            "config": {"workload": "BASELINE config #5 TX leg: %d streams/GPU x %d frames of %d payload bytes (%d samples each, one per %d-sample slot), Bell-202 1200 baud @48 kHz"
                                   % (S, m["frames"], payload_len, m["frame_len"], m["slot"]),
                       "streams_per_gpu": S, "frames_per_stream": m["frames"], "samples_per_frame": m["frame_len"],
                       "parallelism": "streams sharded across %d GPU(s), no collective" % world},
            "roofline": {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 4),
                         "traffic": None, "kernel": "fsk::modulate_wide_kernel<%s>" % ("true" if args.precision == "f64" else "false"),
                         "avg_kernel_ms": round(m["kernel_ms_per_step"] / max(1, m["launches_per_step"]), 4), "launches": m["launches_per_step"] * args.steps,
                         "algorithmic_bytes_per_launch": alg / max(1, m["launches_per_step"]),
                         "binding_note": "4 B written per output sample; the kernel is bound by the f64 phase / sine chain of one lane per stream, not by HBM"},
            "cpu_baseline": cpu_obj}), flush=True)
    eng.close()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    if not parity_ok:
        sys.exit(3)


def worker(args):
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    dry = args.dry_engine

    import numpy as np
    import torch
    import __graft_entry__ as ge

    if not dry:
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs a GPU (the engine has no CPU fallback)")
        torch.cuda.set_device(local_rank)
    dev = "cpu" if dry else "cuda"
    sync = (lambda: None) if dry else torch.cuda.synchronize
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if dry:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
    if dry and os.environ.get("BENCH_DRY_FAIL_RANK") == str(rank):   # launcher test: a rank that dies must fail the whole run
        sys.exit(7)
    # one rank runs make (a no-op when the shipped libraries are current); the others must not race it in the same tree
    if rank == 0 and not dry:
        ge.build()
    if dist is not None:
        dist.barrier()
    from webaudio_modem_amd.sharding import max_over_ranks, stream_shard
    wm = None
    if not dry:
        import webaudio_modem_amd as wm
        if args.opt:
            import webaudio_modem_amd.engine as wme
            bench_opts = dict(o.split("=", 1) for o in args.opt)
            wme.option_hook = lambda n_streams, precision: bench_opts

    wl = WORKLOADS[args.workload]
    cfg = wl["cfg"]
    snr = args.snr_db if args.snr_db is not None else wl["snr"]
    strong_only = args.total_streams > 0
    if strong_only:
        first_stream, S = stream_shard(args.total_streams, rank, world)
        total_streams = args.total_streams
        scaling = "strong"
    else:
        S = args.streams
        first_stream = rank * S
        total_streams = S * world
        scaling = "weak"
    sr = 48000
    N = int(round(args.seconds * sr))
    N = (N + 31) // 32 * 32
    pitch = (N + 63) // 64 * 64 + args.pitch_pad  # 256-B row pitch
    spb = sr // int(cfg.get("baudRate", 1200))
    seed = 0xF5C0DE + 0x1000 * rank

    def per_stream_cfgs(first, count):
        if not wl.get("per_stream"):   # config #4: every stream its own tone pair (per-stream constants in the kernels)
            return None
        if wl.get("tones1200"):
            return [dict(cfg, markFrequency=1200 + 7 * ((first + s) % 13), spaceFrequency=2200 + 5 * ((first + s) % 11)) for s in range(count)]
        return [dict(cfg, markFrequency=1000 + 10 * ((first + s) % 100), spaceFrequency=1200 + 10 * ((first + s) % 100))
                for s in range(count)]

    cfgs = per_stream_cfgs(first_stream, S)
    c5q = None
    if dry:
        eng = DryEngine(S)
        x = out = counts = eod = None
        out_pitch = eng.max_bytes(N)
        stream = None

        def step():
            eng.demodulate_device()
    else:
        prec = wm.PRECISION_F32 if args.precision == "f32" else wm.PRECISION_F64
        eng = wm.FSKEngine(S, cfgs if cfgs is not None else cfg, device=local_rank, precision=prec)
        stream = torch.cuda.current_stream().cuda_stream
        x = torch.empty((S, pitch), dtype=torch.float32, device="cuda")
        out_pitch = eng.max_bytes(N)
        out = torch.empty((S, out_pitch), dtype=torch.uint8, device="cuda")
        counts = torch.empty(S, dtype=torch.int32, device="cuda")
        eod = torch.empty(S, dtype=torch.int32, device="cuda")
        if wl.get("roundtrip"):
            c5q = c5_build_and_score(torch, np, wm, eng, cfg, x, N, pitch, snr, seed, wl["payload"], stream,
                                     args.cpu_seconds if rank == 0 else 0, first_stream, args.full)
        elif wl.get("idle_db") is not None:
            # one frame per stream (the synthesiser's first, with its random lead-in and level), zeros behind it, then noise
            # over everything: sigma^2 = (mean square of the stream's frame) / 10^(idle_db / 10).  add_awgn_device takes its
            # SNR against the mean square of the WHOLE buffer, of which the frame is frame_len / N.
            import math
            frame_len = eng.modulated_length(wl["payload"])
            lead_max = 10 * spb
            n0 = min(N, (lead_max + frame_len + 31) // 32 * 32)
            x.zero_()
            eng.synth_device(x.data_ptr(), n0, pitch, wl["payload"], seed, lead_max, 0.1, 1.0, stream)
            torch.cuda.synchronize()
            ends = np.array([eng.synth_stream_params(seed, s_, lead_max, 0.1, 1.0)[0] for s_ in range(S)], np.int64) + frame_len
            d_end = torch.as_tensor(ends, device="cuda")
            c0 = int(ends.min())
            if c0 < n0:   # what the synthesiser put behind each stream's first frame
                cols = torch.arange(c0, n0, device="cuda")
                x[:, c0:n0] *= (cols[None, :] < d_end[:, None])
            eng.add_awgn_device(x.data_ptr(), N, pitch, wl["idle_db"] - 10.0 * math.log10(N / float(frame_len)), seed ^ 0xA36, stream)
        else:
            eng.synth_device(x.data_ptr(), N, pitch, wl["payload"], seed, args.lead_max if args.lead_max is not None else 10 * spb, 0.1, 1.0, stream)
            if snr is not None:
                eng.add_awgn_device(x.data_ptr(), N, pitch, snr, seed ^ 0xA36, stream)
        torch.cuda.synchronize()

        def fill_idle(e_, idle_db):
            # (--workload idle's generator, for the side measurement below: one frame per stream, zeros, a noise floor idle_db under the frame)
            import math
            frame_len = e_.modulated_length(wl["payload"])
            lead_max = 10 * spb
            n0 = min(N, (lead_max + frame_len + 31) // 32 * 32)
            x.zero_()
            e_.synth_device(x.data_ptr(), n0, pitch, wl["payload"], seed, lead_max, 0.1, 1.0, stream)
            torch.cuda.synchronize()
            ends = np.array([e_.synth_stream_params(seed, s_, lead_max, 0.1, 1.0)[0] for s_ in range(S)], np.int64) + frame_len
            c0 = int(ends.min())
            if c0 < n0:
                cols = torch.arange(c0, n0, device="cuda")
                x[:, c0:n0] *= (cols[None, :] < torch.as_tensor(ends, device="cuda")[:, None])
            e_.add_awgn_device(x.data_ptr(), N, pitch, idle_db - 10.0 * math.log10(N / float(frame_len)), seed ^ 0xA36, stream)
            torch.cuda.synchronize()

        def step():
            eng.demodulate_device(x.data_ptr(), N, pitch, out.data_ptr(), out_pitch, counts.data_ptr(), eod.data_ptr(),
                                  0, stream)

    # ---- first pass doubles as the parity sample: copy its outputs before state moves on -------
    step()
    sync()
    kernel_name = eng.last_kernel()
    lanes_main = eng.blk_lanes() if ("demod_blk_kernel" in kernel_name or "demod_blk6_kernel" in kernel_name) else None
    first_counts = np.zeros(S, np.int64) if dry else counts.cpu().numpy().astype(np.int64)
    cpu_obj = None
    parity_ok = True
    oracle_rows = {}
    if rank == 0 and args.full and args.cpu_seconds > 0 and not dry:
        est_rate = 7.0e6  # oracle samples/s/core
        n_cpu_streams = int(max(1, min(S, args.cpu_seconds * est_rate // N)))
        # a strided sample over the whole batch (first and last groups included)
        rows = np.unique(np.linspace(0, S - 1, n_cpu_streams).astype(np.int64))
        idx = torch.as_tensor(rows, device="cuda")
        xs = x.index_select(0, idx)[:, :N].cpu().numpy()
        gpu_bytes = out.index_select(0, idx).cpu().numpy()
        from oracle import pyoracle as po
        t0 = time.perf_counter()
        mism = 0
        for j, s in enumerate(rows):
            o = po.OracleCore(cfgs[int(s)] if cfgs is not None else cfg)
            ob, _ = o.demodulate(xs[j])
            oracle_rows[int(s)] = ob            # kept: the exact (fp64) engine's bytes are checked against the same oracle run
            gb = gpu_bytes[j, :first_counts[s]].tobytes()
            if ob != gb:
                mism += 1
        dt = time.perf_counter() - t0
        parity_ok = mism == 0
        cpu_obj = {
            "value": round(len(rows) * N / dt / 1e6, 3), "unit": "Msamples/s", "cores": 1, "kind": "port",
            "sample": "%d streams (evenly strided over the rank-0 batch) x %d samples, oracle/fsk_oracle.c (scalar fp64 C "
                      "port of the reference, -O2, 1 thread)" % (len(rows), N),
            "parity_ok": parity_ok, "streams_byte_identical": int(len(rows) - mism), "streams_checked": int(len(rows)),
            "host_cpus": os.cpu_count(),
        }
        if c5q is not None and c5q.get("oracle_streams_checked") is not None:
            parity_ok = parity_ok and c5q["oracle_streams_checked"] == c5q["oracle_streams_byte_identical"]

    if args.probe_reads and not dry:
        # counter calibration aid: the same buffer streamed with the kernel's read pattern and nothing else
        for _ in range(args.probe_reads):
            eng.probe_read_device(x.data_ptr(), N, pitch, stream)
        torch.cuda.synchronize()

    # (the engine picks between its four-wave kernels by the previous call's tile statistics, which arrive with an
    # asynchronous copy: which call switches depends on host / GPU timing.  Let the choice settle before the timed region -- two
    # synchronised steps: the first one's statistics are in when the second is issued -- and record the kernel of the first and
    # of the last timed launch: a region that mixes two kernels says so.)
    kernel_first = None
    if not dry:
        for _ in range(2):
            step()
            sync()
        step()
        sync()
        kernel_first = eng.last_kernel()
    elapsed, n_launch, kernel_ms = measure(sync, dist, eng, step, args.steps, args.warmup, dev)
    if not dry:
        kernel_name = eng.last_kernel()
        lanes_main = eng.blk_lanes() if ("demod_blk_kernel" in kernel_name or "demod_blk6_kernel" in kernel_name) else None
    if rank == 0 and args.dump_outputs:
        # what the last timed call returned: every stream's byte count and 'eod' count, and the bytes of a fixed sample of
        # streams (-1 past a stream's count: out_pitch bounds the bytes, the rest of a row is not written)
        rows = dump_rows(S, 4 * out_pitch)
        n_out = counts.cpu().numpy().astype(np.int64)
        b = out.index_select(0, torch.as_tensor(rows, device="cuda")).cpu().numpy().astype(np.float32)
        b[np.arange(out_pitch)[None, :] >= n_out[rows][:, None]] = -1.0
        write_dump(args.dump_outputs, {"bytes": b, "bytes_rows": np.asarray(rows, np.float64),
                                       "counts": n_out.astype(np.float64), "eod": eod.cpu().numpy().astype(np.float64)})

    # ---- the shader clock the device holds under this load: a one-wave probe (fskhip_clock_probe_*) started
    # first, a few more steps of the same work behind it.  Outside the timed region on purpose: the probe's wave takes a slot
    # that one workgroup of a full-device launch has to wait for.
    clock_ghz = None
    if rank == 0 and not dry and args.full and not args.no_clock_probe:
        try:
            per_step_ms = elapsed / args.steps * 1e3
            k_probe = max(2, min(6, int(250.0 / max(per_step_ms, 1e-3)) + 1))
            eng.clock_probe_begin(min(2000.0, 0.8 * k_probe * per_step_ms))
            for _ in range(k_probe):
                step()
            sync()
            clock_ghz, _covered = eng.clock_probe_end()
        except Exception as ex:
            print("clock probe failed: %s" % ex, file=sys.stderr)

    # ---- N > 1: the strong-scaling shape of the same job (BASELINE config #3 as written), same line -------------------
    strong = None
    if world > 1 and not strong_only and args.full:
        first2, S2 = stream_shard(args.streams, rank, world)
        if dry:
            e2 = DryEngine(S2)

            def step2():
                e2.demodulate_device()
        else:
            cfgs2 = per_stream_cfgs(first2, S2)
            e2 = wm.FSKEngine(S2, cfgs2 if cfgs2 is not None else cfg, device=local_rank, precision=prec)

            def step2():   # the first S2 rows of this rank's resident batch
                e2.demodulate_device(x.data_ptr(), N, pitch, out.data_ptr(), out_pitch, counts.data_ptr(), eod.data_ptr(), 0, stream)
        step2()
        sync()
        el2, nl2, kms2 = measure(sync, dist, e2, step2, args.steps, args.warmup, dev)
        k2 = e2.last_kernel()
        lanes2 = e2.blk_lanes()
        e2.close()
        v2 = float(args.streams) * N * args.steps / el2 / 1e6
        strong = {"total_streams": args.streams, "streams_per_gpu": S2, "Msamples_per_s": round(v2, 1),
                  "ms_per_step": round(el2 / args.steps * 1e3, 3), "kernel": k2, "streams_per_workgroup": lanes2,
                  "avg_kernel_ms_rank0": round(kms2 / max(1, nl2), 4),
                  "frac_of_hbm_peak_per_gpu": round(v2 / world * 4 / 1e3 / HBM_PEAK_GBS, 4),
                  "note": "BASELINE config #3 as written: %d streams in total, contiguous blocks of %d per GPU, no collective" % (args.streams, S2)}

    # every rank reports what it processed: the aggregate is checked, not assumed
    ranks_reported, streams_all = 1, S
    if dist is not None:
        t = torch.tensor([1.0, float(S), 0.0 if parity_ok else 1.0], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        ranks_reported, streams_all = int(t[0].item()), int(t[1].item())
        parity_ok = parity_ok and t[2].item() == 0.0

    # ---- side measurements (rank 0, one GPU): reported in `config`, never as `value` ------------------------------
    side = {}
    if rank == 0 and world == 1 and args.full and not args.no_side and args.precision == "f32" and cfgs is None and not dry and c5q is None:
        k_side = max(2, min(args.steps, 4))
        # (0) one GPU's share of BASELINE configs #3 (65 536 streams over eight GPUs = 8 192) and #5 (16 384 over eight = 2 048):
        # the strong-scaling estimate in the driver's own record (VERDICT r03 "missing" 3).  Same signal, same length: the first
        # rows of the resident batch.
        try:
            shares = {}
            for s_share in (8192, 2048):
                if s_share >= S:
                    continue
                es = wm.FSKEngine(s_share, cfg, device=local_rank, precision=prec)

                def step_s():
                    es.demodulate_device(x.data_ptr(), N, pitch, out.data_ptr(), out_pitch, counts.data_ptr(), eod.data_ptr(), 0, stream)
                step_s()
                nl, ms = timed_steps(sync, es, step_s, k_side)
                r = s_share * N * nl / (ms / 1e3) / 1e6
                shares[str(s_share)] = {"Msamples_per_s": round(r, 1), "frac_of_hbm_peak": round(r * 4 / 1e3 / HBM_PEAK_GBS, 4),
                                        "kernel": es.last_kernel(), "streams_per_workgroup": es.blk_lanes(),
                                        "x8_GPUs_Msamples_per_s": round(8 * r, 1)}
                es.close()
            side["per_gpu_share"] = shares
        except Exception as ex:
            side["per_gpu_share"] = {"error": str(ex)}
        # (0b) FSKCore.modulateData (VERDICT r04 "missing" #2): config #5's TX leg in short -- 16 384 streams, the 10 s buffer filled
        # with frames -- as a one-line summary; the full line with its own oracle check is `bench.py --workload mod`
        try:
            s_mod = min(S, 16384)
            em = wm.FSKEngine(s_mod, cfg, device=local_rank, precision=prec)
            mm = measure_modulate(torch, np, wm, em, s_mod, N, pitch, wl["payload"], seed, stream, 2, 1, sync)
            rm = mm["samples_per_step"] / (mm["kernel_ms_per_step"] / 1e3) / 1e6
            side["modulate"] = {"streams": s_mod, "frames_per_stream": mm["frames"], "samples_per_frame": mm["frame_len"],
                                "Msamples_per_s": round(rm, 1), "write_GB_per_s": round(rm * 4 / 1e3, 1),
                                "frac_of_hbm_peak": round(rm * 4 / 1e3 / HBM_PEAK_GBS, 4), "kernel": "fsk::modulate_wide_kernel<false>",
                                "note": "fskhip_modulate_device, kernel time from the library's HIP events; `bench.py --workload mod` is the full line"}
            del mm
            em.close()
        except Exception as ex:
            side["modulate"] = {"error": str(ex)}
        # (1) the EXACT path: the fp64 engine -- the reference's operations in the reference's order -- on the
        # SAME batch at its FULL length, its first pass checked byte for byte against the oracle's run of the strided sample
        # above (the engine starts from the same reset state the oracle does); also reported top-level as "exact"
        try:
            e64 = wm.FSKEngine(S, cfg, device=local_rank, precision=wm.PRECISION_F64)

            def step64():
                e64.demodulate_device(x.data_ptr(), N, pitch, out.data_ptr(), out_pitch, counts.data_ptr(), eod.data_ptr(), 0, stream)
            step64()
            sync()
            chk = None
            if oracle_rows:
                rows64 = np.array(sorted(oracle_rows), np.int64)
                idx64 = torch.as_tensor(rows64, device="cuda")
                b64 = out.index_select(0, idx64).cpu().numpy()
                c64 = counts.index_select(0, idx64).cpu().numpy().astype(np.int64)
                same64 = sum(1 for j, s_ in enumerate(rows64) if b64[j, :c64[j]].tobytes() == oracle_rows[int(s_)])
                chk = {"streams_checked": int(len(rows64)), "streams_byte_identical": int(same64)}
                if same64 != len(rows64):
                    parity_ok = False
            nl, ms = timed_steps(sync, e64, step64, k_side)
            r = S * N * nl / (ms / 1e3) / 1e6
            side["f64_parity_path"] = {"streams": S, "samples_per_stream": N, "kernel": e64.last_kernel(),
                                       "Msamples_per_s": round(r, 1), "frac_of_hbm_peak": round(r * 4 / 1e3 / HBM_PEAK_GBS, 4),
                                       "avg_kernel_ms": round(ms / max(1, nl), 4), "launches": nl,
                                       **(chk or {"streams_checked": 0, "streams_byte_identical": 0})}
            e64.close()
        except Exception as ex:  # a side measurement must not take the headline down
            side["f64_parity_path"] = {"error": str(ex)}
        # (2) a batch large enough to give every SIMD four waves with one wave per 64-stream group
        try:
            S2, n2 = 262144, 24000 // 32 * 32
            p2 = (n2 + 63) // 64 * 64
            e2 = wm.FSKEngine(S2, cfg, device=local_rank, precision=prec)
            x2 = torch.empty((S2, p2), dtype=torch.float32, device="cuda")
            o2 = torch.empty((S2, e2.max_bytes(n2)), dtype=torch.uint8, device="cuda")
            c2 = torch.empty(S2, dtype=torch.int32, device="cuda")
            e2.synth_device(x2.data_ptr(), n2, p2, wl["payload"], seed, 10 * spb, 0.1, 1.0, stream)
            if snr is not None:
                e2.add_awgn_device(x2.data_ptr(), n2, p2, snr, seed ^ 0xA36, stream)

            def step2():
                e2.demodulate_device(x2.data_ptr(), n2, p2, o2.data_ptr(), o2.shape[1], c2.data_ptr(), 0, 0, stream)
            step2()
            nl, ms = timed_steps(sync, e2, step2, k_side)
            r = S2 * n2 * nl / (ms / 1e3) / 1e6
            side["large_batch"] = {"streams": S2, "samples_per_stream": n2, "kernel": e2.last_kernel(),
                                   "Msamples_per_s": round(r, 1), "frac_of_hbm_peak": round(r * 4 / 1e3 / HBM_PEAK_GBS, 4)}
            e2.close()
            del x2, o2, c2
        except Exception as ex:
            side["large_batch"] = {"error": str(ex)}
        # (3) PCIe-inclusive: host buffers through fskhip_demodulate_host (H2D + kernel + D2H; calls longer than ~1.5 time
        # slabs are a two-buffer pipeline, include/fskhip.h), from pageable and from page-locked memory
        try:
            S3, n3 = 16384, 48000
            e3 = wm.FSKEngine(S3, cfg, device=local_rank, precision=prec)
            h = np.ascontiguousarray(x[:S3, :n3].cpu().numpy())
            hp = wm.pinned_empty((S3, n3), np.float32)
            hp[:] = h
            rates = {}
            for name, buf in (("pageable", h), ("pinned", hp)):
                e3.reset()
                e3.demodulate_data(buf)  # first call allocates the staging buffers
                best = 1e9
                for _ in range(2):
                    e3.reset()
                    t1 = time.perf_counter()
                    e3.demodulate_data(buf)
                    best = min(best, time.perf_counter() - t1)
                rates[name] = round(S3 * n3 / best / 1e6, 1)
            side["pcie_inclusive"] = {"streams": S3, "samples_per_stream": n3, "Msamples_per_s": rates["pinned"],
                                      "Msamples_per_s_pageable": rates["pageable"],
                                      "GB_per_s_of_input": round(rates["pinned"] * 4 / 1e3, 1),
                                      "note": "fskhip_demodulate_host: H2D + kernel + D2H pipelined over time slabs, wall clock "
                                              "incl. the Python wrapper; never the headline"}
            e3.close()
            del hp
        except Exception as ex:
            side["pcie_inclusive"] = {"error": str(ex)}
        # (4) the batched generic IIRFilter (SURVEY 8 row a3 / f3', filters.ts:8-106: fskhip_iir_*): order-2 Butterworth low-pass,
        # processBuffer semantics (f32 in / out), 8 B per sample against the HBM roofline -- VERDICT r05 #7: a driver-recorded number
        try:
            iir = {}
            co = wm.FilterDesign.butterworthLowpass(1200, 48000)
            n_i = 48000
            for s_i in (65536, 16384):
                xi = torch.randn((s_i, n_i), dtype=torch.float32, device="cuda")
                yi = torch.empty_like(xi)
                for pname, pv in (("f32", wm.PRECISION_F32), ("f64", wm.PRECISION_F64)):
                    flt = wm.IIRFilterBatch(co["b"], co["a"], s_i, precision=pv)
                    flt.process_device(xi.data_ptr(), n_i, n_i, yi.data_ptr(), n_i, stream)
                    sync()
                    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    ev0.record()
                    for _ in range(5):
                        flt.process_device(xi.data_ptr(), n_i, n_i, yi.data_ptr(), n_i, stream)
                    ev1.record()
                    sync()
                    ms_i = ev0.elapsed_time(ev1) / 5
                    r_i = s_i * n_i / (ms_i / 1e3) / 1e6
                    iir["%d_%s" % (s_i, pname)] = {"Msamples_per_s": round(r_i, 1), "GB_per_s": round(r_i * 8 / 1e3, 1),
                                                   "frac_of_hbm_peak": round(r_i * 8 / 1e3 / HBM_PEAK_GBS, 4), "avg_kernel_ms": round(ms_i, 4)}
                    flt.close()
                del xi, yi
            iir["note"] = ("fsk::iir_kernel, order 2 (butterworthLowpass(1200, 48000)), %d samples per stream, f32 in / out = 8 algorithmic bytes per sample; "
                           "torch events on the launch stream (the call's stream argument is torch's current stream)" % n_i)
            side["iir"] = iir
        except Exception as ex:
            side["iir"] = {"error": str(ex)}
        # (4b) one GPU's share of BASELINE config #4 over eight GPUs: 4 096 streams, 300 baud, every stream its own tone pair
        # (mark_s = 1000 + 10 (s mod 100), space_s = mark_s + 200) -- since round 6 the seven-wave kernel's per-stream instantiation
        try:
            s4 = 4096
            w4 = WORKLOADS["c4"]
            cfgs4 = [dict(w4["cfg"], markFrequency=1000 + 10 * (s_ % 100), spaceFrequency=1200 + 10 * (s_ % 100)) for s_ in range(s4)]
            e4 = wm.FSKEngine(s4, cfgs4, device=local_rank, precision=prec)
            x4 = torch.empty((s4, pitch), dtype=torch.float32, device="cuda")
            op4 = e4.max_bytes(N)
            o4 = torch.empty((s4, op4), dtype=torch.uint8, device="cuda")
            c4 = torch.empty(s4, dtype=torch.int32, device="cuda")
            e4.synth_device(x4.data_ptr(), N, pitch, w4["payload"], seed, 10 * (sr // 300), 0.1, 1.0, stream)
            torch.cuda.synchronize()

            def step4():
                e4.demodulate_device(x4.data_ptr(), N, pitch, o4.data_ptr(), op4, c4.data_ptr(), 0, 0, stream)
            step4()
            sync()
            chk4 = {"streams_checked": 0, "streams_byte_identical": 0}
            if args.cpu_seconds > 0:
                from oracle import pyoracle as po
                rows4 = np.unique(np.linspace(0, s4 - 1, int(max(4, 0.25 * args.cpu_seconds * 7.0e6 // N))).astype(np.int64))
                i4 = torch.as_tensor(rows4, device="cuda")
                xs4 = x4.index_select(0, i4)[:, :N].cpu().numpy()
                b4 = o4.index_select(0, i4).cpu().numpy()
                n4 = c4.index_select(0, i4).cpu().numpy().astype(np.int64)
                same4 = sum(1 for j, s_ in enumerate(rows4) if po.OracleCore(cfgs4[int(s_)]).demodulate(xs4[j])[0] == b4[j, :n4[j]].tobytes())
                chk4 = {"streams_checked": int(len(rows4)), "streams_byte_identical": int(same4)}
                if same4 != len(rows4):
                    parity_ok = False
            nl, ms = timed_steps(sync, e4, step4, k_side)
            r4 = s4 * N * nl / (ms / 1e3) / 1e6
            side["c4_per_gpu_share"] = {"streams": s4, "samples_per_stream": N, "kernel": e4.last_kernel(), "streams_per_workgroup": e4.blk_lanes(),
                                        "Msamples_per_s": round(r4, 1), "frac_of_hbm_peak": round(r4 * 4 / 1e3 / HBM_PEAK_GBS, 4),
                                        "x8_GPUs_Msamples_per_s": round(8 * r4, 1), **chk4,
                                        "note": "BASELINE config #4 (32 768 streams with per-stream mark / space, 300 baud) as one of eight GPUs would hold it"}
            e4.close()
            del x4, o4, c4
        except Exception as ex:
            side["c4_per_gpu_share"] = {"error": str(ex)}
        # (5) the unfavourable shapes of the SAME batch size: the resident buffer regenerated in place, LAST (nothing
        # above needs the headline's signal any more).  staggered: every stream's frames at a random offset within one frame length
        # (a reset in some lane of a wave every few tiles; the headline's streams all start within ten bit cells of one another);
        # idle: ONE frame per stream, then a noise floor 30 dB under it (every stream fires 'eod' on its own schedule).  Each with
        # the kernel the library chose and its own oracle check of a strided sample of the first pass.
        for sname in ("staggered", "idle"):
            try:
                es = wm.FSKEngine(S, cfg, device=local_rank, precision=prec)
                frame_len_s = es.modulated_length(wl["payload"])
                if sname == "staggered":
                    es.synth_device(x.data_ptr(), N, pitch, wl["payload"], seed, frame_len_s, 0.1, 1.0, stream)
                    torch.cuda.synchronize()
                else:
                    fill_idle(es, 30.0)

                def step_u():
                    es.demodulate_device(x.data_ptr(), N, pitch, out.data_ptr(), out_pitch, counts.data_ptr(), eod.data_ptr(), 0, stream)
                step_u()
                sync()
                chk = {"streams_checked": 0, "streams_byte_identical": 0}
                if args.cpu_seconds > 0:
                    from oracle import pyoracle as po
                    rows_u = np.unique(np.linspace(0, S - 1, int(max(4, min(S, 0.4 * args.cpu_seconds * 7.0e6 // N)))).astype(np.int64))
                    idx_u = torch.as_tensor(rows_u, device="cuda")
                    xs_u = x.index_select(0, idx_u)[:, :N].cpu().numpy()
                    b_u = out.index_select(0, idx_u).cpu().numpy()
                    c_u = counts.index_select(0, idx_u).cpu().numpy().astype(np.int64)
                    e_u = eod.index_select(0, idx_u).cpu().numpy().astype(np.int64)
                    same_u = 0
                    for j in range(len(rows_u)):
                        ob, oe = po.OracleCore(cfg).demodulate(xs_u[j])
                        same_u += (ob == b_u[j, :c_u[j]].tobytes()) and (oe == int(e_u[j]))
                    chk = {"streams_checked": int(len(rows_u)), "streams_byte_identical": int(same_u)}
                    if same_u != len(rows_u):
                        parity_ok = False
                for _ in range(2):                       # (the kernel choice by tile statistics settles, as for the headline)
                    step_u()
                    sync()
                nl, ms = timed_steps(sync, es, step_u, k_side)
                r = S * N * nl / (ms / 1e3) / 1e6
                side[sname] = {"streams": S, "samples_per_stream": N, "kernel": es.last_kernel(), "Msamples_per_s": round(r, 1),
                               "frac_of_hbm_peak": round(r * 4 / 1e3 / HBM_PEAK_GBS, 4), "avg_kernel_ms": round(ms / max(1, nl), 4), **chk,
                               "signal": ("lead_max_samples = %d (one frame length): frames -- and resets -- do not line up across a wave" % frame_len_s) if sname == "staggered"
                               else "one frame per stream, then a Gaussian floor 30 dB under it: every stream fires 'eod' each samplesForEOD decimated samples on its own schedule"}
                es.close()
            except Exception as ex:
                side[sname] = {"error": str(ex)}

    total_samples = float(total_streams) * N * args.steps if strong_only else float(streams_all) * N * args.steps
    value = total_samples / elapsed / 1e6
    alg_bytes_per_launch = 4.0 * S * N  # 4 B read per input sample
    avg_kernel_s = max(1e-12, kernel_ms / 1e3 / max(1, n_launch))
    achieved = alg_bytes_per_launch / avg_kernel_s / 1e9
    decoded = int(first_counts.sum())

    def committed(name):
        """a committed profile of THIS kernel (profiles/<round>_<name>.json): the newest round that has one"""
        for rnd in ("r06", "r05", "r04", "r03", "r02"):
            pth = os.path.join(ROOT, "profiles", "%s_%s.json" % (rnd, name))
            if os.path.exists(pth):
                with open(pth) as fh:
                    j = json.load(fh)
                if j.get("kernel", "").split("<")[0] == kernel_name.split("<")[0]:
                    return j, "profiles/%s_%s.json" % (rnd, name)
        return None, None

    # HBM traffic per launch: only from a committed PMC pass of this kernel on this workload (tools/pmc.sh)
    traffic, traffic_src = None, None
    tj, tsrc = committed("traffic")
    if tj is not None and args.workload == "c3" and args.precision == "f32" and snr is None:
        traffic = round(tj["hbm_bytes_per_input_sample"] * S * N / avg_kernel_s / 1e9, 1)
        traffic_src = tsrc + " (separate rocprofv3 --pmc passes of this kernel; bytes per input sample x this run's rate, not counters of this run)"

    # the ceiling that actually binds: vector instruction issue.  The instruction mix is a committed PMC profile of this
    # kernel (like the traffic figure); the rate is this run's.
    issue = None
    priced = None
    ij, isrc = committed("issue")
    clk = clock_ghz if clock_ghz else CLOCK_GHZ
    clk_note = ("measured in this run: one-wave probe, delta s_memtime / delta s_memrealtime x 100 MHz over extra steps of the same work "
                "behind the timed region") if clock_ghz else "NOT measured in this run: the part's maximum"
    # (the committed instruction mix is config #3's -- Bell-202, whole 64-stream groups; other workloads, narrow groups
    # and the small-batch kernel issue a different mix per workgroup, so the two issue ceilings are only emitted where the profile
    # applies and are left null elsewhere, as `traffic` already is)
    if ij is not None and not (args.workload == "c3" and args.precision == "f32" and snr is None and (lanes_main in (None, 64))):
        ij = None
    if ij is not None:
        ns = avg_kernel_s / N * 1e9
        groups = (S + 63) // 64
        valu_per_s = ij["insts_per_group_sample"]["valu"] * groups * N / avg_kernel_s
        peak = SIMDS * clk * 1e9 / 2.0
        issue = {"bound": "valu_issue", "achieved": round(valu_per_s / 1e9, 1), "peak": round(peak / 1e9, 1), "unit": "Ginst/s",
                 "frac": round(valu_per_s / peak, 4),
                 # (tools/valu_probe has four waves retire a full-rate instruction per 1.74 cycles, not 2.0)
                 "frac_probe": round(valu_per_s / (SIMDS * clk * 1e9 / 1.74), 4),
                 "frac_probe_definition": "the same against one wave64 vector instruction per 1.74 cycles per SIMD (tools/valu_probe, four waves per SIMD)",
                 "clock_ghz_measured": round(clock_ghz, 3) if clock_ghz else None,
                 "clock_note": clk_note,
                 "insts_per_group_sample": ij["insts_per_group_sample"],
                 "measured_ns_per_sample": round(ns, 1),
                 "peak_definition": "%d SIMD-32 x one wave64 vector instruction per 2 cycles at %.3f GHz" % (SIMDS, clk),
                 "source": isrc + " (rocprofv3 --pmc SQ_INSTS_* pass of this kernel; instructions per 64-stream group and input "
                                  "sample x this run's rate)"}
        pc = ij.get("class_priced_cycles_per_group_sample")
        if pc:
            # SIMD cycles the vector + scalar work of one group-sample is priced at (tools/isa_classes.py's classes: full rate 2,
            # half rate 4, transcendental 8, scalar 2 cycles) against the SIMD cycles one group-sample may take at this rate
            avail = ns * clk * SIMDS / groups
            priced = {"bound": "valu_class_priced", "achieved": round(pc, 1), "peak": round(avail, 1),
                      "unit": "SIMD cycles per group-sample (priced / available)", "frac": round(pc / avail, 4),
                      "frac_probe": round(pc * (1.74 / 2.0) / avail, 4),
                      "source": ij.get("class_priced_source", isrc)}
    hbm_frac = achieved / HBM_PEAK_GBS
    fr = {"hbm": hbm_frac, "valu_issue": issue["frac"] if issue else 0.0, "valu_class_priced": priced["frac"] if priced else 0.0}
    binding = max(fr, key=lambda k_: fr[k_])

    if rank == 0:
        line = {
            "metric": "Msamples/s demodulated (fused I/Q demod kernel, inputs resident in HBM)",
            "value": round(value, 1), "unit": "Msamples/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 3),
            "higher_is_better": True, "scaling": scaling, "vs_baseline": None,
            "dtype": args.precision, "data": "dry-run: no GPU, stand-in engine (launcher test)" if dry else "synthetic",
            "config": {
                "workload": "BASELINE config #%s: %d streams%s x %d samples (%.2f s) %s, back-to-back %d-byte "
                            "frames%s" % (
                                wl["num"], total_streams if strong_only else S,
                                " in total" if strong_only else "/GPU", N, N / sr, wl["desc"], wl["payload"],
                                "" if wl.get("roundtrip") else ", random lead-in and amplitude"),
                "lead_max_samples": args.lead_max if args.lead_max is not None else 10 * spb,
                "streams_per_gpu": S, "total_streams": total_streams if strong_only else streams_all,
                "ranks_reported": ranks_reported, "samples_per_stream": N, "row_pitch_floats": pitch,
                "resident_input_GB_per_gpu": round(S * pitch * 4 / 1e9, 2),
                "parallelism": "streams sharded across %d GPU(s) (%s scaling), no collective" % (world, scaling),
                "decoded_bytes_first_pass_rank0": decoded,
                **({"strong_scaling": strong} if strong is not None else {}),
                **({"c5_quality": c5q} if c5q is not None else {}),
                **side,
            },
            "roofline": {
                "bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic, "traffic_source": traffic_src,
                "kernel": kernel_name, "kernel_mixed_in_timed_region": (kernel_first != kernel_name) if kernel_first is not None else None,
                "streams_per_workgroup": lanes_main,
                "avg_kernel_ms": round(avg_kernel_s * 1e3, 4), "launches": n_launch,
                "algorithmic_bytes_per_launch": alg_bytes_per_launch,
                "binding_bound": binding,
                "valu_issue": issue,
                "valu_class_priced": priced,
                "binding_note": "the kernel is bound by SIMD time -- vector instruction issue (half-rate and transcendental "
                                "classes included) plus the cycles every branch / LDS / memory instruction costs its wave -- "
                                "not by HBM (DESIGN.md section 5): `frac` is the HBM fraction BASELINE.json's metric asks "
                                "for, `valu_issue.frac` is the same run's vector instructions against the SIMDs' issue peak",
            },
            "cpu_baseline": cpu_obj,
        }
        f64 = side.get("f64_parity_path")
        if args.precision == "f64":
            line["exact"] = {"dtype": "f64", "value": line["value"], "unit": "Msamples/s", "frac": round(achieved / HBM_PEAK_GBS, 4),
                             "note": "this run IS the exact path"}
        elif f64 and "Msamples_per_s" in f64:
            # the guaranteed-bit-exact number next to the fp32 headline (fp32 byte-exactness is a measured rate)
            line["exact"] = {"dtype": "f64", "value": f64["Msamples_per_s"], "unit": "Msamples/s", "frac": f64["frac_of_hbm_peak"],
                             "kernel": f64["kernel"], "streams": f64["streams"], "samples_per_stream": f64["samples_per_stream"],
                             "streams_checked": f64["streams_checked"], "streams_byte_identical": f64["streams_byte_identical"],
                             "note": "fp64 engine (the reference's operations in the reference's order) on the same resident batch at full "
                                     "length, kernel time from HIP events; bytes of a strided sample compared with the oracle in this run"}
        print(json.dumps(line), flush=True)
    eng.close()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    if not parity_ok:
        sys.exit(3)


def main():
    argv = sys.argv[1:]
    ap = build_parser()
    args = ap.parse_args(argv)
    check_args(ap, args)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args, argv))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        args.gpus = world
    if args.workload == "mod":
        worker_mod(args)
    else:
        worker(args)


if __name__ == "__main__":
    main()
