"""Playback formats at full size (include/fskhip.h: fskhip_modulate_host_fmt, fskhip_egress_device), one process, one MI355X.

PCIe-inclusive: 16 384 streams x 48 000 samples, Bell 202, one 115-byte payload per stream (47 680 samples of signal, silence behind
it), into page-locked memory (fskhip_host_alloc).  fskhip_modulate_host on floats is the comparator, timed in the same run; then
fskhip_modulate_host_fmt for S16, MULAW and ALAW stream-major and S16 sample-major.  Wall clock around the synchronous call (it ends
in a stream synchronise), median of --reps after 2 warm-ups, every case on an engine of its own; Gsamples/s and the ratio to the
float call.  The expectation to be checked is PCIe-bound: S16 towards 2 x, G.711 towards 4 x.

Kernel alone: fskhip_egress_device at 65 536 x 48 000 for every format x layout, device buffers, no lengths array, HIP events around
one launch, the same median; GB/s of bytes read plus bytes written.  The comparator is a device-to-device hipMemcpy of the same INPUT
bytes in the same run (it reads and writes them: its GB/s counts both).

usage: python tools/egress_bench.py [--reps 7] [--out profiles/egress_bench.jsonl] [--host-streams 16384] [--kernel-streams 65536] [--samples 48000]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from ingest_bench import BELL, WARMUP, Hip, _stats  # noqa: E402

FORMATS = {"f32": (0, np.float32), "s16": (1, np.int16), "mulaw": (2, np.uint8), "alaw": (3, np.uint8)}
LAYOUTS = {"stream": 0, "sample": 1}


def host_rows(a, wm, emit):
    from webaudio_modem_amd import _lib
    from webaudio_modem_amd.engine import payload_args
    L = _lib.lib()
    S, N = a.host_streams, a.samples
    probe = wm.FSKEngine(1, BELL)
    n_bytes = 0
    while probe.modulated_length(n_bytes + 1) <= N:   # the longest payload whose signal fits
        n_bytes += 1
    probe.close()
    rng = np.random.default_rng(67001)
    pay, lens, ppitch = payload_args([rng.integers(0, 256, n_bytes, dtype=np.int32).astype(np.uint8).tobytes() for _ in range(S)])
    out_lens = np.zeros(S, np.uint32)

    def timed_case(call):
        eng = wm.FSKEngine(S, BELL)
        ms = []
        for r in range(a.reps + WARMUP):
            t0 = time.perf_counter()
            _lib.check(call(eng))
            t1 = time.perf_counter()
            if r >= WARMUP:
                ms.append((t1 - t0) * 1e3)
        eng.close()
        return ms

    floats = wm.pinned_empty((S, N), np.float32)
    ms = timed_case(lambda e: L.fskhip_modulate_host(e._h, pay.ctypes.data, lens.ctypes.data, ppitch, floats.ctypes.data, N, out_lens.ctypes.data))
    base = float(np.median(ms))
    emit(dict(part="pcie", call="fskhip_modulate_host", format="f32", layout="stream", streams=S, samples=N, payload_bytes=n_bytes, signal_samples=int(out_lens[0]),
              bytes_per_sample=4, gsamples_per_s=round(S * N / base / 1e6, 3), output_gb_per_s=round(S * N * 4 / base / 1e6, 2), x_float_call=1.0, **_stats(ms)))
    del floats
    for fmt, layout in (("s16", "stream"), ("mulaw", "stream"), ("alaw", "stream"), ("s16", "sample")):
        code, dtype = FORMATS[fmt]
        arr = wm.pinned_empty((S, N) if layout == "stream" else (N, S), dtype)
        pitch = N if layout == "stream" else S
        ms = timed_case(lambda e: L.fskhip_modulate_host_fmt(e._h, pay.ctypes.data, lens.ctypes.data, ppitch, code, LAYOUTS[layout], arr.ctypes.data, N, pitch,
                                                             out_lens.ctypes.data))
        med = float(np.median(ms))
        esz = np.dtype(dtype).itemsize
        emit(dict(part="pcie", call="fskhip_modulate_host_fmt", format=fmt, layout=layout, streams=S, samples=N, payload_bytes=n_bytes, signal_samples=int(out_lens[0]),
                  bytes_per_sample=esz, gsamples_per_s=round(S * N / med / 1e6, 3), output_gb_per_s=round(S * N * esz / med / 1e6, 2),
                  x_float_call=round(base / med, 3), **_stats(ms)))
        del arr


def kernel_rows(a, wm, emit):
    hip = Hip()
    S, N = a.kernel_streams, a.samples
    eng = wm.FSKEngine(1, {})
    in_bytes = S * N * 4
    d_src = eng.device_malloc(in_bytes)           # zeros (the kernels' time does not depend on the values)
    d_dst = eng.device_malloc(in_bytes)           # large enough for every format
    hip.check(hip.L.hipMemset(C.c_void_p(d_src), 0, C.c_size_t(in_bytes)), "hipMemset")
    hip.check(hip.L.hipMemset(C.c_void_p(d_dst), 0, C.c_size_t(in_bytes)), "hipMemset")
    ms = hip.timed(lambda: hip.check(hip.L.hipMemcpyDtoD(C.c_void_p(d_dst), C.c_void_p(d_src), C.c_size_t(in_bytes)), "hipMemcpyDtoD"), a.reps)
    copy = float(np.median(ms))
    emit(dict(part="kernel", call="hipMemcpyDtoD", streams=S, samples=N, bytes_moved=2 * in_bytes, gb_per_s=round(2 * in_bytes / copy / 1e6, 1), **_stats(ms)))
    for fmt, (_code, dtype) in FORMATS.items():
        esz = np.dtype(dtype).itemsize
        for layout in ("stream", "sample"):
            pitch = N if layout == "stream" else S
            ms = hip.timed(lambda: wm.egress_device(d_src, N, None, S, N, fmt, layout, d_dst, pitch), a.reps)
            med = float(np.median(ms))
            moved = S * N * (4 + esz)
            emit(dict(part="kernel", call="fskhip_egress_device", format=fmt, layout=layout, streams=S, samples=N, bytes_moved=moved,
                      gb_per_s=round(moved / med / 1e6, 1), gsamples_per_s=round(S * N / med / 1e6, 1), x_dtod_time=round(med / copy, 3), **_stats(ms)))
    eng.device_free(d_src)
    eng.device_free(d_dst)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--host-streams", type=int, default=16384)
    ap.add_argument("--kernel-streams", type=int, default=65536)
    ap.add_argument("--samples", type=int, default=48000)
    ap.add_argument("--parts", default="kernel,pcie")
    a = ap.parse_args()
    import webaudio_modem_amd as wm
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)
        if a.out:                                   # (rewritten after every row: a run that is cut short keeps what it measured)
            with open(a.out, "w") as fh:
                for r in rows:
                    fh.write(json.dumps(r) + "\n")

    if "kernel" in a.parts:
        kernel_rows(a, wm, emit)
    if "pcie" in a.parts:
        host_rows(a, wm, emit)


if __name__ == "__main__":
    main()
