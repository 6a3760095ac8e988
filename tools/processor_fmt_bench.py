"""The streaming quantum in the capture formats (include/fskhip_next.h: fskhip_processor_process_fmt_host / _device) at DESIGN f1's size:
262 144 streams, Bell 202, quanta of 128 and 160 samples, one process, one MI355X.  Median of --reps after 2 warm-ups.

(a) host call, PCIe-inclusive, page-locked memory (fskhip_host_alloc): fskhip_processor_process_host on floats is the comparator, timed in
    the same run; then fskhip_processor_process_fmt_host with S16 and mu-law on both sides, stream-major and as interleaved frames.  Every
    case is a processor of its own with a modulation pending on every stream, fed the same quantum (a stretch of a modulated frame,
    quantised to the format; the float call gets the mu-law case's decoded values).  Wall clock around the synchronous call.  The
    expectation to check against the float call is PCIe-bound: towards 2 x for S16 and 4 x for G.711, until launch latency takes over.

(b) kernels alone, HIP events on the null stream, device buffers, TX only: the fused format-writing io kernel (one launch) against the
    pair it replaces -- the float io kernel followed by egress_kernel -- for the same shapes in the same run.  The pair is timed twice
    (pair_a, pair_b): their difference is the run's own spread, the margin within which "not slower" is to be read.

usage: python tools/processor_fmt_bench.py [--reps 7] [--out profiles/processor_fmt_bench.jsonl] [--streams 262144] [--parts host,kernel]"""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

from ingest_bench import BELL, WARMUP, Hip, _stats  # noqa: E402
import samples_ref as sr  # noqa: E402

QUANTA = (128, 160)
CASES = (("s16", "stream"), ("s16", "sample"), ("mulaw", "stream"), ("mulaw", "sample"))
PAYLOAD = 100       # bytes pending on every stream: 41 600 samples of signal, more than any timed series consumes


def pending(wm, eng, S):
    """a processor with a modulation of PAYLOAD bytes pending on every stream"""
    proc = wm.FSKProcessorBatch(eng, clear_rx_on_tx_complete=True)
    proc.modulate([bytes((7 * i + 3) & 0xFF for i in range(PAYLOAD))] * S)
    return proc


def quantum(wm, q):
    """q samples out of the middle of a modulated frame, float32"""
    eng = wm.FSKEngine(1, BELL)
    sig = np.asarray(eng.modulate_data([bytes(range(32))])[0], np.float32)
    eng.close()
    return sig[4000:4000 + q].copy()


def host_rows(a, wm, emit):
    from webaudio_modem_amd import _lib
    L = _lib.lib()
    S = a.streams
    eng = wm.FSKEngine(S, BELL)
    for q in QUANTA:
        row = quantum(wm, q)

        def timed_case(call):
            proc = pending(wm, eng, S)
            ms = []
            for r in range(a.reps + WARMUP):
                t0 = time.perf_counter()
                _lib.check(call(proc))
                t1 = time.perf_counter()
                if r >= WARMUP:
                    ms.append((t1 - t0) * 1e3)
            proc.close()
            return ms

        x = wm.pinned_empty((S, q), np.float32)
        x[:] = sr.decode(sr.encode(row, "mulaw"), "mulaw")
        y = wm.pinned_empty((S, q), np.float32)
        ms = timed_case(lambda p: L.fskhip_processor_process_host(p._h, x.ctypes.data, q, q, y.ctypes.data, q, q, p.flags))
        base = float(np.median(ms))
        emit(dict(part="host", call="fskhip_processor_process_host", format="f32", layout="stream", streams=S, quantum=q, bytes_per_sample=4,
                  link_mb_per_call=round(2 * S * q * 4 / 1e6, 1), x_float_call=1.0, **_stats(ms)))
        del x, y
        for fmt, layout in CASES:
            code, lay, dtype = sr.FORMATS[fmt], sr.LAYOUTS[layout], sr.DTYPES[fmt]
            shape, pitch = ((S, q), q) if layout == "stream" else ((q, S), S)
            x, y = wm.pinned_empty(shape, dtype), wm.pinned_empty(shape, dtype)
            codes = sr.encode(row, fmt)
            x[:] = codes if layout == "stream" else codes[:, None]
            ms = timed_case(lambda p: L.fskhip_processor_process_fmt_host(p._h, x.ctypes.data, code, lay, q, pitch, y.ctypes.data, code, lay, q, pitch, p.flags))
            med = float(np.median(ms))
            esz = np.dtype(dtype).itemsize
            emit(dict(part="host", call="fskhip_processor_process_fmt_host", format=fmt, layout=layout, streams=S, quantum=q, bytes_per_sample=esz,
                      link_mb_per_call=round(2 * S * q * esz / 1e6, 1), x_float_call=round(base / med, 3), **_stats(ms)))
            del x, y
    eng.close()


def kernel_rows(a, wm, emit):
    hip = Hip()
    S = a.streams
    eng = wm.FSKEngine(S, BELL)
    qmax = max(QUANTA)
    d_float = eng.device_malloc(S * qmax * 4)
    d_out = eng.device_malloc(S * qmax * 4)
    for q in QUANTA:
        for fmt, layout in CASES:
            pitch = q if layout == "stream" else S

            def series(step):
                proc = pending(wm, eng, S)
                ms = hip.timed(lambda: step(proc), a.reps)
                proc.close()
                return ms

            def pair(p):
                p.process_device(None, 0, 0, d_float, q, q, stream=None, flags=0)
                wm.egress_device(d_float, q, None, S, q, fmt, layout, d_out, pitch)

            def fused(p):
                p.process_samples_device(None, "f32", "stream", 0, 0, d_out, fmt, layout, q, pitch, stream=None, flags=0)

            pair_a, fused_ms, pair_b = series(pair), series(fused), series(pair)
            ma, mf, mb = (float(np.median(m)) for m in (pair_a, fused_ms, pair_b))
            emit(dict(part="kernel", format=fmt, layout=layout, streams=S, quantum=q,
                      pair="processor_io_kernel + egress_kernel", fused="processor_io_fmt_kernel",
                      pair_a=_stats(pair_a), pair_b=_stats(pair_b), fused_ms=_stats(fused_ms),
                      pair_spread=round(abs(ma - mb) / min(ma, mb), 4), fused_over_pair=round(mf / min(ma, mb), 4)))
    eng.device_free(d_float)
    eng.device_free(d_out)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--streams", type=int, default=262144)
    ap.add_argument("--parts", default="kernel,host")
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
    if "host" in a.parts:
        host_rows(a, wm, emit)


if __name__ == "__main__":
    main()
