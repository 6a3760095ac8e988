"""Capture formats at full size (include/fskhip.h: fskhip_demodulate_host_fmt, fskhip_ingest_device), one process, one MI355X.

PCIe-inclusive: the committed PCIe-inclusive shape -- 16 384 streams x 48 000 samples, Bell 202, one synthetic signal (frames behind
staggered lead-ins) quantised on the host to each format -- from page-locked memory (fskhip_host_alloc).  fskhip_demodulate_host on
the floats is the comparator, timed in the same run; then fskhip_demodulate_host_fmt for S16, MULAW and ALAW stream-major and S16
sample-major.  Wall clock around the synchronous call (it ends in a stream synchronise), median of --reps after 2 warm-ups, every
case on an engine of its own; Gsamples/s and the ratio to the float call.

Kernel alone: fskhip_ingest_device at 65 536 x 48 000 for every format x layout, device buffers, HIP events around one launch, the
same median; GB/s of bytes read plus bytes written.  The comparator is a device-to-device hipMemcpy of the same OUTPUT bytes in the
same run (it reads and writes them: its GB/s counts both).

usage: python tools/ingest_bench.py [--reps 7] [--out profiles/ingest_bench.jsonl] [--host-streams 16384] [--kernel-streams 65536] [--samples 48000]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

BELL = dict(baudRate=1200, markFrequency=1200, spaceFrequency=2200)
WARMUP = 2


def _stats(ms):
    return dict(ms_median=round(float(np.median(ms)), 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4))


class Hip:
    """the few runtime calls the C ABI has no wrapper for: events and a device-to-device copy"""

    def __init__(self):
        self.L = C.CDLL("libamdhip64.so")

    def check(self, rc, what):
        if rc != 0:
            raise RuntimeError("%s failed: hipError %d" % (what, rc))

    def event(self):
        ev = C.c_void_p()
        self.check(self.L.hipEventCreate(C.byref(ev)), "hipEventCreate")
        return ev

    def timed(self, fn, reps):
        """milliseconds between two events on the null stream around fn(), reps times after the warm-ups"""
        a, b = self.event(), self.event()
        ms = []
        for r in range(reps + WARMUP):
            self.check(self.L.hipEventRecord(a, None), "hipEventRecord")
            fn()
            self.check(self.L.hipEventRecord(b, None), "hipEventRecord")
            self.check(self.L.hipEventSynchronize(b), "hipEventSynchronize")
            t = C.c_float()
            self.check(self.L.hipEventElapsedTime(C.byref(t), a, b), "hipEventElapsedTime")
            if r >= WARMUP:
                ms.append(t.value)
        self.L.hipEventDestroy(a)
        self.L.hipEventDestroy(b)
        return ms


def host_rows(a, wm, emit):
    import samples_ref as ir
    from webaudio_modem_amd import _lib
    L = _lib.lib()
    S, N = a.host_streams, a.samples
    gen = wm.FSKEngine(S, BELL)
    d = gen.device_malloc(S * N * 4)
    gen.synth_device(d, N, N, 100, 67001, 400, 0.1, 1.0)
    gen.synchronize()
    floats = wm.pinned_empty((S, N), np.float32)
    gen.d2h(floats, d)
    gen.device_free(d)
    opitch = gen.max_bytes(N)
    gen.close()
    out, counts, eod = np.zeros((S, opitch), np.uint8), np.zeros(S, np.uint32), np.zeros(S, np.uint32)

    def timed_case(call):
        eng = wm.FSKEngine(S, BELL)
        ms = []
        for r in range(a.reps + WARMUP):
            t0 = time.perf_counter()
            _lib.check(call(eng))
            t1 = time.perf_counter()
            if r >= WARMUP:
                ms.append((t1 - t0) * 1e3)
        total = int(counts.sum())
        eng.close()
        return ms, total

    ms, nbytes = timed_case(lambda e: L.fskhip_demodulate_host(e._h, floats.ctypes.data, N, N, out.ctypes.data, opitch, counts.ctypes.data, eod.ctypes.data, 0))
    base = float(np.median(ms))
    emit(dict(part="pcie", call="fskhip_demodulate_host", format="f32", layout="stream", streams=S, samples=N, bytes_per_sample=4,
              gsamples_per_s=round(S * N / base / 1e6, 3), input_gb_per_s=round(S * N * 4 / base / 1e6, 2), x_float_call=1.0, decoded_bytes=nbytes, **_stats(ms)))
    # the narrow forms of the same signal: int16 by rounding, G.711 through a table over the int16 values (the nearest code of each)
    s16 = wm.pinned_empty((S, N), np.int16)
    for r0 in range(0, S, 1024):
        s16[r0:r0 + 1024] = ir.quantise(floats[r0:r0 + 1024], "s16")
    s16_values = np.arange(-32768, 32768, dtype=np.int32).astype(np.int16)
    narrow8 = wm.pinned_empty((S, N), np.uint8)
    cases = [("s16", "stream", s16, N)]
    for fmt in ("mulaw", "alaw"):
        cases.append((fmt, "stream", fmt, N))
    cases.append(("s16", "sample", "transpose", S))
    for fmt, layout, src, pitch in cases:
        if isinstance(src, str) and src == "transpose":
            frames = wm.pinned_empty((N, S), np.int16)
            for r0 in range(0, S, 1024):
                frames[:, r0:r0 + 1024] = s16[r0:r0 + 1024].T
            arr = frames
        elif isinstance(src, str):
            table = ir.quantise(ir.decode(s16_values, "s16"), fmt)
            for r0 in range(0, S, 1024):
                narrow8[r0:r0 + 1024] = table[s16[r0:r0 + 1024].astype(np.int32) + 32768]
            arr = narrow8
        else:
            arr = src
        code, lay = ir.FORMATS[fmt], ir.LAYOUTS[layout]
        ms, nb = timed_case(lambda e: L.fskhip_demodulate_host_fmt(e._h, arr.ctypes.data, code, lay, N, pitch, out.ctypes.data, opitch, counts.ctypes.data,
                                                                    eod.ctypes.data, 0))
        med = float(np.median(ms))
        emit(dict(part="pcie", call="fskhip_demodulate_host_fmt", format=fmt, layout=layout, streams=S, samples=N, bytes_per_sample=arr.dtype.itemsize,
                  gsamples_per_s=round(S * N / med / 1e6, 3), input_gb_per_s=round(S * N * arr.dtype.itemsize / med / 1e6, 2),
                  x_float_call=round(base / med, 3), decoded_bytes=nb, **_stats(ms)))


def kernel_rows(a, wm, emit):
    import samples_ref as ir
    hip = Hip()
    S, N = a.kernel_streams, a.samples
    eng = wm.FSKEngine(1, {})
    out_bytes = S * N * 4
    d_src = eng.device_malloc(out_bytes)          # large enough for every format; zeros (the kernels' time does not depend on the values)
    d_dst = eng.device_malloc(out_bytes)
    hip.check(hip.L.hipMemset(C.c_void_p(d_src), 0, C.c_size_t(out_bytes)), "hipMemset")
    hip.check(hip.L.hipMemset(C.c_void_p(d_dst), 0, C.c_size_t(out_bytes)), "hipMemset")
    ms = hip.timed(lambda: hip.check(hip.L.hipMemcpyDtoD(C.c_void_p(d_dst), C.c_void_p(d_src), C.c_size_t(out_bytes)), "hipMemcpyDtoD"), a.reps)
    copy = float(np.median(ms))
    emit(dict(part="kernel", call="hipMemcpyDtoD", streams=S, samples=N, bytes_moved=2 * out_bytes, gb_per_s=round(2 * out_bytes / copy / 1e6, 1), **_stats(ms)))
    for fmt in ("f32", "s16", "mulaw", "alaw"):
        esz = np.dtype(ir.DTYPES[fmt]).itemsize
        for layout in ("stream", "sample"):
            pitch = N if layout == "stream" else S
            ms = hip.timed(lambda: wm.ingest_device(d_src, fmt, layout, S, N, pitch, d_dst, N), a.reps)
            med = float(np.median(ms))
            moved = S * N * (esz + 4)
            emit(dict(part="kernel", call="fskhip_ingest_device", format=fmt, layout=layout, streams=S, samples=N, bytes_moved=moved,
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
