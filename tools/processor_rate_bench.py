"""The streaming quantum at a trunk's low rate (include/fskhip_next.h: fskhip_processor_process_rate_host / _device): 262 144 streams,
Bell 202 at 48 kHz behind an 8 kHz trunk (factor 6, the default 97 taps), quanta of 80 and 160 low rate samples, S16 and mu-law,
stream-major and as interleaved frames, one process, one MI355X.  Median of --reps after 2 warm-ups.  Every step -- one quantum length of
one part -- is a process of its own under its own time limit, and appends its rows to --out.

(a) kernels alone, HIP events on the null stream, device buffers, TX only: the fused kernel (processor_io_rate_kernel, one launch)
    against the pair it replaces -- processor_io_kernel into a float tile, then resample_down_kernel -- for the same shapes in the same
    run.  The pair is timed twice (pair_a, pair_b): their difference is the run's own spread.  The one condition on the fused kernel:
    its median may not exceed the pair's by more than that spread (row field `within_spread`).  Only the shapes the call dispatches
    to the fused kernel are compared (csrc/fsk_processor_rate_plan.h: stream-major); interleaved frames run the pair itself, and
    their row holds the call's time beside the pair's (`path`: which of the two the call took).

(b) host call, PCIe-inclusive, page-locked memory, wall clock around the synchronous call: fskhip_processor_process_rate_host against
    fskhip_processor_process_fmt_host at 48 kHz in the same format, which moves six times the bytes.

usage: python tools/processor_rate_bench.py [--reps 7] [--out profiles/processor_rate_bench.jsonl] [--streams 262144] [--parts kernel,host]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from ingest_bench import BELL, WARMUP, Hip, _stats  # noqa: E402
from processor_fmt_bench import CASES, pending  # noqa: E402
import samples_ref as sr  # noqa: E402

QUANTA = (80, 160)
FACTOR = 6
STEP_SECONDS = 240


def tx_path(layout):
    """what fskhip_processor_process_rate_* runs for the default design at FACTOR: processor_rate_plan's choice (it fits; fused where
    stream-major)"""
    return "fused" if layout == "stream" else "pair"


def kernel_rows(a, wm, q, emit):
    hip = Hip()
    S = a.streams
    eng = wm.FSKEngine(S, BELL)
    tpitch = q * FACTOR
    d_float = eng.device_malloc(S * tpitch * 4)
    d_out = eng.device_malloc(S * q * 2)
    for fmt, layout in CASES:
        pitch = q if layout == "stream" else S

        def series(step):
            proc, dn = pending(wm, eng, S), wm.Downsampler(FACTOR, S)
            ms = hip.timed(lambda: step(proc, dn), a.reps)
            dn.close()
            proc.close()
            return ms

        def pair(p, dn):
            p.process_device(None, 0, 0, d_float, q * FACTOR, tpitch, stream=None, flags=0)
            dn.process_device(d_float, q * FACTOR, tpitch, None, d_out, fmt, layout, pitch)

        def fused(p, dn):
            p.process_samples_at_device(None, fmt, layout, 0, 0, None, d_out, fmt, layout, q, pitch, dn, stream=None, flags=0)

        pair_a, call_ms, pair_b = series(pair), series(fused), series(pair)
        ma, mf, mb = (float(np.median(m)) for m in (pair_a, call_ms, pair_b))
        row = dict(part="kernel", format=fmt, layout=layout, streams=S, quantum=q, factor=FACTOR, taps=16 * FACTOR + 1, path=tx_path(layout),
                   pair="processor_io_kernel + resample_down_kernel", pair_a=_stats(pair_a), pair_b=_stats(pair_b),
                   pair_spread_ms=round(abs(ma - mb), 4))
        if tx_path(layout) == "fused":
            row.update(fused="processor_io_rate_kernel", fused_ms=_stats(call_ms), fused_minus_pair_ms=round(mf - 0.5 * (ma + mb), 4),
                       fused_over_pair=round(mf / (0.5 * (ma + mb)), 4), within_spread=bool(mf <= max(ma, mb) + abs(ma - mb)))
        else:
            row.update(call_ms=_stats(call_ms))       # the same two launches through fskhip_processor_process_rate_device
        emit(row)
    eng.device_free(d_float)
    eng.device_free(d_out)
    eng.close()


def host_rows(a, wm, q, emit):
    from webaudio_modem_amd import _lib
    L = _lib.lib()
    S = a.streams
    eng = wm.FSKEngine(S, BELL)
    for fmt, layout in CASES:
        code, lay, dtype = sr.FORMATS[fmt], sr.LAYOUTS[layout], sr.DTYPES[fmt]
        esz = np.dtype(dtype).itemsize

        def timed_case(n, call, handles):
            proc = pending(wm, eng, S)
            hs = [wm.Upsampler(FACTOR, S), wm.Downsampler(FACTOR, S)] if handles else []
            shape, pitch = ((S, n), n) if layout == "stream" else ((n, S), S)
            x, y = wm.pinned_empty(shape, dtype), wm.pinned_empty(shape, dtype)
            x[:] = sr.silence(fmt)
            ms = []
            for r in range(a.reps + WARMUP):
                t0 = time.perf_counter()
                _lib.check(call(proc, hs, x, y, n, pitch))
                t1 = time.perf_counter()
                if r >= WARMUP:
                    ms.append((t1 - t0) * 1e3)
            for h in hs:
                h.close()
            proc.close()
            return ms

        wide = timed_case(q * FACTOR, lambda p, hs, x, y, n, pitch: L.fskhip_processor_process_fmt_host(
            p._h, x.ctypes.data, code, lay, n, pitch, y.ctypes.data, code, lay, n, pitch, p.flags), False)
        low = timed_case(q, lambda p, hs, x, y, n, pitch: L.fskhip_processor_process_rate_host(
            p._h, hs[0]._h, hs[1]._h, x.ctypes.data, code, lay, n, pitch, y.ctypes.data, code, lay, n, pitch, p.flags), True)
        emit(dict(part="host", format=fmt, layout=layout, streams=S, quantum=q, factor=FACTOR, tx_path=tx_path(layout),
                  rate_call="fskhip_processor_process_rate_host", rate_ms=_stats(low), rate_link_mb=round(2 * S * q * esz / 1e6, 1),
                  wide_call="fskhip_processor_process_fmt_host at 48 kHz", wide_ms=_stats(wide), wide_link_mb=round(2 * S * q * FACTOR * esz / 1e6, 1),
                  wide_over_rate=round(float(np.median(wide)) / float(np.median(low)), 3)))
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "processor_rate_bench.jsonl"))
    ap.add_argument("--streams", type=int, default=262144)
    ap.add_argument("--parts", default="kernel,host")
    ap.add_argument("--step", default=None, help="(internal) part:quantum of the one step this process runs")
    a = ap.parse_args()
    if a.step is None:
        open(a.out, "w").close()
        failed = 0
        for part in a.parts.split(","):
            for q in QUANTA:
                cmd = ["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--out", a.out,
                       "--streams", str(a.streams), "--step", "%s:%d" % (part, q)]
                rc = subprocess.call(cmd)
                if rc != 0:     # a step that failed or ran out of time ends the run: nothing more is started on the device
                    print("step %s:%d ended with status %d" % (part, q, rc), flush=True)
                    failed = rc
                    break
            if failed:
                break
        sys.exit(failed)
    import webaudio_modem_amd as wm
    part, q = a.step.split(":")

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        with open(a.out, "a") as fh:
            fh.write(line + "\n")

    {"kernel": kernel_rows, "host": host_rows}[part](a, wm, int(q), emit)


if __name__ == "__main__":
    main()
