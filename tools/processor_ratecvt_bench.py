"""The streaming quantum at 44.1 kHz (include/fskhip_next.h: fskhip_processor_process_ratecvt_host / _device): 262 144 streams, Bell 202
at 48 kHz between a CaptureConverter (160 / 147) and a PlaybackConverter (147 / 160) of the default design (2 561 taps), quanta of 147
and 441 samples at 44.1 kHz (160 and 480 engine samples), S16 and mu-law, stream-major and as interleaved frames, one process, one
MI355X.  Median of --reps after 2 warm-ups.  Every step -- one quantum length of one part -- is a process of its own under its own time
limit, and appends its rows to --out.

(a) kernels alone, HIP events on the null stream, device buffers, TX only: the fused kernel (processor_io_ratecvt_kernel, one launch)
    against the pair it replaces -- processor_io_kernel into a float tile, then ratecvt_playback_kernel -- for the same shapes in the
    same run.  The pair is timed twice (pair_a, pair_b): their difference is the run's own spread.  `faster_than_pair`: the fused
    kernel's median is below the pair's faster median by more than that spread.  Only the shapes the call dispatches to the fused
    kernel are compared (csrc/fsk_processor_rate_plan.h: stream-major); interleaved frames run the pair itself, and their row holds
    the call's time beside the pair's (`path`: which of the two the call took).

(b) host calls, PCIe-inclusive, page-locked memory, wall clock around the synchronous calls, both sides in every call:
    fskhip_processor_process_ratecvt_host; fskhip_processor_process_fmt_host at 48 kHz in the same format (160 / 147 of the bytes and
    no filters); and the chain of three calls the new one stands for -- fskhip_ratecvt_capture_host, fskhip_processor_process_host on
    the floats, fskhip_ratecvt_playback_host -- which carries the floats over the link both ways.

usage: python tools/processor_ratecvt_bench.py [--reps 7] [--out profiles/processor_ratecvt_bench.jsonl] [--streams 262144] [--parts kernel,host]"""
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

QUANTA = (147, 441)
OUTER, ENGINE = 44100, 48000
UP, DOWN = 147, 160          # the playback converter's; the capture converter's are the other way round
TAPS = 16 * DOWN + 1
STEP_SECONDS = 400


def tx_path(layout):
    """what fskhip_processor_process_ratecvt_* runs for the default design: processor_ratecvt_plan's choice (it fits; fused where
    stream-major)"""
    return "fused" if layout == "stream" else "pair"


def kernel_rows(a, wm, q, emit):
    hip = Hip()
    S = a.streams
    n_eng = q // UP * DOWN
    eng = wm.FSKEngine(S, BELL)
    d_float = eng.device_malloc(S * n_eng * 4)
    d_out = eng.device_malloc(S * q * 2)
    for fmt, layout in CASES:
        pitch = q if layout == "stream" else S

        def series(step):
            proc, play = pending(wm, eng, S), wm.PlaybackConverter(ENGINE, OUTER, S)
            ms = hip.timed(lambda: step(proc, play), a.reps)
            play.close()
            proc.close()
            return ms

        def pair(p, play):
            p.process_device(None, 0, 0, d_float, n_eng, n_eng, stream=None, flags=0)
            play.process_device(d_float, n_eng, n_eng, None, d_out, fmt, layout, pitch)

        def fused(p, play):
            p.process_samples_at_device(None, fmt, layout, 0, 0, None, d_out, fmt, layout, q, pitch, play, stream=None, flags=0)

        pair_a, call_ms, pair_b = series(pair), series(fused), series(pair)
        ma, mf, mb = (float(np.median(m)) for m in (pair_a, call_ms, pair_b))
        row = dict(part="kernel", format=fmt, layout=layout, streams=S, quantum=q, engine_samples=n_eng, up=UP, down=DOWN, taps=TAPS, path=tx_path(layout),
                   pair="processor_io_kernel + ratecvt_playback_kernel", pair_a=_stats(pair_a), pair_b=_stats(pair_b),
                   pair_spread_ms=round(abs(ma - mb), 4))
        if tx_path(layout) == "fused":
            row.update(fused="processor_io_ratecvt_kernel", fused_ms=_stats(call_ms), fused_minus_pair_ms=round(mf - 0.5 * (ma + mb), 4),
                       fused_over_pair=round(mf / (0.5 * (ma + mb)), 4), faster_than_pair=bool(mf < min(ma, mb) - abs(ma - mb)))
        else:
            row.update(call_ms=_stats(call_ms))       # the same two launches through fskhip_processor_process_ratecvt_device
        emit(row)
    eng.device_free(d_float)
    eng.device_free(d_out)
    eng.close()


def host_rows(a, wm, q, emit):
    from webaudio_modem_amd import _lib
    L = _lib.lib()
    S = a.streams
    n_eng = q // UP * DOWN
    eng = wm.FSKEngine(S, BELL)
    fin, fout = wm.pinned_empty((S, n_eng), np.float32), wm.pinned_empty((S, n_eng), np.float32)
    for fmt, layout in CASES:
        code, lay, dtype = sr.FORMATS[fmt], sr.LAYOUTS[layout], sr.DTYPES[fmt]
        esz = np.dtype(dtype).itemsize

        def timed_case(n, call, handles):
            proc = pending(wm, eng, S)
            hs = [wm.CaptureConverter(OUTER, ENGINE, S), wm.PlaybackConverter(ENGINE, OUTER, S)] if handles else []
            shape, pitch = ((S, n), n) if layout == "stream" else ((n, S), S)
            x, y = wm.pinned_empty(shape, dtype), wm.pinned_empty(shape, dtype)
            x[:] = sr.silence(fmt)
            ms = []
            for r in range(a.reps + WARMUP):
                t0 = time.perf_counter()
                call(proc, hs, x, y, n, pitch)
                t1 = time.perf_counter()
                if r >= WARMUP:
                    ms.append((t1 - t0) * 1e3)
            for h in hs:
                h.close()
            proc.close()
            return ms

        def wide_call(p, hs, x, y, n, pitch):
            _lib.check(L.fskhip_processor_process_fmt_host(p._h, x.ctypes.data, code, lay, n, pitch, y.ctypes.data, code, lay, n, pitch, p.flags))

        def cvt_call(p, hs, x, y, n, pitch):
            _lib.check(L.fskhip_processor_process_ratecvt_host(p._h, hs[0]._h, hs[1]._h, x.ctypes.data, code, lay, n, pitch, y.ctypes.data, code, lay, n, pitch,
                                                               p.flags))

        def chain_call(p, hs, x, y, n, pitch):
            _lib.check(L.fskhip_ratecvt_capture_host(hs[0]._h, x.ctypes.data, code, lay, n, pitch, fin.ctypes.data, n_eng))
            _lib.check(L.fskhip_processor_process_host(p._h, fin.ctypes.data, n_eng, n_eng, fout.ctypes.data, n_eng, n_eng, p.flags))
            _lib.check(L.fskhip_ratecvt_playback_host(hs[1]._h, fout.ctypes.data, n_eng, n_eng, None, y.ctypes.data, code, lay, pitch))

        wide, cvt, chain = timed_case(n_eng, wide_call, False), timed_case(q, cvt_call, True), timed_case(q, chain_call, True)
        emit(dict(part="host", format=fmt, layout=layout, streams=S, quantum=q, engine_samples=n_eng, up=UP, down=DOWN, taps=TAPS, tx_path=tx_path(layout),
                  ratecvt_call="fskhip_processor_process_ratecvt_host", ratecvt_ms=_stats(cvt), ratecvt_link_mb=round(2 * S * q * esz / 1e6, 1),
                  wide_call="fskhip_processor_process_fmt_host at 48 kHz", wide_ms=_stats(wide), wide_link_mb=round(2 * S * n_eng * esz / 1e6, 1),
                  chain_call="fskhip_ratecvt_capture_host + fskhip_processor_process_host + fskhip_ratecvt_playback_host", chain_ms=_stats(chain),
                  chain_link_mb=round(2 * S * (q * esz + n_eng * 4) / 1e6, 1),
                  ratecvt_over_wide=round(float(np.median(cvt)) / float(np.median(wide)), 3),
                  chain_over_ratecvt=round(float(np.median(chain)) / float(np.median(cvt)), 3)))
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "processor_ratecvt_bench.jsonl"))
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
