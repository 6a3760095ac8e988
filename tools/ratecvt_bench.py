"""Rate conversion by 160 / 147 and 147 / 160 at full size (include/fskhip_next.h: fskhip_ratecvt_capture_device / _playback_device),
one process, one MI355X.

65 536 streams x 44 100 inputs at 44.1 kHz (capture; 48 000 outputs) and x 48 000 inputs at 48 kHz (playback; 44 100 outputs), the
default designs' 2 561 taps, s16 and mu-law, both layouts, fp32 and fp64; device buffers of zeros (no kernel's time here depends
on the values), HIP events on the null stream, median of --reps after 2 warm-ups.  In the same run, for comparison:
  * a device-to-device hipMemcpy of the 48 kHz float tile;
  * resample_up_kernel at L = 6 with the default design's 97 taps, 8 000 inputs -> the same 48 000 outputs per stream: 16-17 taps
    per output as here (2 561 / 160 = 16-17, 2 561 / 147 = 17-18), so the time per output sample is comparable.
A row gives the kernel's time, its ratio to the copy and its time per output sample; nothing is asserted.

usage: python tools/ratecvt_bench.py [--reps 7] [--out profiles/ratecvt_bench.jsonl] [--streams 65536] [--periods 300]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from ingest_bench import Hip, _stats  # noqa: E402

ESZ = {"s16": 2, "mulaw": 1}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--streams", type=int, default=65536)
    ap.add_argument("--periods", type=int, default=300, help="periods of 147 samples at 44.1 kHz = 160 at 48 kHz per stream (300: one second)")
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

    hip = Hip()
    S = a.streams
    n_lo, n_hi = a.periods * 147, a.periods * 160                                 # samples per stream at 44.1 / 48 kHz
    n8 = n_hi // 6                                                                # ... and at 8 kHz, for the integer interpolator
    eng = wm.FSKEngine(1, {})
    wide_bytes = S * n_hi * 4
    d_a, d_b = eng.device_malloc(wide_bytes), eng.device_malloc(wide_bytes)       # two float tiles at 48 kHz
    d_n = eng.device_malloc(S * n_lo * 2)                                         # narrow samples, up to 44.1 kHz s16
    for p, b in ((d_a, wide_bytes), (d_b, wide_bytes), (d_n, S * n_lo * 2)):
        hip.check(hip.L.hipMemset(C.c_void_p(p), 0, C.c_size_t(b)), "hipMemset")
    ms = hip.timed(lambda: hip.check(hip.L.hipMemcpyDtoD(C.c_void_p(d_b), C.c_void_p(d_a), C.c_size_t(wide_bytes)), "hipMemcpyDtoD"), a.reps)
    copy = float(np.median(ms))
    emit(dict(call="hipMemcpyDtoD", streams=S, samples=n_hi, bytes_moved=2 * wide_bytes, gb_per_s=round(2 * wide_bytes / copy / 1e6, 1), **_stats(ms)))

    for pname, prec in (("fp32", wm.PRECISION_F32), ("fp64", wm.PRECISION_F64)):
        cap, play = wm.CaptureConverter(44100, 48000, S, precision=prec), wm.PlaybackConverter(48000, 44100, S, precision=prec)
        up = wm.Upsampler(6, S, precision=prec)
        for fmt in ("s16", "mulaw"):
            for layout in ("stream", "sample"):
                ms = hip.timed(lambda: up.process_device(d_n, fmt, layout, n8, n8 if layout == "stream" else S, d_b, n_hi), a.reps)
                up_ms = float(np.median(ms))
                emit(dict(call="fskhip_resampler_up_device", precision=pname, format=fmt, layout=layout, streams=S, samples_in=n8, samples_out=n_hi, factor=6,
                          taps=len(up.taps), ps_per_output=round(up_ms * 1e9 / (S * n_hi), 3), x_dtod_time=round(up_ms / copy, 3), **_stats(ms)))
                ms = hip.timed(lambda: cap.process_device(d_n, fmt, layout, n_lo, n_lo if layout == "stream" else S, d_b, n_hi), a.reps)
                t = float(np.median(ms))
                moved = S * n_lo * ESZ[fmt] + wide_bytes
                emit(dict(call="fskhip_ratecvt_capture_device", precision=pname, format=fmt, layout=layout, streams=S, samples_in=n_lo, samples_out=n_hi, up=cap.up,
                          down=cap.down, taps=len(cap.taps), ps_per_output=round(t * 1e9 / (S * n_hi), 3), bytes_moved=moved, gb_per_s=round(moved / t / 1e6, 1),
                          x_dtod_time=round(t / copy, 3), x_resample_up_time_per_output=round(t / up_ms, 3), **_stats(ms)))
                ms = hip.timed(lambda: play.process_device(d_a, n_hi, n_hi, None, d_n, fmt, layout, n_lo if layout == "stream" else S), a.reps)
                t = float(np.median(ms))
                emit(dict(call="fskhip_ratecvt_playback_device", precision=pname, format=fmt, layout=layout, streams=S, samples_in=n_hi, samples_out=n_lo, up=play.up,
                          down=play.down, taps=len(play.taps), ps_per_output=round(t * 1e9 / (S * n_lo), 3), bytes_moved=moved, gb_per_s=round(moved / t / 1e6, 1),
                          x_dtod_time=round(t / copy, 3), x_resample_up_time_per_output=round((t / n_lo) / (up_ms / n_hi), 3), **_stats(ms)))
        for h in (cap, play, up):
            h.close()
    for p in (d_a, d_b, d_n):
        eng.device_free(p)
    eng.close()


if __name__ == "__main__":
    main()
