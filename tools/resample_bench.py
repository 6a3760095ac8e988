"""Rate conversion at full size (include/fskhip_next.h: fskhip_resampler_up_device / _down_device), one process, one MI355X.

65 536 streams x 8 000 samples at the low rate, L = 6, the default design's 97 taps, mu-law and s16, both layouts, fp32 and fp64;
device buffers of zeros (no kernel's time here depends on the values), HIP events on the null stream, median of --reps after 2
warm-ups.  In the same run, for the same output:
  * what the tree offered before -- up: ingest_kernel on the zero-stuffed full rate input, then fir_kernel; down: fir_kernel, then
    egress_kernel on every sixth column (the float rows taken as [streams x 8 000][6] with one element each, which is the only way
    fskhip_egress_device strides a column, so stream-major only) -- each part and the pair;
  * a device-to-device hipMemcpy of the full rate float bytes.
A row gives the polyphase kernel's time, the pair's, and their ratio; nothing is asserted.

usage: python tools/resample_bench.py [--reps 7] [--out profiles/resample_bench.jsonl] [--streams 65536] [--samples 8000] [--factor 6]"""
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
    ap.add_argument("--samples", type=int, default=8000)
    ap.add_argument("--factor", type=int, default=6)
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
    S, n, L = a.streams, a.samples, a.factor
    N = n * L
    eng = wm.FSKEngine(1, {})
    wide_bytes = S * N * 4
    d_a, d_b = eng.device_malloc(wide_bytes), eng.device_malloc(wide_bytes)       # two float tiles
    d_n = eng.device_malloc(S * N * 2)                                            # narrow samples, up to full rate s16
    for p, b in ((d_a, wide_bytes), (d_b, wide_bytes), (d_n, S * N * 2)):
        hip.check(hip.L.hipMemset(C.c_void_p(p), 0, C.c_size_t(b)), "hipMemset")
    ms = hip.timed(lambda: hip.check(hip.L.hipMemcpyDtoD(C.c_void_p(d_b), C.c_void_p(d_a), C.c_size_t(wide_bytes)), "hipMemcpyDtoD"), a.reps)
    copy = float(np.median(ms))
    emit(dict(call="hipMemcpyDtoD", streams=S, samples=N, bytes_moved=2 * wide_bytes, gb_per_s=round(2 * wide_bytes / copy / 1e6, 1), **_stats(ms)))

    for pname, prec in (("fp32", wm.PRECISION_F32), ("fp64", wm.PRECISION_F64)):
        up, down = wm.Upsampler(L, S, precision=prec), wm.Downsampler(L, S, precision=prec)
        fir_up, fir_down = wm.FIRFilterBatch(up.taps, S, precision=prec), wm.FIRFilterBatch(down.taps, S, precision=prec)
        ms = hip.timed(lambda: fir_up.process_device(d_a, N, N, d_b, N), a.reps)
        fir_ms = float(np.median(ms))
        emit(dict(call="fskhip_fir_process_device", precision=pname, streams=S, samples=N, taps=len(up.taps), gsamples_per_s=round(S * N / fir_ms / 1e6, 1),
                  x_dtod_time=round(fir_ms / copy, 3), **_stats(ms)))
        for fmt in ("mulaw", "s16"):
            for layout in ("stream", "sample"):
                # ---- up: low rate narrow -> float tile ------------------------------------------------------------------------
                lp, fp = (n, N) if layout == "stream" else (S, S)                 # narrow pitches at the low / full rate
                ms = hip.timed(lambda: up.process_device(d_n, fmt, layout, n, lp, d_b, N), a.reps)
                poly = float(np.median(ms))
                ms_i = hip.timed(lambda: wm.ingest_device(d_n, fmt, layout, S, N, fp, d_a, N), a.reps)

                def pair():
                    wm.ingest_device(d_n, fmt, layout, S, N, fp, d_a, N)
                    fir_up.process_device(d_a, N, N, d_b, N)

                ms_p = hip.timed(pair, a.reps)
                pair_ms = float(np.median(ms_p))
                emit(dict(call="fskhip_resampler_up_device", precision=pname, format=fmt, layout=layout, streams=S, samples_in=n, factor=L, taps=len(up.taps),
                          gsamples_out_per_s=round(S * N / poly / 1e6, 1), bytes_moved=S * n * ESZ[fmt] + wide_bytes,
                          gb_per_s=round((S * n * ESZ[fmt] + wide_bytes) / poly / 1e6, 1), x_dtod_time=round(poly / copy, 3),
                          ingest_ms_median=round(float(np.median(ms_i)), 4), pair_ms_median=round(pair_ms, 4), pair_ms_min=round(min(ms_p), 4),
                          pair_ms_max=round(max(ms_p), 4), x_pair_time=round(poly / pair_ms, 3), **_stats(ms)))
                # ---- down: float tile -> low rate narrow ------------------------------------------------------------------------
                ms = hip.timed(lambda: down.process_device(d_a, N, N, None, d_n, fmt, layout, lp), a.reps)
                poly = float(np.median(ms))
                row = dict(call="fskhip_resampler_down_device", precision=pname, format=fmt, layout=layout, streams=S, samples_in=N, factor=L, taps=len(down.taps),
                           gsamples_in_per_s=round(S * N / poly / 1e6, 1), bytes_moved=S * n * ESZ[fmt] + wide_bytes,
                           gb_per_s=round((S * n * ESZ[fmt] + wide_bytes) / poly / 1e6, 1), x_dtod_time=round(poly / copy, 3), **_stats(ms))
                if layout == "stream":
                    ms_e = hip.timed(lambda: wm.egress_device(d_b, L, None, S * n, 1, fmt, "stream", d_n, 1), a.reps)

                    def pair_down():
                        fir_down.process_device(d_a, N, N, d_b, N)
                        wm.egress_device(d_b, L, None, S * n, 1, fmt, "stream", d_n, 1)

                    ms_p = hip.timed(pair_down, a.reps)
                    pair_ms = float(np.median(ms_p))
                    row.update(egress_ms_median=round(float(np.median(ms_e)), 4), pair_ms_median=round(pair_ms, 4), pair_ms_min=round(min(ms_p), 4),
                               pair_ms_max=round(max(ms_p), 4), x_pair_time=round(poly / pair_ms, 3))
                else:
                    row.update(pair_ms_median=None, x_fir_time=round(poly / fir_ms, 3))   # (no strided sample-major egress exists: the FIR pass alone)
                emit(row)
        for h in (up, down, fir_up, fir_down):
            h.close()
    for p in (d_a, d_b, d_n):
        eng.device_free(p)
    eng.close()


if __name__ == "__main__":
    main()
