"""fskhip_remap_streams at full size: 65 536 config-#3 streams (Bell-202, 1200 baud), fp32 and fp64, four maps -- identity, reversed,
64-block shuffle (whole 64-stream groups permuted), random permutation.  The source has demodulated 0.1 s first (its state is
live); every timed call remaps into a new, never demodulated engine.  Timing: wall clock around the synchronous call, after two
warm-up calls, median of --reps -- the whole call: map allocation and copy, checks, device synchronisations and the gather.  The
gather alone: run this under `rocprofv3 --kernel-trace` and take remap_kernel's dispatches (profiles/remap_kernel_time.txt).  GB/s counts the per-stream state read and written once each (RF / IF rows, polyphase registers,
amplitude ring: fsk_params.h) against the 8 TB/s HBM peak.

usage: python tools/remap_bench.py [--streams 65536] [--reps 7] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM_PEAK_GBS = 8000.0


def state_bytes_per_stream(prec, d, wide):
    import state_fields
    real = len(state_fields.REAL) * (8 if prec else 4)
    ints = len(state_fields.INT) * 4
    poly = d * (8 if wide else 4)
    amp = 8 * d * 4
    return real + ints + poly + amp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import webaudio_modem_amd as wm
    S = a.streams
    cfg = dict(baudRate=1200, markFrequency=1200, spaceFrequency=2200)
    d = int(48000 // 2 // 1200)
    rng = np.random.default_rng(1)
    blocks = rng.permutation(S // 64)
    maps = {
        "identity": np.arange(S, dtype=np.int64),
        "reversed": np.arange(S - 1, -1, -1, dtype=np.int64),
        "block64-shuffle": (blocks[:, None] * 64 + np.arange(64)[None, :]).reshape(-1).astype(np.int64),
        "random": rng.permutation(S).astype(np.int64),
    }
    rows = []
    for prec, pname in ((wm.PRECISION_F32, "fp32"), (wm.PRECISION_F64, "fp64")):
        src = wm.FSKEngine(S, cfg, precision=prec)
        n = 4800
        x = src.device_malloc(S * n * 4)
        o = src.device_malloc(S * 64)
        c = src.device_malloc(S * 4)
        src.synth_device(x, n, n, 100, 67001, 400, 0.1, 1.0)
        src.demodulate_device(x, n, n, o, 64, c)
        src.synchronize()
        for p_ in (x, o, c):
            src.device_free(p_)
        per = state_bytes_per_stream(prec, d, False)
        for mname, m in maps.items():
            times = []
            for r in range(a.reps + 2):
                dst = wm.FSKEngine(S, cfg, precision=prec)
                dst.synchronize()
                t0 = time.perf_counter()
                dst.remap_from(src, m)
                t1 = time.perf_counter()
                dst.close()
                if r >= 2:
                    times.append((t1 - t0) * 1e3)
            ms = float(np.median(times))
            gbs = 2.0 * per * S / (ms * 1e-3) / 1e9
            row = dict(precision=pname, map=mname, streams=S, state_bytes_per_stream=per, ms_median=round(ms, 4),
                       ms_min=round(min(times), 4), gbs=round(gbs, 1), frac_of_hbm_peak=round(gbs / HBM_PEAK_GBS, 4))
            rows.append(row)
            print(json.dumps(row), flush=True)
        src.close()
    if a.out:
        with open(a.out, "w") as fh:
            for row in rows:
                fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
