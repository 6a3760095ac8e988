"""fskhip_snapshot_streams / fskhip_restore_streams at full size: 65 536 config-#3 streams (Bell-202, 1200 baud), fp32 and fp64,
identity and random selection / map, into and out of page-locked and pageable host memory.  The source has demodulated 0.1 s
first (its state is live); every timed restore goes into a new, never demodulated engine.  Timing: wall clock around the
synchronous call, after two warm-up calls, median / min / max of --reps -- the whole call: validation and checksum on the host,
staging allocation, device synchronisations, kernels and copies.  The floor it is reported against is timed here too: one
hipMemcpy of the same byte count from / to page-locked memory.  The kernels alone: run this under `rocprofv3 --kernel-trace --stats`
(with --reps 3) and take snap_pack_kernel's / snap_unpack_kernel's dispatches (profiles/snapshot_kernel_time.txt); nothing timed
under the profiler is a wall-clock figure.

usage: python tools/snapshot_bench.py [--streams 65536] [--reps 7] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _timed(fn, reps):
    t = []
    for r in range(reps + 2):
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        if r >= 2:
            t.append((t1 - t0) * 1e3)
    return dict(ms_median=round(float(np.median(t)), 4), ms_min=round(min(t), 4), ms_max=round(max(t), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import webaudio_modem_amd as wm
    S = a.streams
    cfg = dict(baudRate=1200, markFrequency=1200, spaceFrequency=2200)
    rng = np.random.default_rng(1)
    orders = {"identity": np.arange(S, dtype=np.int64), "random": rng.permutation(S).astype(np.int64)}
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
        for p_ in (o, c):
            src.device_free(p_)
        nbytes = len(src.snapshot())
        pinned = wm.pinned_empty(nbytes, np.uint8)
        pageable = np.zeros(nbytes, np.uint8)
        # the floor: one copy of the same bytes between the device and page-locked memory
        dbuf = src.device_malloc(nbytes)
        floor_d2h = _timed(lambda: src.d2h(pinned, dbuf), a.reps)
        floor_h2d = _timed(lambda: src.h2d(dbuf, pinned), a.reps)
        src.device_free(dbuf)
        src.device_free(x)
        for oname, order in orders.items():
            for mname, buf in (("page-locked", pinned), ("pageable", pageable)):
                t = _timed(lambda: src.snapshot(order, out=buf), a.reps)
                row = dict(call="snapshot", precision=pname, order=oname, memory=mname, streams=S, bytes=nbytes,
                           floor_ms=floor_d2h["ms_median"], x_floor=round(t["ms_median"] / floor_d2h["ms_median"], 2), **t)
                rows.append(row)
                print(json.dumps(row), flush=True)
        src.snapshot(out=pinned)
        pageable[:] = pinned
        for oname, order in orders.items():
            for mname, buf in (("page-locked", pinned), ("pageable", pageable)):
                t = []
                for r in range(a.reps + 2):
                    dst = wm.FSKEngine(S, cfg, precision=prec)
                    dst.synchronize()
                    t0 = time.perf_counter()
                    dst.restore_from(buf, order)
                    t1 = time.perf_counter()
                    dst.close()
                    if r >= 2:
                        t.append((t1 - t0) * 1e3)
                tt = dict(ms_median=round(float(np.median(t)), 4), ms_min=round(min(t), 4), ms_max=round(max(t), 4))
                row = dict(call="restore", precision=pname, order=oname, memory=mname, streams=S, bytes=nbytes,
                           floor_ms=floor_h2d["ms_median"], x_floor=round(tt["ms_median"] / floor_h2d["ms_median"], 2), **tt)
                rows.append(row)
                print(json.dumps(row), flush=True)
        # the yardstick the issue names for the kernels: an identity remap in the same run (its kernel shows in the same trace)
        t = []
        for r in range(a.reps + 2):
            dst = wm.FSKEngine(S, cfg, precision=prec)
            dst.synchronize()
            t0 = time.perf_counter()
            dst.remap_from(src, orders["identity"])
            t1 = time.perf_counter()
            dst.close()
            if r >= 2:
                t.append((t1 - t0) * 1e3)
        row = dict(call="remap", precision=pname, order="identity", streams=S, ms_median=round(float(np.median(t)), 4), ms_min=round(min(t), 4),
                   ms_max=round(max(t), 4))
        rows.append(row)
        print(json.dumps(row), flush=True)
        src.close()
    if a.out:
        with open(a.out, "w") as fh:
            for row in rows:
                fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
