"""fskhip_processor_remap / _snapshot / _restore at the size the processor row is quoted at: 262 144 streams, rx_capacity 1024 (fp32
engines, Bell-202).  Cases: map identity | random permutation; ring fill empty | half (every other stream's span wraps) | full;
with and without a pending modulation (an 11-byte payload, mid-signal) on every stream.  The source processor is brought to each
state by restoring an image crafted here from the documented layout (include/fskhip_next.h), so a case costs no demodulation.
Timing: wall clock around each synchronous call into a freshly created processor, after two warm-up calls, median of --reps --
the whole call: checks, map copy, payload-size pass, staging, device synchronisations, kernels (the image calls: PCIe and the
host's checksum as well).  Kernels alone: run this under `rocprofv3 --kernel-trace --stats` with --reps 1
(profiles/processor_remap_kernel_time.txt).
Comparators, measured here: a device-to-device copy of the bytes actually live (ring spans + payloads + words) and of the whole
ring store; the engine's fskhip_remap_streams at the same stream count and map; a page-locked host<->device copy of the image's size.
GB/s of the remap counts live bytes read and written once each.

--fills / --maps / --pending narrow the cases (a profiler run of one case); --no-comparators skips the copies and the engine remap.

usage: python tools/processor_remap_bench.py [--streams 262144] [--rx-capacity 1024] [--reps 7] [--out FILE]
                                             [--fills empty,half,full] [--maps identity,random] [--pending 0,1] [--no-comparators]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG = dict(baudRate=1200, markFrequency=1200, spaceFrequency=2200)
HEADER, FIXED = 48, 64


def checksum(blob):
    w = blob.view("<u8")
    with np.errstate(over="ignore"):
        a = np.cumsum(w, dtype=np.uint64)
        b = np.sum(a, dtype=np.uint64)
        return int((a[-1] * np.uint64(0x9E3779B97F4A7C15)) ^ b)


def craft_image(S, cap, fill, pending, rng):
    """a canonical image of S streams: `fill` bytes in every ring (odd streams start 3/4 of the way round, so their span wraps
    unless the ring is empty), and where `pending` an 11-byte payload 1000 samples into its 5600-sample signal"""
    pay_cap = 16 if pending else 0
    rb = FIXED + pay_cap + cap
    blob = np.zeros(HEADER + S * rb, np.uint8)
    blob[:HEADER].view("<u4")[:8] = [0x504B5346, 1, HEADER, rb, S, cap, pay_cap, 0]
    rec = blob[HEADER:].reshape(S, rb)
    words = np.zeros((S, 16), np.uint32)
    read = np.where(np.arange(S) % 2 == 1, (3 * cap) // 4, 0).astype(np.uint32) if fill else np.zeros(S, np.uint32)
    words[:, 0] = (read + fill) % cap
    words[:, 1] = read
    words[:, 2] = fill
    if pending:
        words[:, 3] = 1
        words[:, 5], words[:, 6], words[:, 7] = 1000, 5600, 11      # (3 + 11) bytes x 10 bits x 40 samples
        words[:, 8], words[:, 9], words[:, 10] = 0, 25, 1           # (a plausible bit cursor: nothing here produces samples)
        rec[:, FIXED:FIXED + 11] = rng.integers(0, 256, (S, 11), dtype=np.uint8)
    rec[:, :FIXED] = words.view(np.uint8)
    if fill:
        ring = rec[:, FIXED + pay_cap:]
        data = rng.integers(1, 256, (S, fill), dtype=np.uint8)
        pos = (read[:, None].astype(np.int64) + np.arange(fill)[None, :]) % cap
        np.put_along_axis(ring, pos, data, axis=1)
    blob[32:40].view("<u8")[0] = checksum(blob)
    return blob, rb


def median_ms(fn, reps, setup=None, teardown=None):
    times = []
    for r in range(reps + 2):
        ctx = setup() if setup else None
        t0 = time.perf_counter()
        fn(ctx)
        t1 = time.perf_counter()
        if teardown:
            teardown(ctx)
        if r >= 2:
            times.append((t1 - t0) * 1e3)
    return float(np.median(times))


def torch_copy_ms(nbytes, kind, reps):
    import torch
    nbytes = max(int(nbytes), 16)
    dev = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    other = torch.empty(nbytes, dtype=torch.uint8, device="cuda") if kind == "d2d" else torch.empty(nbytes, dtype=torch.uint8).pin_memory()

    def run(_):
        if kind == "h2d":
            dev.copy_(other, non_blocking=True)
        else:
            other.copy_(dev, non_blocking=True)
        torch.cuda.synchronize()
    return median_ms(run, reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=262144)
    ap.add_argument("--rx-capacity", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--fills", default="empty,half,full")
    ap.add_argument("--maps", default="identity,random")
    ap.add_argument("--pending", default="0,1")
    ap.add_argument("--no-comparators", action="store_true")
    a = ap.parse_args()
    import webaudio_modem_amd as wm
    from webaudio_modem_amd import _lib
    L = _lib.lib()
    S, cap = a.streams, a.rx_capacity
    rng = np.random.default_rng(7)
    maps = {"identity": np.arange(S, dtype=np.int64), "random": rng.permutation(S).astype(np.int64)}
    maps = {k: v for k, v in maps.items() if k in a.maps.split(",")}
    copy_ms = (lambda nbytes, kind: float("nan")) if a.no_comparators else (lambda nbytes, kind: torch_copy_ms(nbytes, kind, a.reps))
    eng_src = wm.FSKEngine(S, CFG, precision=wm.PRECISION_F32)
    eng_dst = wm.FSKEngine(S, CFG, precision=wm.PRECISION_F32)
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    # comparator: the engine's own gather at this stream count (fskhip_remap_streams into a new engine)
    for mname, m in ({} if a.no_comparators else maps).items():
        ms = median_ms(lambda e: e.remap_from(eng_src, m), a.reps, setup=lambda: wm.FSKEngine(S, CFG, precision=wm.PRECISION_F32), teardown=lambda e: e.close())
        emit(dict(case="engine_remap_streams", map=mname, streams=S, ms_median=round(ms, 3)))
    if not a.no_comparators:
        emit(dict(case="d2d_copy_whole_ring_store", streams=S, bytes=S * cap, ms_median=round(copy_ms(S * cap, "d2d"), 3)))

    fresh = lambda: wm.FSKProcessorBatch(eng_dst, rx_capacity=cap)   # noqa: E731
    for fname, fill in (("empty", 0), ("half", cap // 2), ("full", cap)):
        for pending in (False, True):
            if fname not in a.fills.split(",") or str(int(pending)) not in a.pending.split(","):
                continue
            blob, rb = craft_image(S, cap, fill, pending, rng)
            ident = maps["identity"]
            src = wm.FSKProcessorBatch(eng_src, rx_capacity=cap)
            _lib.check(L.fskhip_processor_restore(src._h, blob.ctypes.data, blob.nbytes, ident.ctypes.data, S))
            live = S * (fill + (11 if pending else 0) + 52)
            d2d = copy_ms(live, "d2d")
            pin_d2h, pin_h2d = copy_ms(blob.nbytes, "d2h"), copy_ms(blob.nbytes, "h2d")
            out = np.zeros(blob.nbytes, np.uint8)
            w = C.c_size_t(0)
            snap = median_ms(lambda _: _lib.check(L.fskhip_processor_snapshot(src._h, None, 0, out.ctypes.data, out.nbytes, C.byref(w))), a.reps)
            assert w.value == blob.nbytes and bytes(out[:4096]) == bytes(blob[:4096])
            for mname, m in maps.items():
                remap = median_ms(lambda d: _lib.check(L.fskhip_processor_remap(d._h, src._h, m.ctypes.data, S)), a.reps, setup=fresh, teardown=lambda d: d.close())
                restore = median_ms(lambda d: _lib.check(L.fskhip_processor_restore(d._h, blob.ctypes.data, blob.nbytes, m.ctypes.data, S)), a.reps, setup=fresh,
                                    teardown=lambda d: d.close())
                emit(dict(case="processor", map=mname, fill=fname, pending=pending, streams=S, rx_capacity=cap, live_bytes=live, image_bytes=int(blob.nbytes),
                          remap_ms=round(remap, 3), remap_gbs=round(2.0 * live / (remap * 1e-3) / 1e9, 1), d2d_live_ms=round(d2d, 3),
                          remap_over_d2d=round(remap / d2d, 2), snapshot_ms=round(snap, 3), restore_ms=round(restore, 3),
                          pinned_d2h_ms=round(pin_d2h, 3), pinned_h2d_ms=round(pin_h2d, 3), snapshot_over_pinned=round(snap / pin_d2h, 2),
                          restore_over_pinned=round(restore / pin_h2d, 2)))
            src.close()
    eng_src.close()
    eng_dst.close()
    if a.out:
        with open(a.out, "w") as fh:
            for row in rows:
                fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
