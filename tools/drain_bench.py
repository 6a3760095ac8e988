"""The compacted RX drain (fskhip_processor_rx_drain_sparse_host) against the dense one (fskhip_processor_rx_drain_host) at the
size the processor row is quoted at: 262 144 streams, rx_capacity 1024 (fp32 engines, Bell-202).  Cases: 0, 0.1 %, 1 %, 10 % and
100 % of the streams hold 1..64 bytes each (random streams, random readIndex, so spans wrap now and then), and every ring full.
One source processor is brought to each state by restoring an image crafted here from the documented layout
(include/fskhip_next.h); every timed call drains a clone of it (fskhip_processor_remap with the identity into a freshly created
processor -- what FSKProcessorBatch.remapped(identity) does underneath), sparse and dense in the same run on the same state, and
the two results are compared stream by stream before anything is timed.
Timing: wall clock around the synchronous C calls with the host buffers already allocated -- sparse: the size query plus the
drain into buffers of exactly the reported size, as FSKProcessorBatch.demodulate_sparse makes them; dense: the one call into an
[S][rx_capacity] slab -- median of --reps after two warm-ups, one process.  Comparator beside both: a bare page-locked
device-to-host copy of the live bytes (plus the two list words per active stream).

usage: python tools/drain_bench.py [--streams 262144] [--rx-capacity 1024] [--reps 7] [--out profiles/drain_bench.jsonl]"""
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


def craft_image(S, cap, lengths, rng):
    """a canonical image of S streams with nothing pending: stream s holds lengths[s] bytes from a random readIndex"""
    rb = FIXED + ((cap + 15) & ~15)
    blob = np.zeros(HEADER + S * rb, np.uint8)
    blob[:HEADER].view("<u4")[:8] = [0x504B5346, 1, HEADER, rb, S, cap, 0, 0]
    rec = blob[HEADER:].reshape(S, rb)
    read = rng.integers(0, cap, S)
    words = np.zeros((S, 4), np.uint32)
    words[:, 0], words[:, 1], words[:, 2] = (read + lengths) % cap, read, lengths
    rec[:, :16] = words.view(np.uint8)
    x = np.arange(cap)[None, :]
    for lo in range(0, S, 16384):   # (slabs: the [S][cap] masks of the whole batch would not fit comfortably)
        hi = min(S, lo + 16384)
        live = (x - read[lo:hi, None]) % cap < lengths[lo:hi, None]
        rec[lo:hi, FIXED:FIXED + cap] = np.where(live, rng.integers(1, 256, (hi - lo, cap), dtype=np.uint8), 0)
    blob[32:40].view("<u8")[0] = checksum(blob)
    return blob


def median_ms(fn, reps, setup, teardown):
    times = []
    for r in range(reps + 2):
        ctx = setup()
        t0 = time.perf_counter()
        fn(ctx)
        t1 = time.perf_counter()
        teardown(ctx)
        if r >= 2:
            times.append((t1 - t0) * 1e3)
    return float(np.median(times))


def pinned_d2h_ms(L, check, eng, nbytes, reps):
    """a bare device-to-host copy of nbytes into page-locked memory (fskhip_host_alloc), synchronous"""
    nbytes = max(int(nbytes), 16)
    dev, host = C.c_void_p(), C.c_void_p()
    check(L.fskhip_device_malloc(eng._h, nbytes, C.byref(dev)))
    check(L.fskhip_host_alloc(nbytes, C.byref(host)))
    try:
        return median_ms(lambda _: check(L.fskhip_memcpy_d2h(eng._h, host, dev, nbytes)), reps, lambda: None, lambda _: None)
    finally:
        L.fskhip_host_free(host)
        L.fskhip_device_free(eng._h, dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=262144)
    ap.add_argument("--rx-capacity", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import webaudio_modem_amd as wm
    from webaudio_modem_amd import _lib
    L = _lib.lib()
    S, cap = a.streams, a.rx_capacity
    rng = np.random.default_rng(11)
    ident = np.arange(S, dtype=np.int64)
    eng_src = wm.FSKEngine(S, CFG, precision=wm.PRECISION_F32)
    eng_dst = wm.FSKEngine(S, CFG, precision=wm.PRECISION_F32)
    rows = []
    dense_out, dense_counts = np.zeros((S, cap), np.uint8), np.zeros(S, np.uint32)
    na, nb = C.c_uint32(0), C.c_uint32(0)
    sparse = L.fskhip_processor_rx_drain_sparse_host

    for name, frac, full in (("idle", 0.0, False), ("0.1%", 0.001, False), ("1%", 0.01, False), ("10%", 0.1, False), ("100%", 1.0, False),
                             ("all_full", 1.0, True)):
        holds = rng.random(S) < frac if frac < 1.0 else np.ones(S, bool)
        lengths = np.where(holds, cap if full else rng.integers(1, min(64, cap) + 1, S), 0)
        blob = craft_image(S, cap, lengths, rng)
        src = wm.FSKProcessorBatch(eng_src, rx_capacity=cap)
        _lib.check(L.fskhip_processor_restore(src._h, blob.ctypes.data, blob.nbytes, ident.ctypes.data, S))
        del blob
        n_active, n_bytes = int(holds.sum() if frac else 0), int(lengths.sum())
        streams, offsets, data = np.zeros(n_active, np.uint32), np.zeros(n_active + 1, np.uint32), np.zeros(n_bytes, np.uint8)

        def clone():
            d = wm.FSKProcessorBatch(eng_dst, rx_capacity=cap)
            _lib.check(L.fskhip_processor_remap(d._h, src._h, ident.ctypes.data, S))
            return d

        def run_sparse(d):
            rc = sparse(d._h, None, 1, None, None, 0, None, 0, C.byref(na), C.byref(nb))
            if rc == _lib.E_OVERFLOW:
                rc = sparse(d._h, None, 1, streams.ctypes.data, offsets.ctypes.data, na.value, data.ctypes.data, nb.value, C.byref(na), C.byref(nb))
            _lib.check(rc)

        def run_dense(d):
            _lib.check(L.fskhip_processor_rx_drain_host(d._h, dense_out.ctypes.data, cap, dense_counts.ctypes.data))

        # the same state, the same bytes: checked before anything is timed
        d1, d2 = clone(), clone()
        run_sparse(d1)
        run_dense(d2)
        assert (na.value, nb.value) == (n_active, n_bytes) and np.array_equal(streams, np.flatnonzero(lengths)) and offsets[-1] == n_bytes
        assert np.array_equal(dense_counts, lengths)
        for i in rng.choice(n_active, min(n_active, 2000), replace=False) if n_active else []:
            s = streams[i]
            assert np.array_equal(data[offsets[i]:offsets[i + 1]], dense_out[s, :lengths[s]]), s
        d1.close()
        d2.close()

        sparse_ms = median_ms(run_sparse, a.reps, clone, lambda d: d.close())
        dense_ms = median_ms(run_dense, a.reps, clone, lambda d: d.close())
        live = n_bytes + 4 * (2 * n_active + 1)
        row = dict(case=name, streams=S, rx_capacity=cap, n_active=n_active, n_bytes=n_bytes, sparse_ms=round(sparse_ms, 3), dense_ms=round(dense_ms, 3),
                   dense_over_sparse=round(dense_ms / sparse_ms, 1), pinned_d2h_live_ms=round(pinned_d2h_ms(L, _lib.check, eng_src, live, a.reps), 3), live_bytes=live,
                   dense_bytes=S * cap + 4 * S, reps=a.reps)
        rows.append(row)
        print(json.dumps(row), flush=True)
        src.close()
    eng_src.close()
    eng_dst.close()
    if a.out:
        with open(a.out, "w") as fh:
            for row in rows:
                fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
