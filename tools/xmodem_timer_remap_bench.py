"""fskhip_xmodem_timer_remap / _snapshot / _restore at the size the XModem rows are quoted at: 262 144 streams (fp32 engine,
rx_capacity 1024), a file receiver's and a sender's timers with random valid words, under one random permutation map:
  (a) remapped     the new call into a freshly created timer;
  (b) by hand      what a host does without it for the same effect: state(), a numpy take of the two words by the map, a new
                   object over the destination handle, set_state();
and snapshot / from_snapshot against a page-locked device -> host / host -> device copy of the image's bytes.  (a)'s words are checked
against (b)'s before a time is taken.  Timing: wall clock around each synchronous call, after two warm-up calls, median of --reps;
(a), (b) and from_snapshot each include creating and closing the destination timer, alike.  Each pair is timed twice in one run
(`pass` 0 and 1), so that a drift of the machine between the two sides of a pair shows.  Writes one JSON line per kind and pass to
--out (default profiles/xmodem_timer_remap_bench.jsonl).

usage: python tools/xmodem_timer_remap_bench.py [--streams 262144] [--reps 7] [--out FILE] [--kinds recv,tx]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(min(t)), float(max(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=262144)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "xmodem_timer_remap_bench.jsonl"))
    ap.add_argument("--kinds", default="recv,tx")
    a = ap.parse_args()
    import webaudio_modem_amd as wm
    from webaudio_modem_amd import _lib
    L = _lib.lib()
    S = a.streams
    rng = np.random.default_rng(0xBE7D)
    perm = rng.permutation(S).astype(np.int64)
    eng = wm.FSKEngine(S, {}, precision=wm.PRECISION_F32)
    procs = [wm.FSKProcessorBatch(eng, rx_capacity=1024) for _ in range(2)]   # the timers never touch the processor: two serve both kinds
    src_proc, dst_proc = procs

    def pinned_ms(n):
        """page-locked host -> device and device -> host copies of n bytes"""
        h, d = C.c_void_p(), C.c_void_p()
        _lib.check(L.fskhip_host_alloc(max(n, 16), C.byref(h)))
        _lib.check(L.fskhip_device_malloc(eng._h, max(n, 16), C.byref(d)))
        up = median_ms(lambda: _lib.check(L.fskhip_memcpy_h2d(eng._h, d, h, max(n, 16))), a.reps)
        down = median_ms(lambda: _lib.check(L.fskhip_memcpy_d2h(eng._h, h, d, max(n, 16))), a.reps)
        L.fskhip_device_free(eng._h, d)
        L.fskhip_host_free(h)
        return up, down

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as out:
        for kind in a.kinds.split(","):
            if kind == "recv":
                src_h, dst_h, timeout, marks = wm.XModemFileReceiverBatch(src_proc, 64, 10), wm.XModemFileReceiverBatch(dst_proc, 64, 10), 144000, (0, 1, 2, 4, 5, 6)
            else:
                src_h, dst_h, timeout, marks = wm.XModemSenderBatch(src_proc, 128, 10), wm.XModemSenderBatch(dst_proc, 128, 10), 144000, (0, 4)
            src = wm.XModemTimers(src_h, timeout)
            src.set_state(waited=rng.integers(0, 2 * timeout, S, dtype=np.uint32), mark=rng.choice(np.array(marks, np.uint32), S))

            def by_hand():
                st = src.state()
                d = wm.XModemTimers(dst_h, timeout)
                d.set_state(waited=st["waited"][perm], mark=st["mark"][perm])
                return d

            def remap():
                return src.remapped(dst_h, perm)
            want, got = by_hand(), remap()
            assert want.snapshot() == got.snapshot(), "the remap and the by-hand path disagree"
            want.close()
            got.close()

            def timed(fn):
                def go():
                    fn().close()
                return median_ms(go, a.reps)
            image = src.snapshot()
            for rep in range(2):
                t_remap, t_hand = timed(remap), timed(by_hand)
                t_snap = median_ms(lambda: src.snapshot(), a.reps)
                t_rest = timed(lambda: wm.XModemTimers.from_snapshot(dst_h, image))
                up, down = pinned_ms(len(image))
                row = dict(kind=kind, streams=S, image_bytes=len(image), reps=a.reps, remapped_ms=t_remap, by_hand_ms=t_hand, snapshot_ms=t_snap,
                           from_snapshot_ms=t_rest, pinned_h2d_ms=up, pinned_d2h_ms=down)
                row["pass"] = rep
                out.write(json.dumps(row) + "\n")
                out.flush()
                print(json.dumps(row))
            for x in (src, src_h, dst_h):
                x.close()
    for p in procs:
        p.close()
    eng.close()


if __name__ == "__main__":
    main()
