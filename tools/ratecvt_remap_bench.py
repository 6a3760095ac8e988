"""A rate converter's remap, snapshot and restore at full size (include/fskhip_next.h: fskhip_ratecvt_remap / _snapshot / _restore),
one process, one MI355X.

262 144 streams, the default designs between 44.1 kHz and 48 kHz (2 561 taps: 160 / 147 with 16 floats of history per stream for
capture, 147 / 160 with 18 for playback), a position in the middle of a period, a random permutation as the map.  Wall clock (every
call timed here is synchronous and ends with the device idle), median of --reps after 2 warm-ups.  In the same run, per design:
  * remapped(map) against the by-hand carry -- state(), a numpy take, a new handle, set_state(), position --, the pair timed twice;
  * snapshot() and from_snapshot() against a copy of the image's bytes between page-locked host memory and the device, each way;
  * a device-to-device copy of the live rows.
Before any time is taken both carries are checked to end in the same state and position, bit for bit, and the restored handle
likewise.  Nothing is asserted about the times: a row gives what the run gave.

usage: python tools/ratecvt_remap_bench.py [--reps 7] [--out profiles/ratecvt_remap_bench.jsonl] [--streams 262144]"""
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
from resample_remap_bench import wall  # noqa: E402

POSITION = 128      # one WebAudio render quantum behind a period boundary


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--streams", type=int, default=262144)
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
    rng = np.random.default_rng(262144)
    perm = rng.permutation(S).astype(np.int64)
    eng = wm.FSKEngine(1, {})
    for name, cls, rates in (("capture", wm.CaptureConverter, (44100, 48000)), ("playback", wm.PlaybackConverter, (48000, 44100))):
        src = cls(*rates, S)
        H = src.history
        src.set_state(rng.uniform(-1, 1, (S, H)).astype(np.float32))
        src.position = POSITION
        live = S * H * 4

        def by_hand():
            nxt = cls(*rates, S, taps=src.taps)
            nxt.set_state(src.state()[perm])
            nxt.position = src.position
            return nxt

        # both carries end in the same state, and so does the image's
        r, b = src.remapped(perm), by_hand()
        snap = src.snapshot()
        back = cls.from_snapshot(snap, perm, in_rate=rates[0], out_rate=rates[1])
        want = b.state().view(np.uint32)
        if not (np.array_equal(r.state().view(np.uint32), want) and np.array_equal(back.state().view(np.uint32), want)
                and r.position == b.position == back.position == POSITION):
            raise SystemExit("%s: remapped(), the by-hand carry and from_snapshot() disagree" % name)
        for h in (r, b, back):
            h.close()
        common = dict(direction=name, streams=S, up=src.up, down=src.down, n_taps=len(src.taps), history=H, position=POSITION, live_bytes=live)

        for timed in (1, 2):
            ms_remap = wall(lambda: src.remapped(perm), a.reps, after=lambda h: h.close())
            ms_hand = wall(by_hand, a.reps, after=lambda h: h.close())
            emit(dict(call="remapped", timed=timed, **common, **_stats(ms_remap)))
            emit(dict(call="by_hand", timed=timed, **common, **_stats(ms_hand), remap_over_by_hand=round(float(np.median(ms_remap) / np.median(ms_hand)), 3)))

        ms_snap = wall(src.snapshot, a.reps)
        ms_rest = wall(lambda: cls.from_snapshot(snap, perm), a.reps, after=lambda h: h.close())
        # the image's bytes between page-locked host memory and the device, and the live rows device to device
        pinned = wm.pinned_empty(len(snap), np.uint8)
        pinned[:] = np.frombuffer(snap, np.uint8)
        d_a, d_b = eng.device_malloc(len(snap)), eng.device_malloc(len(snap))

        def h2d():
            eng.h2d(d_a, pinned)
            eng.synchronize()

        def d2h():
            eng.d2h(pinned, d_a)
            eng.synchronize()

        ms_h2d, ms_d2h = wall(h2d, a.reps), wall(d2h, a.reps)
        ms_d2d = hip.timed(lambda: hip.check(hip.L.hipMemcpyDtoD(C.c_void_p(d_b), C.c_void_p(d_a), C.c_size_t(max(live, 1))), "hipMemcpyDtoD"), a.reps)
        eng.device_free(d_a)
        eng.device_free(d_b)
        emit(dict(call="snapshot", **common, image_bytes=len(snap), **_stats(ms_snap), over_pinned_d2h=round(float(np.median(ms_snap) / np.median(ms_d2h)), 3)))
        emit(dict(call="from_snapshot", **common, image_bytes=len(snap), **_stats(ms_rest), over_pinned_h2d=round(float(np.median(ms_rest) / np.median(ms_h2d)), 3)))
        emit(dict(call="pinned_d2h", **common, image_bytes=len(snap), **_stats(ms_d2h)))
        emit(dict(call="pinned_h2d", **common, image_bytes=len(snap), **_stats(ms_h2d)))
        emit(dict(call="hipMemcpyDtoD_live_rows", **common, clock="events", **_stats(ms_d2d)))
        src.close()
    eng.close()


if __name__ == "__main__":
    main()
