"""The rate converters' calls of any length at full size, and the whole-period calls against the commit before (include/fskhip_next.h:
"Rate conversion in calls of any length"), one process, one MI355X.

65 536 streams, the default designs' 2 561 taps, s16, device buffers of zeros, HIP events on the null stream, medians of --reps after
2 warm-ups; 44 100 samples per stream at 44.1 kHz <-> 48 000 at 48 kHz.
  (a) the existing whole-period calls, fskhip_ratecvt_capture_device / _playback_device on a handle at position 0, both layouts, fp32
      and fp64, from this tree's library and from --parent-lib (libfskhip.so built from the commit before), each pair timed twice in
      the run: rows "existing", with lib = this / parent and pass = 1 / 2.  A row "existing_vs_parent" per case gives this / parent
      of the medians and the spread the two passes of either library show; nothing is asserted here.
  (b) the any-length calls at the same size from position 0 and from position 73 (one sample fewer, so that the call is no whole
      number of periods), and the same stream in calls of 128 samples (344 calls, their time summed): rows "any".
  (c) --processor: FSKProcessorBatch.process_samples_at_any at 262 144 streams in 128-frame quanta against process_samples_at in
      147-frame quanta, as frames in s16 and mu-law, host calls, wall clock, per sample: rows "processor".
usage: python tools/ratecvt_any_bench.py [--parent-lib PATH] [--reps 7] [--out profiles/ratecvt_any_bench.jsonl] [--streams 65536] [--processor]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from ingest_bench import Hip, _stats  # noqa: E402

S16, STREAM, SAMPLE = 1, 0, 1
CAPTURE, PLAYBACK = 0, 1
P = C.c_void_p


def _raw(path):
    """the whole-period entry points of a libfskhip.so by path: both builds have them"""
    L = C.CDLL(path)
    L.fskhip_ratecvt_create.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_uint32, P, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(P)]
    L.fskhip_ratecvt_capture_device.argtypes = [P, P, C.c_int, C.c_int, C.c_size_t, C.c_size_t, P, C.c_size_t, P]
    L.fskhip_ratecvt_playback_device.argtypes = [P, P, C.c_size_t, C.c_size_t, P, P, C.c_int, C.c_int, C.c_size_t, P]
    L.fskhip_ratecvt_destroy.argtypes = [P]
    L.fskhip_last_error.restype = C.c_char_p
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--streams", type=int, default=65536)
    ap.add_argument("--periods", type=int, default=300)
    ap.add_argument("--parent-lib", default=None, help="libfskhip.so built from the commit before; without it (a) has no parent rows")
    ap.add_argument("--processor", action="store_true", help="(c) as well")
    ap.add_argument("--processor-streams", type=int, default=262144)
    a = ap.parse_args()
    import webaudio_modem_amd as wm
    from webaudio_modem_amd import _lib
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
    n_lo, n_hi = a.periods * 147, a.periods * 160
    eng = wm.FSKEngine(1, {})
    d_wide, d_narrow = eng.device_malloc(S * n_hi * 4), eng.device_malloc(S * n_lo * 2)
    for p, b in ((d_wide, S * n_hi * 4), (d_narrow, S * n_lo * 2)):
        hip.check(hip.L.hipMemset(C.c_void_p(p), 0, C.c_size_t(b)), "hipMemset")
    taps = {CAPTURE: wm.CaptureConverter.default_taps(44100, 48000), PLAYBACK: wm.PlaybackConverter.default_taps(48000, 44100)}
    ratio = {CAPTURE: (160, 147), PLAYBACK: (147, 160)}

    # ---- (a) ----
    libs = [("this", _raw(_lib.LIB_PATH))] + ([("parent", _raw(a.parent_lib))] if a.parent_lib else [])
    med = {}
    for pname, prec in (("fp32", wm.PRECISION_F32), ("fp64", wm.PRECISION_F64)):
        for direction, dname in ((CAPTURE, "capture"), (PLAYBACK, "playback")):
            for layout, lname in ((STREAM, "stream"), (SAMPLE, "sample")):
                handles = {}
                for name, L in libs:
                    h = P()
                    t = taps[direction]
                    rc = L.fskhip_ratecvt_create(0, direction, ratio[direction][0], ratio[direction][1], (C.c_double * len(t))(*t), len(t), S, prec, C.byref(h))
                    if rc:
                        raise RuntimeError(L.fskhip_last_error().decode())
                    handles[name] = h
                npitch = n_lo if layout == STREAM else S
                for rep in (1, 2):
                    for name, L in libs:
                        h = handles[name]
                        if direction == CAPTURE:
                            fn = lambda: L.fskhip_ratecvt_capture_device(h, d_narrow, S16, layout, n_lo, npitch, d_wide, n_hi, None)      # noqa: E731
                        else:
                            fn = lambda: L.fskhip_ratecvt_playback_device(h, d_wide, n_hi, n_hi, None, d_narrow, S16, layout, npitch, None)   # noqa: E731
                        assert fn() == 0, L.fskhip_last_error().decode()
                        ms = hip.timed(fn, a.reps)
                        med[(pname, dname, lname, name, rep)] = float(np.median(ms))
                        emit(dict(part="existing", lib=name, **{"pass": rep}, call="fskhip_ratecvt_%s_device" % dname, precision=pname, format="s16", layout=lname,
                                  streams=S, samples_in=n_lo if direction == CAPTURE else n_hi, **_stats(ms)))
                for name, L in libs:
                    L.fskhip_ratecvt_destroy(handles[name])
                if a.parent_lib:
                    k = (pname, dname, lname)
                    this, parent = [med[k + ("this", r)] for r in (1, 2)], [med[k + ("parent", r)] for r in (1, 2)]
                    spread = max(abs(this[0] - this[1]) / min(this), abs(parent[0] - parent[1]) / min(parent))
                    emit(dict(part="existing_vs_parent", precision=pname, direction=dname, layout=lname, this_ms=[round(v, 4) for v in this],
                              parent_ms=[round(v, 4) for v in parent], this_over_parent=round(min(this) / min(parent), 4),
                              this_over_parent_of_means=round(sum(this) / sum(parent), 4), spread_of_a_pair=round(spread, 4)))

    # ---- (b) ----
    for pname, prec in (("fp32", wm.PRECISION_F32), ("fp64", wm.PRECISION_F64)):
        cap, play = wm.CaptureConverter(44100, 48000, S, precision=prec), wm.PlaybackConverter(48000, 44100, S, precision=prec)
        for layout in ("stream", "sample"):
            npitch = n_lo if layout == "stream" else S
            for h, dname, n_full, m in ((cap, "capture", n_lo, 147), (play, "playback", n_hi, 160)):
                def call(n, at=0):
                    if h is cap:
                        off = at * 2 if layout == "stream" else at * S * 2
                        return h.process_any_device(d_narrow + off, "s16", layout, n, npitch, d_wide, n_hi)
                    return h.process_any_device(d_wide + at * 4, n, n_hi, None, d_narrow, "s16", layout, npitch)

                def from_position(pos, n):
                    def fn():
                        h.position = pos
                        call(n)
                    return fn

                def in_quanta():
                    h.position = 0
                    for q in range(n_full // 128):
                        call(128, q * 128)
                for what, fn, n in (("position 0", from_position(0, n_full), n_full), ("position 0, one sample fewer", from_position(0, n_full - 1), n_full - 1),
                                    ("position 73", from_position(73, n_full - 1), n_full - 1), ("calls of 128", in_quanta, n_full // 128 * 128)):
                    ms = hip.timed(fn, a.reps)
                    ref = med.get((pname, dname, layout, "this", 1))
                    emit(dict(part="any", call="fskhip_ratecvt_%s_any_device" % dname, case=what, precision=pname, format="s16", layout=layout, streams=S, samples_in=n,
                              x_existing_call=None if ref is None else round(float(np.median(ms)) / ref * n_full / n, 3), **_stats(ms)))
        cap.close()
        play.close()
    for p in (d_wide, d_narrow):
        eng.device_free(p)
    eng.close()

    # ---- (c) ----
    if a.processor:
        Sp = a.processor_streams
        e = wm.FSKEngine(Sp, dict(baudRate=1200, markFrequency=1200, spaceFrequency=2200))
        proc = wm.FSKProcessorBatch(e)
        cap, play = wm.CaptureConverter(44100, 48000, Sp), wm.PlaybackConverter(48000, 44100, Sp)
        for fmt, dt in (("s16", np.int16), ("mulaw", np.uint8)):
            for name, fn, q in (("process_samples_at_any", proc.process_samples_at_any, 128), ("process_samples_at", proc.process_samples_at, 147)):
                for h in (cap, play):
                    h.reset()
                x = np.zeros((q, Sp), dt)
                ms = []
                for r in range(a.reps + 2):
                    t0 = time.perf_counter()
                    fn(x, fmt, "sample", cap, q, fmt, "sample", play)
                    if r >= 2:
                        ms.append((time.perf_counter() - t0) * 1e3)
                emit(dict(part="processor", call=name, format=fmt, layout="sample", streams=Sp, quantum=q, us_per_sample=round(float(np.median(ms)) * 1e3 / q, 3), **_stats(ms)))
        for h in (cap, play, proc, e):
            h.close()


if __name__ == "__main__":
    main()
