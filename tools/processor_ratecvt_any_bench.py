"""The any-length streaming quantum at 44.1 kHz (include/fskhip_next.h: fskhip_processor_process_ratecvt_any_host / _device): 262 144
streams, Bell 202 at 48 kHz between a CaptureConverter (160 / 147) and a PlaybackConverter (147 / 160) of the default design (2 561
taps), fp32 handles, S16 and mu-law, stream-major, one process, one MI355X.  Median of --reps after 2 warm-ups.  Every step is a
process of its own under its own time limit, and appends its rows to --out.

(a) `kernel`: TX only, HIP events on the null stream, device buffers, quanta of 128 starting from playback positions 0 and 73 (the
    position moves on from call to call, as it does in use): the fused any-length kernel (processor_io_ratecvt_kernel<any>, one
    launch) against the pair it replaces -- processor_io_kernel into a float tile, then ratecvt_playback_any_kernel -- which
    FSKHIP_PROC_RATECVT_PAIR forces through the same call.  The pair is timed twice (pair_a, pair_b): their difference is the run's
    own spread.  `faster_than_pair`: the fused median is below the pair's faster median by more than that spread -- the rule by
    which a case is dispatched to the fused kernel.  The whole-period kernel at 147 and its pair are timed the same way in the
    same run.
(b) `host`: fskhip_processor_process_ratecvt_any_host at 128-frame quanta, page-locked memory, wall clock around the synchronous
    call: RX only, TX only and both, so that how a quantum's time divides between the capture side and the TX side is on record.
(c) `whole`: fskhip_processor_process_ratecvt_host at 147, both sides, in the same run, for the per-sample ratio.

usage: python tools/processor_ratecvt_any_bench.py [--reps 7] [--out profiles/processor_ratecvt_any_bench.jsonl] [--streams 262144]
       [--parts kernel,host,whole]"""
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
from processor_fmt_bench import pending  # noqa: E402
import samples_ref as sr  # noqa: E402

QUANTUM, WHOLE = 128, 147
OUTER, ENGINE = 44100, 48000
UP, DOWN = 147, 160          # the playback converter's; the capture converter's are the other way round
TAPS = 16 * DOWN + 1
FORMATS = ("s16", "mulaw")
POSITIONS = (0, 73)
STEP_SECONDS = 400


def kernel_rows(a, wm, emit):
    from webaudio_modem_amd import _lib
    hip = Hip()
    S = a.streams
    eng = wm.FSKEngine(S, BELL)
    d_out = eng.device_malloc(S * WHOLE * 2)

    def series(q, fmt, pos, pair, whole):
        proc, play = pending(wm, eng, S), wm.PlaybackConverter(ENGINE, OUTER, S)
        play.position = pos
        flags = _lib.PROC_RATECVT_PAIR if pair else 0
        call = proc.process_samples_at_device if whole else proc.process_samples_at_any_device
        ms = hip.timed(lambda: call(None, fmt, "stream", 0, 0, None, d_out, fmt, "stream", q, q, play, stream=None, flags=flags), a.reps)
        name = proc.last_tx_kernel
        play.close()
        proc.close()
        return ms, name

    for fmt in FORMATS:
        for q, pos, whole in [(QUANTUM, p, False) for p in POSITIONS] + [(WHOLE, 0, True)]:
            (pair_a, pair_name), (fused, fused_name), (pair_b, _) = series(q, fmt, pos, True, whole), series(q, fmt, pos, False, whole), series(q, fmt, pos, True, whole)
            ma, mf, mb = (float(np.median(m)) for m in (pair_a, fused, pair_b))
            emit(dict(part="kernel", format=fmt, layout="stream", streams=S, quantum=q, from_position=pos, up=UP, down=DOWN, taps=TAPS,
                      form="whole periods" if whole else "any length", fused=fused_name, fused_ms=_stats(fused), pair=pair_name, pair_a=_stats(pair_a),
                      pair_b=_stats(pair_b), pair_spread_ms=round(abs(ma - mb), 4), fused_over_pair=round(mf / (0.5 * (ma + mb)), 4),
                      faster_than_pair=bool(mf < min(ma, mb) - abs(ma - mb))))
    eng.device_free(d_out)
    eng.close()


def host_rows(a, wm, emit, whole):
    S = a.streams
    q = WHOLE if whole else QUANTUM
    eng = wm.FSKEngine(S, BELL)
    for fmt in FORMATS:
        dtype = sr.DTYPES[fmt]
        row = dict(part="whole" if whole else "host", format=fmt, layout="stream", streams=S, quantum=q, up=UP, down=DOWN, taps=TAPS,
                   call="fskhip_processor_process_ratecvt_host" if whole else "fskhip_processor_process_ratecvt_any_host")
        for sides in (("both",) if whole else ("rx", "tx", "both")):
            proc = pending(wm, eng, S)
            cap, play = wm.CaptureConverter(OUTER, ENGINE, S), wm.PlaybackConverter(ENGINE, OUTER, S)
            x = wm.pinned_empty((S, q), dtype)
            x[:] = sr.silence(fmt)
            call = proc.process_samples_at if whole else proc.process_samples_at_any
            ms = []
            for r in range(a.reps + WARMUP):
                t0 = time.perf_counter()
                call(x if sides != "tx" else None, fmt, "stream", cap, q if sides != "rx" else 0, fmt, "stream", play)
                t1 = time.perf_counter()
                if r >= WARMUP:
                    ms.append((t1 - t0) * 1e3)
            row[sides + "_ms"] = _stats(ms)
            row[sides + "_us_per_sample"] = round(float(np.median(ms)) * 1e3 / q, 2)
            if sides != "rx":
                row["tx_path"] = proc.last_tx_kernel
            for h in (cap, play, proc):
                h.close()
        emit(row)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "processor_ratecvt_any_bench.jsonl"))
    ap.add_argument("--streams", type=int, default=262144)
    ap.add_argument("--parts", default="kernel,host,whole")
    ap.add_argument("--step", default=None, help="(internal) the part this process runs")
    a = ap.parse_args()
    if a.step is None:
        open(a.out, "w").close()
        for part in a.parts.split(","):
            cmd = ["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--out", a.out,
                   "--streams", str(a.streams), "--step", part]
            rc = subprocess.call(cmd)
            if rc != 0:     # a step that failed or ran out of time ends the run: nothing more is started on the device
                print("step %s ended with status %d" % (part, rc), flush=True)
                sys.exit(rc)
        sys.exit(0)
    import webaudio_modem_amd as wm

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        with open(a.out, "a") as fh:
            fh.write(line + "\n")

    if a.step == "kernel":
        kernel_rows(a, wm, emit)
    else:
        host_rows(a, wm, emit, a.step == "whole")


if __name__ == "__main__":
    main()
