"""What FSKProcessorBatchSharded's fan-out costs: the host call of one streaming quantum (128 samples in, 128 out, a modulation
pending on every stream) through the sharded class against the plain FSKProcessorBatch at the same size in the same run, and
`remapped` under a random permutation against the single class's.  262 144 streams, fp32 engines, float32 stream-major and
mu-law interleaved frames.  Wall clock around the synchronous call; median of --reps after 2 warm-up quanta; the pair (plain,
sharded) is timed twice, plain - sharded - plain - sharded, and both medians of each are reported: their spread is the run's noise.

Rows (profiles/processor_sharded_bench.jsonl):
  fanout   devices [0] and [0, 0] against the plain class: the fan-out's cost on one device
  devices  every device of the box, where it has more than one (else the row says so and nothing is claimed)
  remap    sharded.remapped(random permutation) on [0, 0] against FSKProcessorBatch.remapped

Every step runs in a child process of its own under its own time limit (--step-timeout seconds); the tool stops at the first
step that fails or runs out of time, and says which.

usage: python tools/processor_sharded_bench.py [--streams 262144] [--reps 7] [--step-timeout 240] [--out profiles/processor_sharded_bench.jsonl]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG = dict(baudRate=1200, markFrequency=1200, spaceFrequency=2200)
N = 128
FORMATS = [("f32", "stream"), ("mulaw", "sample")]


def quantum_ms(batch, fmt, layout, x, out, reps):
    """median wall clock of one quantum (both sides) after two warm-ups"""
    times = []
    for r in range(reps + 2):
        t0 = time.perf_counter()
        batch.process_samples(x, fmt, layout, N, fmt, layout, out=out)
        t1 = time.perf_counter()
        if r >= 2:
            times.append((t1 - t0) * 1e3)
    return float(np.median(times))


def make(wm, S, devices):
    """the plain class (devices None) or the sharded one, a modulation of 11 bytes pending on every stream (5 600 samples: longer
    than every quantum timed here)"""
    if devices is None:
        b = wm.FSKProcessorBatch(wm.FSKEngine(S, CFG, precision=wm.PRECISION_F32))
    else:
        b = wm.FSKProcessorBatchSharded(S, CFG, devices=devices, precision=wm.PRECISION_F32)
    b.modulate([b"hello world"] * S)
    return b


def close(b):
    eng = getattr(b, "engine", None)
    b.close()
    if eng is not None:
        eng.close()


def arrays(wm, S, fmt, layout, rng):
    dt = wm.engine._FORMAT_DTYPE[wm.SAMPLE_FORMATS[fmt]]
    shape = (S, N) if layout == "stream" else (N, S)
    x = (rng.standard_normal(shape) * 0.05).astype(np.float32) if fmt == "f32" else rng.integers(0, 256, shape).astype(dt)
    return x, np.zeros(shape, dt)


def step_pair(wm, S, reps, devices, case):
    rows = []
    rng = np.random.default_rng(11)
    for fmt, layout in FORMATS:
        x, out = arrays(wm, S, fmt, layout, rng)
        plain, sharded = make(wm, S, None), make(wm, S, devices)
        try:
            ms = [quantum_ms(b, fmt, layout, x, out, reps) for b in (plain, sharded, plain, sharded)]
        finally:
            close(plain)
            close(sharded)
        rows.append(dict(case=case, devices=devices, streams=S, quantum=N, format=fmt, layout=layout, reps=reps,
                         plain_ms=[round(ms[0], 3), round(ms[2], 3)], sharded_ms=[round(ms[1], 3), round(ms[3], 3)]))
    return rows


def step_remap(wm, S, reps):
    rng = np.random.default_rng(13)
    m = rng.permutation(S).astype(np.int64)
    plain, sharded = make(wm, S, None), make(wm, S, [0, 0])
    x, out = arrays(wm, S, "f32", "stream", rng)
    try:
        for b in (plain, sharded):       # (a few quanta, so that the modulations are under way)
            quantum_ms(b, "f32", "stream", x, out, 1)
        ms = []
        for b in (plain, sharded, plain, sharded):
            times = []
            for r in range(reps + 2):
                t0 = time.perf_counter()
                nxt = b.remapped(m)
                t1 = time.perf_counter()
                close(nxt)
                if r >= 2:
                    times.append((t1 - t0) * 1e3)
            ms.append(float(np.median(times)))
    finally:
        close(plain)
        close(sharded)
    return [dict(case="remap", devices=[0, 0], streams=S, map="random permutation", reps=reps, plain_remapped_ms=[round(ms[0], 1), round(ms[2], 1)],
                 sharded_remapped_ms=[round(ms[1], 1), round(ms[3], 1)])]


def run_step(name, S, reps):
    import webaudio_modem_amd as wm
    from webaudio_modem_amd import _lib
    if name == "fanout-1":
        return step_pair(wm, S, reps, [0], "fanout")
    if name == "fanout-2":
        return step_pair(wm, S, reps, [0, 0], "fanout")
    if name == "devices":
        n = int(_lib.lib().fskhip_device_count())
        if n < 2:
            return [dict(case="devices", devices=list(range(n)), note="the box has one device: not run")]
        return step_pair(wm, S, reps, list(range(n)), "devices")
    if name == "remap":
        return step_remap(wm, S, reps)
    raise SystemExit("unknown step %r" % name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=262144)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--steps", default="fanout-1,fanout-2,devices,remap")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "processor_sharded_bench.jsonl"))
    ap.add_argument("--step", default=None, help="(internal) run this one step in this process and print its rows")
    a = ap.parse_args()
    if a.step:
        for row in run_step(a.step, a.streams, a.reps):
            print("ROW " + json.dumps(row), flush=True)
        return 0
    rows = []
    for name in a.steps.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--streams", str(a.streams), "--reps", str(a.reps)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
        except subprocess.TimeoutExpired:
            print("step %s ran out of its %d s: stopping here" % (name, a.step_timeout), file=sys.stderr)
            break
        if r.returncode != 0:
            print("step %s failed (exit status %d): stopping here\n%s" % (name, r.returncode, r.stderr[-2000:]), file=sys.stderr)
            break
        for line in r.stdout.splitlines():
            if line.startswith("ROW "):
                rows.append(json.loads(line[4:]))
                print(line[4:], flush=True)
    else:
        name = None
    if rows:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            for row in rows:
                fh.write(json.dumps(row) + "\n")
    return 0 if name is None else 1


if __name__ == "__main__":
    sys.exit(main())
