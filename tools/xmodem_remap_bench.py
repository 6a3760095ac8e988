"""fskhip_xmodem_{tx,recv}_remap / _snapshot / _restore at the size the XModem rows are quoted at: 262 144 streams (fp32 engines,
rx_capacity 1024).  For each of the sender (tx) and the file receiver (recv), with files of 128 bytes and of 4 KB held by 1 %,
10 % and 100 % of the streams, under one random permutation map:
  (a) remap        the new call into a freshly created handle;
  (b) by hand      what a host does without it for the same effect -- tx: send() of the host's permuted files + set_state();
                   recv: files(), then set_files() and set_state() of the permuted lists;
  (c) d2d          a device-to-device copy of the same live bytes (files + words), in the same run.
and snapshot / from_snapshot against a page-locked host<->device copy of the image's bytes.  Every (a) result is checked against (b)'s
(state words, files or image) before a time is taken.  Timing: wall clock around each synchronous call, after two warm-up calls,
median of --reps; (a), (b) and from_snapshot each include creating and closing the destination handle, alike.  Writes one JSON line per case to --out (default profiles/xmodem_remap_bench.jsonl).

usage: python tools/xmodem_remap_bench.py [--streams 262144] [--reps 7] [--out FILE] [--kinds tx,recv] [--sizes 128,4096] [--shares 1,10,100]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "xmodem_remap_bench.jsonl"))
    ap.add_argument("--kinds", default="tx,recv")
    ap.add_argument("--sizes", default="128,4096")
    ap.add_argument("--shares", default="1,10,100")
    a = ap.parse_args()
    import webaudio_modem_amd as wm
    from webaudio_modem_amd import _lib
    L = _lib.lib()
    S = a.streams
    rng = np.random.default_rng(0xBE7C)
    perm = rng.permutation(S).astype(np.int64)
    eng = wm.FSKEngine(S, {}, precision=wm.PRECISION_F32)
    procs = [wm.FSKProcessorBatch(eng, rx_capacity=1024) for _ in range(2)]   # the handles never touch the processor: two serve every case
    src_proc, dst_proc = procs

    def dev_buf(n):
        p = C.c_void_p()
        _lib.check(L.fskhip_device_malloc(eng._h, max(n, 16), C.byref(p)))
        return p

    def hip_runtime():
        """the HIP runtime libfskhip.so has loaded into this process (the library offers host<->device copies only, and a copy through
        another package's runtime would not be the same device context)"""
        with open("/proc/self/maps") as fh:
            paths = sorted({line.split()[-1] for line in fh if "libamdhip64.so" in line and "/torch/" not in line})
        if not paths:
            raise RuntimeError("no libamdhip64.so is mapped into this process: the device-to-device comparator needs the HIP runtime libfskhip.so uses")
        hip = C.CDLL(paths[0])
        hip.hipMemcpy.argtypes, hip.hipMemcpy.restype = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], C.c_int
        hip.hipDeviceSynchronize.argtypes, hip.hipDeviceSynchronize.restype = [], C.c_int
        return hip

    def d2d_ms(n):
        """a device-to-device copy of n bytes on the same device, synchronised"""
        hip = hip_runtime()
        x, y = dev_buf(n), dev_buf(n)

        def go():
            assert hip.hipMemcpy(y, x, max(n, 16), 3) == 0 and hip.hipDeviceSynchronize() == 0   # 3: hipMemcpyDeviceToDevice
        t = median_ms(go, a.reps)
        L.fskhip_device_free(eng._h, x)
        L.fskhip_device_free(eng._h, y)
        return t

    def pinned_ms(n):
        """page-locked host -> device and device -> host copies of n bytes"""
        h = C.c_void_p()
        _lib.check(L.fskhip_host_alloc(max(n, 16), C.byref(h)))
        d = dev_buf(n)
        up = median_ms(lambda: _lib.check(L.fskhip_memcpy_h2d(eng._h, d, h, max(n, 16))), a.reps)
        down = median_ms(lambda: _lib.check(L.fskhip_memcpy_d2h(eng._h, h, d, max(n, 16))), a.reps)
        L.fskhip_device_free(eng._h, d)
        L.fskhip_host_free(h)
        return up, down

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as out:
        for kind in a.kinds.split(","):
            for size in (int(x) for x in a.sizes.split(",")):
                for share in (int(x) for x in a.shares.split(",")):
                    has = rng.random(S) < share / 100.0
                    files = [bytes(rng.integers(0, 256, size, dtype=np.uint8)) if h else (None if kind == "tx" else b"") for h in has]
                    live = int(has.sum()) * size
                    if kind == "tx":
                        src = wm.XModemSenderBatch(src_proc, 128, 10)
                        src.send(files, mask=has)
                        make = lambda: wm.XModemSenderBatch(dst_proc, 128, 10)   # noqa: E731
                        words = 6
                    else:
                        src = wm.XModemFileReceiverBatch(src_proc, size, 10)
                        src.set_files(files)
                        make = lambda: wm.XModemFileReceiverBatch(dst_proc, size, 10)   # noqa: E731
                        words = 7
                    state = src.state()
                    pfiles = [files[p] for p in perm]
                    pstate = {k: v[perm] for k, v in state.items()}
                    phas = has[perm]

                    def by_hand():
                        d = make()
                        if kind == "tx":
                            d.send(pfiles, mask=phas)
                            d.set_state(**pstate)
                        else:
                            got = src.files()
                            d.set_files([got[p] for p in perm])
                            d.set_state(**{k: v for k, v in pstate.items() if k != "file_len"})
                        return d

                    def remap():
                        return src.remapped(dst_proc, perm)
                    want, got = by_hand(), remap()
                    assert want.snapshot() == got.snapshot(), "the remap and the by-hand path disagree"
                    want.close()
                    got.close()

                    def timed(fn):
                        def go():
                            fn().close()
                        return median_ms(go, a.reps)
                    image = src.snapshot()
                    t_remap, t_hand = timed(remap), timed(by_hand)
                    t_d2d = d2d_ms(live + 4 * words * S)
                    t_snap = median_ms(lambda: src.snapshot(), a.reps)
                    t_rest = timed(lambda: type(src).from_snapshot(dst_proc, image))
                    up, down = pinned_ms(len(image))
                    row = dict(kind=kind, streams=S, file_bytes=size, share_percent=share, live_bytes=live, image_bytes=len(image), reps=a.reps,
                               remap_ms=t_remap, by_hand_ms=t_hand, d2d_copy_ms=t_d2d, snapshot_ms=t_snap, restore_ms=t_rest, pinned_h2d_ms=up, pinned_d2h_ms=down)
                    out.write(json.dumps(row) + "\n")
                    out.flush()
                    print(json.dumps(row))
                    src.close()
    for p in procs:
        p.close()
    eng.close()


if __name__ == "__main__":
    main()
