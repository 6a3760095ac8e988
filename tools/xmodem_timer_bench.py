"""The resident XModem wait timers' timed poll (fskhip_xmodem_recv_poll_timed_host) against what a host does today for the same
effect, at the size the processor row is quoted at: 262 144 streams, rx_capacity 1024 (fp32 engines, Bell-202).  Every stream is a
file receiver that waits for packet 1; in 0.1 %, 1 %, 10 % and 100 % of the streams the packet (128 payload bytes) has arrived.
One source processor is brought to each state by restoring an image crafted from the documented layout (tools/xmodem_rx_bench.py's
craft); every timed call works on a clone of it (fskhip_processor_remap with the identity into a freshly created processor) with a
fresh file receiver over it (state_set, not timed), all variants in one run on the same state:
  timed     XModemTimers' one fskhip_xmodem_recv_poll_timed_host into lists that fit: fire, the poll, arm
  host      the same effect with the timers on the host: the receiver's state words, the processor's pending flags and ring
            lengths read back, the contract's fire rule in numpy over host arrays of waited / mark, the timeout mask uploaded with
            the plain fskhip_xmodem_recv_poll_host, the state words and ring lengths read back again and the arm rule in numpy
  plain     the plain fskhip_xmodem_recv_poll_host with no timers at all: what the two added launches cost is timed - plain
The timed / host pair is timed twice in the same run, in the order timed, host, timed, host, then plain; each figure is the median
of --reps after two warm-ups, wall clock around the synchronous calls, host buffers allocated beforehand, one process.  The
variants' events and the timers' words are compared before anything is timed.

usage: python tools/xmodem_timer_bench.py [--streams 262144] [--rx-capacity 1024] [--reps 7] [--out profiles/xmodem_timer_bench.jsonl]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from drain_bench import CFG, median_ms   # noqa: E402
from xmodem_rx_bench import craft        # noqa: E402
from xmodem_recv_bench import crc16      # noqa: E402

SOH = 0x01
PAYLOAD, FILE_CAP, TIMEOUT, ELAPSED = 128, 256, 144000, 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=262144)
    ap.add_argument("--rx-capacity", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import webaudio_modem_amd as wm
    from webaudio_modem_amd import _lib
    from webaudio_modem_amd.xmodem import RECV_EVENT_DTYPE
    L = _lib.lib()
    S, cap = a.streams, a.rx_capacity
    rng = np.random.default_rng(29)
    ident = np.arange(S, dtype=np.int64)
    eng_src = wm.FSKEngine(S, CFG, precision=wm.PRECISION_F32)
    eng_dst = wm.FSKEngine(S, CFG, precision=wm.PRECISION_F32)
    payload = bytes(rng.integers(0, 256, PAYLOAD, dtype=np.uint8))
    crc = crc16(payload)
    pkt = bytes([SOH, 1, 254, PAYLOAD]) + payload + bytes([crc >> 8, crc & 0xFF])
    words = {"state": np.full(S, 2, np.uint32), "expected": np.ones(S, np.uint32), "packets_sent": np.ones(S, np.uint32)}
    rows = []
    ne = C.c_uint32(0)

    for name, frac in (("0.1%", 0.001), ("1%", 0.01), ("10%", 0.1), ("100%", 1.0)):
        busy = np.flatnonzero(rng.random(S) < frac) if frac < 1.0 else np.arange(S)
        blob = craft(S, cap, {int(s): pkt for s in busy}, rng)
        src = wm.FSKProcessorBatch(eng_src, rx_capacity=cap)
        _lib.check(L.fskhip_processor_restore(src._h, blob.ctypes.data, blob.nbytes, ident.ctypes.data, S))
        del blob
        n_busy = len(busy)
        streams, events = np.zeros(max(n_busy, 1), np.uint32), np.zeros(max(n_busy, 1), RECV_EVENT_DTYPE)
        state, held, live = np.zeros(S, np.uint32), np.zeros(S, np.uint32), np.zeros(S, np.uint32)
        pos, total, done, pend = np.zeros(S, np.uint32), np.zeros(S, np.uint32), np.zeros(S, np.uint32), np.zeros(S, np.uint8)
        flag = np.zeros(S, np.uint8)

        def clone(timed):
            d = wm.FSKProcessorBatch(eng_dst, rx_capacity=cap)
            _lib.check(L.fskhip_processor_remap(d._h, src._h, ident.ctypes.data, S))
            rx = wm.XModemFileReceiverBatch(d, FILE_CAP, 10)
            rx.set_state(**words)
            t = wm.XModemTimers(rx, TIMEOUT) if timed else None
            return d, rx, t, np.zeros(S, np.uint32), np.zeros(S, np.uint32)   # (and the host's own waited / mark)

        def close(ctx):
            if ctx[2] is not None:
                ctx[2].close()
            ctx[1].close()
            ctx[0].close()

        def run_timed(ctx):
            _lib.check(L.fskhip_xmodem_recv_poll_timed_host(ctx[2]._h, ELAPSED, None, None, streams.ctypes.data, events.ctypes.data, len(streams), C.byref(ne)))
            return ne.value

        def run_plain(ctx):
            _lib.check(L.fskhip_xmodem_recv_poll_host(ctx[1]._h, None, None, None, streams.ctypes.data, events.ctypes.data, len(streams), C.byref(ne)))
            return ne.value

        def run_host(ctx):
            d, rx, _, waited, mark = ctx
            # fire: what the rule reads, read back
            _lib.check(L.fskhip_xmodem_recv_state_get(rx._h, state.ctypes.data, None, None, None, None, None, None))
            _lib.check(L.fskhip_processor_tx_state_host(d._h, pos.ctypes.data, total.ctypes.data, pend.ctypes.data, done.ctypes.data))
            _lib.check(L.fskhip_processor_rx_length_host(d._h, held.ctypes.data))
            sel = state != 0
            pending = sel & (pend != 0)
            wait = sel & ~pending
            begins = wait & (((mark & 4) != 0) | (state == 1) | (state == 3))
            runs = wait & ~begins
            mark[pending] |= 4
            waited[begins] = 0
            mark[begins] = 0
            waited[runs] = np.minimum(waited[runs].astype(np.uint64) + ELAPSED, 0xFFFFFFFF).astype(np.uint32)
            flag[:] = wait & (waited >= TIMEOUT)
            _lib.check(L.fskhip_xmodem_recv_poll_host(rx._h, None, flag.ctypes.data, None, streams.ctypes.data, events.ctypes.data, len(streams), C.byref(ne)))
            n = ne.value
            # arm: the words after the poll, read back
            _lib.check(L.fskhip_xmodem_recv_state_get(rx._h, state.ctypes.data, None, None, None, None, None, None))
            _lib.check(L.fskhip_processor_rx_length_host(d._h, live.ctypes.data))
            listed = np.zeros(S, bool)
            listed[streams[:n]] = True
            stage = np.where(live == 0, 0, np.where(live < 4, 1, 2)).astype(np.uint32)
            idle = sel & (state == 0)
            w = wait & ~idle
            waited[w & (listed | (live < held) | (stage > (mark & 3)))] = 0
            mark[w] = (mark[w] & ~np.uint32(3)) | stage[w]
            waited[idle] = 0
            mark[idle] = 0
            return n

        # the same events and the same timers: checked before anything is timed
        c1, c2 = clone(True), clone(False)
        n1 = run_timed(c1)
        s1, e1 = streams[:n1].copy(), events[:n1].copy()
        n2 = run_host(c2)
        assert n1 == n2 == n_busy and np.array_equal(s1, streams[:n2]) and e1.tolist() == events[:n2].tolist() and np.array_equal(s1, busy)
        t = c1[2].state()
        assert np.array_equal(t["waited"], c2[3]) and np.array_equal(t["mark"], c2[4])
        assert np.array_equal(c1[0].tx_state()["pendingModulation"], c2[0].tx_state()["pendingModulation"])
        close(c1)
        close(c2)

        timed_ms, host_ms = [], []
        for _ in range(2):   # the pair twice in the same run
            timed_ms.append(median_ms(run_timed, a.reps, lambda: clone(True), close))
            host_ms.append(median_ms(run_host, a.reps, lambda: clone(False), close))
        plain_ms = median_ms(run_plain, a.reps, lambda: clone(False), close)
        row = dict(case=name, streams=S, rx_capacity=cap, n_answering=n_busy, timed_poll_ms=[round(x, 3) for x in timed_ms],
                   host_timers_ms=[round(x, 3) for x in host_ms], plain_poll_ms=round(plain_ms, 3), reps=a.reps)
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
