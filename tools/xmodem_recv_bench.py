"""The resident XModem file receiver's poll (fskhip_xmodem_recv_poll_host) against the host loop it replaces, at the size the
processor row is quoted at: 262 144 streams, rx_capacity 1024 (fp32 engines, Bell-202).  Every stream is a receiver that waits for
packet 1; in 0.1 %, 1 %, 10 % and 100 % of the streams the packet (128 payload bytes) has arrived, behind one to three noise bytes.
One source processor is brought to each state by restoring an image crafted from the documented layout (tools/xmodem_rx_bench.py's
craft); every timed call works on a clone of it (fskhip_processor_remap with the identity into a freshly created processor), both
variants in one run on the same state:
  poll      a file receiver over the clone (state_set, not timed), then its one fskhip_xmodem_recv_poll_host into lists that fit
  host      what a host does per poll without it: XModemReceiverBatch's fskhip_xmodem_rx_poll_host into lists that fit, one call as
            XModemReceiverBatch.poll() makes in its steady state (the accepted payloads cross to the host), the one-byte control
            payloads built in numpy from the result records, and fskhip_processor_modulate_host with their mask
The pair is timed twice in the same run, in the order poll, host, poll, host; each figure is the median of --reps after two
warm-ups, wall clock around the synchronous calls, host buffers allocated beforehand, one process.  Every timed call is the first
poll of a fresh handle: the existing receiver's first poll grows its device staging, which a steady-state host pays once, so those
three allocations are also timed on their own (host_first_poll_alloc_ms) for the reader to take off host_loop_ms.  The two variants' pending
modulations (tx_state) and ring lengths are compared before anything is timed.  Then files(): the one packed copy of every file at
the end, against the sum of payload bytes the existing receiver returned poll by poll (reported as bytes, and files() as time).

usage: python tools/xmodem_recv_bench.py [--streams 262144] [--rx-capacity 1024] [--reps 7] [--out profiles/xmodem_recv_bench.jsonl]"""
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

ACK, NAK, SOH = 0x06, 0x15, 0x01
PAYLOAD, FILE_CAP = 128, 256


def crc16(data):
    c = 0xFFFF
    for b in data:
        c ^= b << 8
        for _ in range(8):
            c = ((c << 1) ^ 0x1021) & 0xFFFF if c & 0x8000 else (c << 1) & 0xFFFF
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=262144)
    ap.add_argument("--rx-capacity", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import webaudio_modem_amd as wm
    from webaudio_modem_amd import _lib
    from webaudio_modem_amd.xmodem import RECV_EVENT_DTYPE, RESULT_DTYPE
    L = _lib.lib()
    S, cap = a.streams, a.rx_capacity
    rng = np.random.default_rng(23)
    ident = np.arange(S, dtype=np.int64)
    eng_src = wm.FSKEngine(S, CFG, precision=wm.PRECISION_F32)
    eng_dst = wm.FSKEngine(S, CFG, precision=wm.PRECISION_F32)
    payload = bytes(rng.integers(0, 256, PAYLOAD, dtype=np.uint8))
    crc = crc16(payload)
    pkt = bytes([SOH, 1, 254, PAYLOAD]) + payload + bytes([crc >> 8, crc & 0xFF])
    words = {"state": np.full(S, 2, np.uint32), "expected": np.ones(S, np.uint32), "packets_sent": np.ones(S, np.uint32)}
    rows = []
    ne, nb = C.c_uint32(0), C.c_uint32(0)

    for name, frac in (("0.1%", 0.001), ("1%", 0.01), ("10%", 0.1), ("100%", 1.0)):
        busy = np.flatnonzero(rng.random(S) < frac) if frac < 1.0 else np.arange(S)
        lines = {int(s): bytes(rng.integers(0x20, 0x80, int(rng.integers(1, 4)), dtype=np.uint8)) + pkt for s in busy}
        blob = craft(S, cap, lines, rng)
        src = wm.FSKProcessorBatch(eng_src, rx_capacity=cap)
        _lib.check(L.fskhip_processor_restore(src._h, blob.ctypes.data, blob.nbytes, ident.ctypes.data, S))
        del blob
        n_busy = len(busy)
        p_streams, p_events = np.zeros(max(n_busy, 1), np.uint32), np.zeros(max(n_busy, 1), RECV_EVENT_DTYPE)
        r_streams, r_results = np.zeros(max(n_busy, 1), np.uint32), np.zeros(max(n_busy, 1), RESULT_DTYPE)
        r_offsets, r_data = np.zeros(n_busy + 2, np.uint32), np.zeros(max(n_busy * PAYLOAD, 1), np.uint8)
        ctl, lens, mask = np.zeros((S, 1), np.uint8), np.zeros(S, np.uint32), np.zeros(S, np.uint8)

        def clone(resident):
            d = wm.FSKProcessorBatch(eng_dst, rx_capacity=cap)
            _lib.check(L.fskhip_processor_remap(d._h, src._h, ident.ctypes.data, S))
            if resident:
                rx = wm.XModemFileReceiverBatch(d, FILE_CAP, 10)
                rx.set_state(**words)
            else:
                rx = wm.XModemReceiverBatch(d)
            return d, rx

        def close(ctx):
            ctx[1].close()
            ctx[0].close()

        def run_poll(ctx):
            _lib.check(L.fskhip_xmodem_recv_poll_host(ctx[1]._h, None, None, None, p_streams.ctypes.data, p_events.ctypes.data, len(p_streams), C.byref(ne)))
            return ne.value

        def run_host(ctx):
            poll = L.fskhip_xmodem_rx_poll_host
            _lib.check(poll(ctx[1]._h, None, r_streams.ctypes.data, r_results.ctypes.data, r_offsets.ctypes.data, len(r_streams), r_data.ctypes.data, len(r_data),
                            C.byref(ne), C.byref(nb)))   # lists that fit, one call: XModemReceiverBatch.poll() in its steady state
            n = ne.value
            if n == 0:
                return 0, 0
            res, who = r_results[:n], r_streams[:n]
            bad = (res["status"] >= 3)                                # the three errors: NAK; everything else listed here: ACK
            mask[:] = 0
            mask[who] = 1
            lens[:] = 0
            lens[who] = 1
            ctl[who, 0] = np.where(bad, NAK, ACK)
            _lib.check(L.fskhip_processor_modulate_host(ctx[0]._h, ctl.ctypes.data, lens.ctypes.data, 1, mask.ctypes.data))
            return n, nb.value

        # the same state, the same modulations: checked before anything is timed
        c1, c2 = clone(True), clone(False)
        n_events = run_poll(c1)
        assert n_events == n_busy and np.array_equal(p_streams[:n_events], busy) and (p_events[:n_events]["accepted_len"] == PAYLOAD).all()
        n_host, host_bytes = run_host(c2)
        assert n_host == n_busy and host_bytes == n_busy * PAYLOAD
        t1, t2 = c1[0].tx_state(), c2[0].tx_state()
        assert np.array_equal(t1["pendingModulation"], t2["pendingModulation"]) and np.array_equal(t1["totalSamples"], t2["totalSamples"])
        assert t1["pendingModulation"].sum() == n_busy and not c1[0].rx_lengths().any() and not c2[0].rx_lengths().any()
        # files(): one packed copy at the end
        sel, offsets, total = busy.astype(np.uint32), np.zeros(n_busy + 1, np.uint64), C.c_uint64(0)
        data = np.zeros(max(n_busy * PAYLOAD, 1), np.uint8)

        def run_files(_):
            _lib.check(L.fskhip_xmodem_recv_files_host(c1[1]._h, sel.ctypes.data, n_busy, offsets.ctypes.data, data.ctypes.data, data.nbytes, C.byref(total)))
        run_files(None)
        assert total.value == host_bytes and bytes(data[:PAYLOAD]) == payload and bytes(data[total.value - PAYLOAD:total.value]) == payload
        files_ms = median_ms(run_files, a.reps, lambda: None, lambda _: None)
        close(c1)
        close(c2)

        # every timed call is the first poll of a fresh handle over a fresh clone.  The resident handle sized its staging at create;
        # the existing receiver's first poll grows its own (three device allocations), which a host in its steady state does not
        # pay again: timed on their own here, to be taken off host_loop_ms by the reader
        sizes = (n_busy * PAYLOAD + 1, 4 * (2 * n_busy + 1), RESULT_DTYPE.itemsize * (n_busy + 1))

        def run_alloc(ptrs):
            for nbytes in sizes:
                q = C.c_void_p()
                _lib.check(L.fskhip_device_malloc(eng_dst._h, nbytes, C.byref(q)))
                ptrs.append(q)

        def free_all(ptrs):   # (outside the timing)
            for q in ptrs:
                L.fskhip_device_free(eng_dst._h, q)
        alloc_ms = median_ms(run_alloc, a.reps, list, free_all)
        poll_ms, host_ms = [], []
        for _ in range(2):   # the pair twice in the same run
            poll_ms.append(median_ms(run_poll, a.reps, lambda: clone(True), close))
            host_ms.append(median_ms(run_host, a.reps, lambda: clone(False), close))
        row = dict(case=name, streams=S, rx_capacity=cap, n_answering=n_busy, payload_bytes=host_bytes, poll_ms=[round(x, 3) for x in poll_ms],
                   host_loop_ms=[round(x, 3) for x in host_ms], host_first_poll_alloc_ms=round(alloc_ms, 3), files_ms=round(files_ms, 3), reps=a.reps)
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
