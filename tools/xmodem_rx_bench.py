"""The resident XModem receiver's poll (fskhip_xmodem_rx_poll_host) against the two ways a host receives XModem over a live batch
without it, at the size the processor row is quoted at: 262 144 streams, rx_capacity 1024 (fp32 engines, Bell-202).
Cases: 0, 0.1 %, 1 %, 10 % and 100 % of the streams hold one to three packets of 16..128 payload bytes with a few noise bytes between
them; a tenth of the busy streams are cut mid-packet.  One source processor is brought to each state by restoring an image crafted
from the documented layout (tools/drain_bench.py's craft); every timed call works on a clone of it (fskhip_processor_remap with the
identity into a freshly created processor), all variants in one run on the same state:
  poll      a fresh receiver's fskhip_xmodem_rx_poll_host as a first call makes it: the size query, then the poll into buffers of
            the reported size -- the scan and totals passes run twice (poll_ms)
  poll_fit  the same receiver's one call into buffers that already fit, as XModemReceiverBatch.poll makes every call after it has
            grown its lists: the passes run once (poll_fit_ms)
  dense     (a) fskhip_processor_rx_drain_host into an [S][rx_capacity] slab + fskhip_xmodem_scan_host over the slab
  sparse    (b) fskhip_processor_rx_drain_sparse_host + packing the drained spans into rows on the host + fskhip_xmodem_scan_host
            over the active rows only
The payloads of all variants are compared before anything is timed (for the streams that are not cut: a burst scan charges a cut
packet as truncated, which is the difference the receiver exists for).  Timing: wall clock around the synchronous calls, host
buffers allocated beforehand, median of --reps after two warm-ups, one process.

usage: python tools/xmodem_rx_bench.py [--streams 262144] [--rx-capacity 1024] [--reps 7] [--out profiles/xmodem_rx_bench.jsonl]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from drain_bench import CFG, FIXED, HEADER, checksum, median_ms   # noqa: E402


def crc16(data):
    crc = 0xFFFF
    for b in data:
        crc ^= b << 8
        for _ in range(8):
            crc = ((crc << 1) ^ 0x1021) & 0xFFFF if crc & 0x8000 else (crc << 1) & 0xFFFF
    return crc


def line_of(rng, cap):
    """(bytes, accepted payload, cut): one to three packets from sequence 1, noise between them, a tenth cut inside the last packet"""
    out, pay = bytearray(), bytearray()
    n_packets = int(rng.integers(1, 4))
    cut = rng.random() < 0.1
    for k in range(n_packets):
        out += bytes(rng.integers(5, 256, int(rng.integers(0, 4)), dtype=np.uint8))   # (5..255: neither SOH nor EOT)
        body = bytes(rng.integers(0, 256, int(rng.integers(16, 129)), dtype=np.uint8))
        crc = crc16(body)
        pkt = bytes([1, k + 1, 254 - k, len(body)]) + body + bytes([crc >> 8, crc & 0xFF])
        if len(out) + len(pkt) > cap:
            break
        if cut and k == n_packets - 1:
            out += pkt[:int(rng.integers(1, len(pkt)))]
            return bytes(out), bytes(pay), True
        out += pkt
        pay += body
    return bytes(out), bytes(pay), False


def craft(S, cap, lines, rng):
    """a canonical processor image: stream s holds lines[s] (a dict stream -> bytes; the others are empty) from a random readIndex"""
    rb = FIXED + ((cap + 15) & ~15)
    blob = np.zeros(HEADER + S * rb, np.uint8)
    blob[:HEADER].view("<u4")[:8] = [0x504B5346, 1, HEADER, rb, S, cap, 0, 0]
    rec = blob[HEADER:].reshape(S, rb)
    read = rng.integers(0, cap, S)
    lengths = np.zeros(S, np.int64)
    for s, b in lines.items():
        lengths[s] = len(b)
        rec[s, FIXED + (read[s] + np.arange(len(b))) % cap] = np.frombuffer(b, np.uint8)
    words = np.zeros((S, 4), np.uint32)
    words[:, 0], words[:, 1], words[:, 2] = (read + lengths) % cap, read, lengths
    rec[:, :16] = words.view(np.uint8)
    blob[32:40].view("<u8")[0] = checksum(blob)
    return blob


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=262144)
    ap.add_argument("--rx-capacity", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import webaudio_modem_amd as wm
    from webaudio_modem_amd import _lib
    from webaudio_modem_amd.xmodem import RESULT_DTYPE
    L = _lib.lib()
    S, cap = a.streams, a.rx_capacity
    rng = np.random.default_rng(12)
    ident = np.arange(S, dtype=np.int64)
    eng_src = wm.FSKEngine(S, CFG, precision=wm.PRECISION_F32)
    eng_dst = wm.FSKEngine(S, CFG, precision=wm.PRECISION_F32)
    rows = []
    dense_out, dense_counts = np.zeros((S, cap), np.uint8), np.zeros(S, np.uint32)
    dense_data, dense_res, ones = np.zeros((S, cap), np.uint8), np.zeros(S, RESULT_DTYPE), np.ones(S, np.uint32)
    ne, nb = C.c_uint32(0), C.c_uint32(0)

    for name, frac in (("idle", 0.0), ("0.1%", 0.001), ("1%", 0.01), ("10%", 0.1), ("100%", 1.0)):
        busy = np.flatnonzero(rng.random(S) < frac) if frac < 1.0 else np.arange(S)
        made = {int(s): line_of(rng, cap) for s in busy}
        blob = craft(S, cap, {s: m[0] for s, m in made.items()}, rng)
        src = wm.FSKProcessorBatch(eng_src, rx_capacity=cap)
        _lib.check(L.fskhip_processor_restore(src._h, blob.ctypes.data, blob.nbytes, ident.ctypes.data, S))
        del blob
        n_busy, n_live = len(busy), sum(len(m[0]) for m in made.values())
        p_streams, p_offsets, p_res = np.zeros(n_busy, np.uint32), np.zeros(n_busy + 1, np.uint32), np.zeros(n_busy, RESULT_DTYPE)
        p_data = np.zeros(max(n_live, 1), np.uint8)
        s_streams, s_offsets, s_data = np.zeros(n_busy, np.uint32), np.zeros(n_busy + 1, np.uint32), np.zeros(max(n_live, 1), np.uint8)
        s_rows, s_counts = np.zeros((max(n_busy, 1), cap), np.uint8), np.zeros(max(n_busy, 1), np.uint32)
        s_out, s_res = np.zeros((max(n_busy, 1), cap), np.uint8), np.zeros(max(n_busy, 1), RESULT_DTYPE)

        def clone():
            d = wm.FSKProcessorBatch(eng_dst, rx_capacity=cap)
            _lib.check(L.fskhip_processor_remap(d._h, src._h, ident.ctypes.data, S))
            return d, wm.XModemReceiverBatch(d)

        def close(ctx):
            ctx[1].close()
            ctx[0].close()

        def run_poll(ctx):
            h = ctx[1]._h
            rc = L.fskhip_xmodem_rx_poll_host(h, None, None, None, None, 0, None, 0, C.byref(ne), C.byref(nb))
            if rc == _lib.E_OVERFLOW:
                rc = L.fskhip_xmodem_rx_poll_host(h, None, p_streams.ctypes.data, p_res.ctypes.data, p_offsets.ctypes.data, ne.value, p_data.ctypes.data, nb.value,
                                                  C.byref(ne), C.byref(nb))
            _lib.check(rc)
            return ne.value

        def run_poll_fit(ctx):
            _lib.check(L.fskhip_xmodem_rx_poll_host(ctx[1]._h, None, p_streams.ctypes.data, p_res.ctypes.data, p_offsets.ctypes.data, n_busy, p_data.ctypes.data,
                                                    max(n_live, 1), C.byref(ne), C.byref(nb)))
            return ne.value

        def run_dense(ctx):
            _lib.check(L.fskhip_processor_rx_drain_host(ctx[0]._h, dense_out.ctypes.data, cap, dense_counts.ctypes.data))
            _lib.check(L.fskhip_xmodem_scan_host(0, dense_out.ctypes.data, cap, dense_counts.ctypes.data, ones.ctypes.data, S, dense_data.ctypes.data, cap,
                                                 dense_res.ctypes.data))

        def run_sparse(ctx):
            na, nby = C.c_uint32(0), C.c_uint32(0)
            sparse = L.fskhip_processor_rx_drain_sparse_host
            rc = sparse(ctx[0]._h, None, 1, None, None, 0, None, 0, C.byref(na), C.byref(nby))
            if rc == _lib.E_OVERFLOW:
                rc = sparse(ctx[0]._h, None, 1, s_streams.ctypes.data, s_offsets.ctypes.data, na.value, s_data.ctypes.data, nby.value, C.byref(na), C.byref(nby))
            _lib.check(rc)
            n = na.value
            if n == 0:
                return 0
            lens = np.diff(s_offsets[:n + 1])
            s_counts[:n] = lens
            row = np.repeat(np.arange(n), lens)
            col = np.arange(nby.value) - np.repeat(s_offsets[:n], lens)
            s_rows[row, col] = s_data[:nby.value]
            _lib.check(L.fskhip_xmodem_scan_host(0, s_rows.ctypes.data, cap, s_counts.ctypes.data, ones.ctypes.data, n, s_out.ctypes.data, cap, s_res.ctypes.data))
            return n

        # the same state, the same payloads: checked before anything is timed
        c1, c2, c3, c4 = clone(), clone(), clone(), clone()
        n_events = run_poll(c1)
        first = (p_streams[:n_events].copy(), p_offsets[:n_events + 1].copy(), p_data[:nb.value].copy())
        assert run_poll_fit(c4) == n_events   # the one-call form returns the same lists
        assert all(np.array_equal(a, b) for a, b in zip(first, (p_streams[:n_events], p_offsets[:n_events + 1], p_data[:nb.value])))
        run_dense(c2)
        n_sparse = run_sparse(c3)
        assert n_sparse == n_busy
        at = {int(s): i for i, s in enumerate(p_streams[:n_events])}
        row_of = {int(s): i for i, s in enumerate(s_streams[:n_sparse])}
        for s in list(made)[:4000]:
            line, pay, cut = made[s]
            got = bytes(p_data[p_offsets[at[s]]:p_offsets[at[s] + 1]]) if s in at else b""
            assert got == pay, s
            assert bytes(dense_data[s, :dense_res[s]["data_len"]]) == pay, s
            i = row_of[s]   # (b): the host's row packing feeds the scan the same bytes
            assert bytes(s_rows[i, :s_counts[i]]) == line and bytes(s_out[i, :s_res[i]["data_len"]]) == pay, s
        for c in (c1, c2, c3, c4):
            close(c)

        poll_ms = median_ms(run_poll, a.reps, clone, close)
        poll_fit_ms = median_ms(run_poll_fit, a.reps, clone, close)
        dense_ms = median_ms(run_dense, a.reps, clone, close)
        sparse_ms = median_ms(run_sparse, a.reps, clone, close)
        row = dict(case=name, streams=S, rx_capacity=cap, n_busy=n_busy, n_events=n_events, live_bytes=n_live, poll_ms=round(poll_ms, 3), poll_fit_ms=round(poll_fit_ms, 3),
                   dense_scan_ms=round(dense_ms, 3), sparse_scan_ms=round(sparse_ms, 3), reps=a.reps)
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
