"""The resident XModem sender's poll (fskhip_xmodem_tx_poll_host) against the host loop it replaces, at the size the processor row
is quoted at: 262 144 streams, rx_capacity 1024 (fp32 engines, Bell-202).  Every stream is a sender that has transmitted fragment 0
of a 256-byte file (maxPayloadSize 128) and waits for its ACK; in 0.1 %, 1 %, 10 % and 100 % of the streams the ACK has arrived,
behind one to three noise bytes.  One source processor is brought to each state by restoring an image crafted from the documented
layout (tools/xmodem_rx_bench.py's craft); every timed call works on a clone of it (fskhip_processor_remap with the identity into a
freshly created processor), both variants in one run on the same state:
  poll      a sender over the clone (send + state_set, not timed), then its one fskhip_xmodem_tx_poll_host into lists that fit
  host      what a host does per poll without it: fskhip_processor_rx_drain_sparse_host (size query + drain), a numpy scan of the
            drained spans for each stream's first ACK / NAK / EOT, the next fragment of the streams that got an ACK cut and
            serialised with fskhip_xmodem_serialize_host, and fskhip_processor_modulate_host with their mask
The two variants' pending modulations (tx_state) are compared before anything is timed.  Timing: wall clock around the synchronous
calls, host buffers allocated beforehand, median of --reps after two warm-ups, one process.

usage: python tools/xmodem_tx_bench.py [--streams 262144] [--rx-capacity 1024] [--reps 7] [--out profiles/xmodem_tx_bench.jsonl]"""
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

ACK, NAK, EOT = 0x06, 0x15, 0x04
MAX_PAYLOAD, FILE_LEN = 128, 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=262144)
    ap.add_argument("--rx-capacity", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import webaudio_modem_amd as wm
    from webaudio_modem_amd import _lib
    from webaudio_modem_amd.xmodem import TX_EVENT_DTYPE
    L = _lib.lib()
    S, cap = a.streams, a.rx_capacity
    rng = np.random.default_rng(21)
    ident = np.arange(S, dtype=np.int64)
    eng_src = wm.FSKEngine(S, CFG, precision=wm.PRECISION_F32)
    eng_dst = wm.FSKEngine(S, CFG, precision=wm.PRECISION_F32)
    files = rng.integers(0, 256, (S, FILE_LEN), dtype=np.uint8)
    offsets = (np.arange(S + 1, dtype=np.uint64) * FILE_LEN)
    words = {"state": np.full(S, 2, np.uint32), "sequence": np.ones(S, np.uint32), "fragment_index": np.zeros(S, np.uint32), "retries": np.zeros(S, np.uint32),
             "packets_sent": np.ones(S, np.uint32), "retransmitted": np.zeros(S, np.uint32)}
    rows = []
    ne = C.c_uint32(0)

    for name, frac in (("0.1%", 0.001), ("1%", 0.01), ("10%", 0.1), ("100%", 1.0)):
        busy = np.flatnonzero(rng.random(S) < frac) if frac < 1.0 else np.arange(S)
        lines = {int(s): bytes(rng.integers(0x20, 0x80, int(rng.integers(1, 4)), dtype=np.uint8)) + bytes([ACK]) for s in busy}
        blob = craft(S, cap, lines, rng)
        src = wm.FSKProcessorBatch(eng_src, rx_capacity=cap)
        _lib.check(L.fskhip_processor_restore(src._h, blob.ctypes.data, blob.nbytes, ident.ctypes.data, S))
        del blob
        n_busy, n_live = len(busy), sum(len(b) for b in lines.values())
        p_streams, p_events = np.zeros(max(n_busy, 1), np.uint32), np.zeros(max(n_busy, 1), TX_EVENT_DTYPE)
        s_streams, s_offsets, s_data = np.zeros(max(n_busy, 1), np.uint32), np.zeros(n_busy + 1, np.uint32), np.zeros(max(n_live, 1), np.uint8)
        frag, lens, seqs = np.zeros((S, MAX_PAYLOAD), np.uint8), np.zeros(S, np.uint32), np.full(S, 2, np.uint32)
        wire, wire_lens, mask = np.zeros((S, MAX_PAYLOAD + 6), np.uint8), np.zeros(S, np.uint32), np.zeros(S, np.uint8)

        def clone(with_sender):
            d = wm.FSKProcessorBatch(eng_dst, rx_capacity=cap)
            _lib.check(L.fskhip_processor_remap(d._h, src._h, ident.ctypes.data, S))
            tx = None
            if with_sender:
                tx = wm.XModemSenderBatch(d, MAX_PAYLOAD, 10)
                _lib.check(L.fskhip_xmodem_tx_send_host(tx._h, None, offsets.ctypes.data, files.ctypes.data))
                tx.set_state(**words)
            return d, tx

        def close(ctx):
            if ctx[1] is not None:
                ctx[1].close()
            ctx[0].close()

        def run_poll(ctx):
            _lib.check(L.fskhip_xmodem_tx_poll_host(ctx[1]._h, None, None, p_streams.ctypes.data, p_events.ctypes.data, len(p_streams), C.byref(ne)))
            return ne.value

        def run_host(ctx):
            na, nby = C.c_uint32(0), C.c_uint32(0)
            sparse = L.fskhip_processor_rx_drain_sparse_host
            rc = sparse(ctx[0]._h, None, 1, None, None, 0, None, 0, C.byref(na), C.byref(nby))
            if rc == _lib.E_OVERFLOW:
                rc = sparse(ctx[0]._h, None, 1, s_streams.ctypes.data, s_offsets.ctypes.data, na.value, s_data.ctypes.data, nby.value, C.byref(na), C.byref(nby))
            _lib.check(rc)
            n = na.value
            if n == 0:
                return 0
            data = s_data[:nby.value]
            ctl = np.flatnonzero((data == ACK) | (data == NAK) | (data == EOT))            # every control byte; the first one of each span decides
            owner = np.searchsorted(s_offsets[1:n + 1], ctl, side="right")
            first = ctl[np.concatenate([[True], owner[1:] != owner[:-1]])] if len(ctl) else ctl
            acked = s_streams[:n][np.unique(owner)][data[first] == ACK] if len(ctl) else np.zeros(0, np.uint32)
            mask[:] = 0
            mask[acked] = 1
            frag[acked] = files[acked, MAX_PAYLOAD:2 * MAX_PAYLOAD]                             # fragment 1 of each file
            lens[:] = 0
            lens[acked] = MAX_PAYLOAD
            _lib.check(L.fskhip_xmodem_serialize_host(0, frag.ctypes.data, MAX_PAYLOAD, lens.ctypes.data, seqs.ctypes.data, S, wire.ctypes.data, MAX_PAYLOAD + 6,
                                                      wire_lens.ctypes.data))
            _lib.check(L.fskhip_processor_modulate_host(ctx[0]._h, wire.ctypes.data, wire_lens.ctypes.data, MAX_PAYLOAD + 6, mask.ctypes.data))
            return len(acked)

        # the same state, the same modulations: checked before anything is timed
        c1, c2 = clone(True), clone(False)
        n_events = run_poll(c1)
        assert n_events == n_busy and np.array_equal(p_streams[:n_events], busy) and (p_events[:n_events]["sent_len"] == MAX_PAYLOAD + 6).all()
        assert run_host(c2) == n_busy
        t1, t2 = c1[0].tx_state(), c2[0].tx_state()
        assert np.array_equal(t1["pendingModulation"], t2["pendingModulation"]) and np.array_equal(t1["totalSamples"], t2["totalSamples"])
        assert t1["pendingModulation"].sum() == n_busy and not c1[0].rx_lengths().any()
        close(c1)
        close(c2)

        poll_ms = median_ms(run_poll, a.reps, lambda: clone(True), close)
        host_ms = median_ms(run_host, a.reps, lambda: clone(False), close)
        row = dict(case=name, streams=S, rx_capacity=cap, n_acked=n_busy, live_bytes=n_live, poll_ms=round(poll_ms, 3), host_loop_ms=round(host_ms, 3), reps=a.reps)
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
