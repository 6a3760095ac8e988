"""The resident XModem wait timers on the GPU (include/fskhip_next.h: fskhip_xmodem_timer_*, fskhip_xmodem_*_poll_timed_*;
XModemTimers).  70 streams -- one full wave and a partial one --, Bell 202 at 1 200 baud, rx_capacity 1 024, quanta of 128 samples.

Against a twin: two identical processor / handle pairs take the same quanta; one is polled through XModemTimers.poll, the other
through the plain poll with the timeout / abort masks of a numpy model of the contract (`Model` below, written from the text of
include/fskhip_next.h, not taken from the library).  After every quantum the lists, the event records, every handle word, the
timers' words, the ring lengths and the transmit state are compared bit for bit.
End to end: a sender and a file receiver looped back through process(), both under timers and with no mask from the host; a lost
packet is recovered from by the receiver's timeout NAK, or -- with a short sender timeout -- ends the sender ABORTED.
Stand-down: an overflowing timed poll changes no word of the timers."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BELL = dict(baudRate=1200, markFrequency=1200, spaceFrequency=2200)   # 40 samples per bit at 48 kHz
S, Q, CAP = 70, 128, 1024
SOH, EOT, ACK, NAK = 0x01, 0x04, 0x06, 0x15
E_OVERFLOW = -7
BURST = lambda n_bytes: (n_bytes + 3) * 400   # noqa: E731  samples of a transmission: preamble (2), SFD (1) and the bytes, 10 bits each


def crc16(data):
    crc = 0xFFFF
    for b in data:
        crc ^= b << 8
        for _ in range(8):
            crc = ((crc << 1) ^ 0x1021) & 0xFFFF if crc & 0x8000 else (crc << 1) & 0xFFFF
    return crc


def packet(seq, payload):
    c = crc16(payload)
    return bytes([SOH, seq, 255 - seq, len(payload)]) + bytes(payload) + bytes([c >> 8, c & 0xFF])


class Model:
    """the contract's fire and arm, vectorised: waited and mark per stream"""

    def __init__(self, n, timeout_samples, recv):
        self.waited, self.mark = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        self.timeout, self.recv = timeout_samples, recv

    def fire(self, elapsed, mask, state, pending, held):
        self.sel = (state != 0) & mask
        pend = self.sel & pending
        self.wait = self.sel & ~pending
        begins = self.wait & (((self.mark & 4) != 0) | (np.isin(state, (1, 3)) if self.recv else False))
        runs = self.wait & ~begins
        self.mark[pend] |= 4
        self.waited[begins], self.mark[begins] = 0, 0
        self.waited[runs] = np.minimum(self.waited[runs].astype(np.uint64) + elapsed, 0xFFFFFFFF).astype(np.uint32)
        self.held = held.copy()
        return self.wait & (self.waited >= self.timeout)

    def arm(self, streams, events, state_after, live):
        listed = np.zeros(len(state_after), bool)
        listed[streams] = True
        if self.recv:
            stage = np.where(live == 0, 0, np.where(live < 4, 1, 2)).astype(np.uint32)
            rearm = listed | (live < self.held) | (stage > (self.mark & 3))
        else:
            stage = np.zeros(len(state_after), np.uint32)
            ev = np.zeros(len(state_after), events.dtype)
            ev[streams] = events
            rearm = listed & ((ev["sent_len"] != 0) | (ev["status"] != 0) | ((ev["state_after"] == 2) & (ev["control"] == EOT)))
        idle = self.sel & (state_after == 0)
        w = self.wait & ~idle
        self.waited[w & rearm] = 0
        self.mark[w] = (self.mark[w] & ~np.uint32(3)) | stage[w]
        self.waited[idle], self.mark[idle] = 0, 0


@pytest.fixture(scope="module")
def wm():
    import __graft_entry__ as ge
    ge.build()
    import webaudio_modem_amd as wm
    return wm


@pytest.fixture(scope="module")
def bursts(wm):
    """the audio of the byte strings the scripts use, modulated once"""
    p1 = packet(1, b"ab")   # short: once its header is in, the rest arrives well inside one timeout
    rows = {"noise": b"\x33\x77", "xy": b"xy", "ack": bytes([ACK]), "nak": bytes([NAK]), "eot": bytes([EOT]), "p1": p1, "p1a": p1[:3], "p1b": p1[3:]}
    eng = wm.FSKEngine(len(rows), BELL, precision=wm.PRECISION_F32)
    sigs = eng.modulate_data(list(rows.values()))
    eng.close()
    return {k: np.asarray(s, np.float32) for k, s in zip(rows, sigs)}


class Pair:
    def __init__(self, wm, make):
        self.eng = wm.FSKEngine(S, BELL, precision=wm.PRECISION_F32)
        self.proc = wm.FSKProcessorBatch(self.eng, rx_capacity=CAP)
        self.h = make(self.proc)

    def words(self):
        tx = self.proc.tx_state()
        return ({k: v.tolist() for k, v in self.h.state().items()}, self.proc.rx_lengths().tolist(),
                {k: tx[k].tolist() for k in ("samplePosition", "totalSamples", "pendingModulation", "completed")})

    def close(self):
        for x in (self.h, self.proc, self.eng):
            x.close()


def run_twins(wm, make, recv, timeout_samples, n_quanta, script, mask, aborts):
    """script(q, streams, events, schedule): called after every quantum with the timed pair's listed events; schedule(s, q_at, name)
    plants a burst into the input of both pairs.  Returns what the timed pair listed -- {stream: [event, ...]} and the quanta of
    those events --, the handle's words and the timers' at the end."""
    A, B = Pair(wm, make), Pair(wm, make)
    timers = wm.XModemTimers(A.h, timeout_samples)
    model = Model(S, timeout_samples, recv)
    line = np.zeros((S, (n_quanta + 2) * Q), np.float32)
    seen, when = {s: [] for s in range(S)}, {s: [] for s in range(S)}

    def schedule(s, q_at, burst):
        n = min(len(burst), line.shape[1] - q_at * Q)
        if n > 0:
            line[s, q_at * Q:q_at * Q + n] = burst[:n]
    try:
        for q in range(n_quanta):
            x = line[:, q * Q:(q + 1) * Q]
            A.proc.process(x, Q)   # (the output is what moves the pending modulations on)
            B.proc.process(x, Q)
            abort = aborts.get(q)
            sa, ea = timers.poll(Q, mask=mask, abort=abort)
            flag = model.fire(Q, mask, B.h.state()["state"], B.proc.tx_state()["pendingModulation"], B.proc.rx_lengths())
            if recv:
                sb, eb = B.h.poll(mask, timeout=flag, abort=abort)
            else:
                sb, eb = B.h.poll(mask, abort=flag if abort is None else flag | abort)
            model.arm(sb, eb, B.h.state()["state"], B.proc.rx_lengths())
            assert sa.tolist() == sb.tolist() and ea.tolist() == eb.tolist(), q
            assert A.words() == B.words(), q
            t = timers.state()
            assert t["waited"].tolist() == model.waited.tolist() and t["mark"].tolist() == model.mark.tolist(), q
            for s, e in zip(sa, ea):
                seen[int(s)].append(e.copy())
                when[int(s)].append(q)
            script(q, sa, ea, schedule)
        return seen, when, A.h.state(), timers.state()
    finally:
        timers.close()
        A.close()
        B.close()


def test_file_receiver_against_a_twin(wm, bursts):
    """by stream % 7: 0 hears nothing (timeout NAKs up to MAX_RETRIES); 1 hears noise bytes; 2 a packet in two halves closer than the
    timeout; 3 the halves further apart than it; 4 is masked out; 5 is aborted by the caller; 6 a whole packet, then EOT"""
    timeout, max_retries = 4096, 2
    kind = np.arange(S) % 7
    mask = kind != 4
    aborts = {30: kind == 5}
    t0 = 20   # the initial NAK (1 600 samples) has gone out by then
    gap = lambda samples: -(-samples // Q)   # noqa: E731

    def script(q, streams, events, schedule):
        if q != 0:
            return
        for s in range(S):
            if kind[s] == 1:
                schedule(s, t0 - 4, bursts["noise"])
            elif kind[s] in (2, 3):
                schedule(s, t0, bursts["p1a"])
                schedule(s, t0 + gap(len(bursts["p1a"]) + (256 if kind[s] == 2 else 6144)), bursts["p1b"])
            elif kind[s] == 6:
                schedule(s, t0, bursts["p1"])
                schedule(s, t0 + gap(len(bursts["p1"])) + 14, bursts["eot"])

    def make(proc):
        rx = wm.XModemFileReceiverBatch(proc, 64, max_retries)
        rx.start()
        return rx
    seen, when, state, tstate = run_twins(wm, make, True, timeout, 170, script, mask, aborts)
    for s in range(S):
        ev = seen[s]
        naks = [e for e in ev if e["control"] == NAK]
        if kind[s] == 0:     # timeout -> NAK, NAK, then MAX_RETRIES
            assert [int(e["status"]) for e in ev] == [0, 0, 2] and len(naks) == 2 and state["state"][s] == 0, s
        elif kind[s] == 1:   # the noise re-armed the timer: its first timeout comes later than a silent stream's
            assert ev[0]["control"] == NAK and when[s][0] > when[0][0], s
        elif kind[s] == 2:   # the gap was shorter than the timeout: accepted, no NAK before the ACK
            assert ev[0]["control"] == ACK and ev[0]["accepted_len"] == 2, s
        elif kind[s] == 3:   # the first half timed out: NAK, ring cleared; the second half is no packet
            assert ev[0]["control"] == NAK and state["file_len"][s] == 0 and state["packets_received"][s] == 0, s
        elif kind[s] == 4:   # masked out: no word moved since start()
            assert not ev and state["state"][s] == 1 and tstate["waited"][s] == 0 and tstate["mark"][s] == 0, s
        elif kind[s] == 5:
            assert [int(e["status"]) for e in ev] == [3] and state["state"][s] == 0, s
        else:
            assert [int(e["control"]) for e in ev[:2]] == [ACK, ACK] and ev[1]["status"] == 1 and state["file_len"][s] == 2, s


def test_sender_against_a_twin(wm, bursts):
    """by stream % 7: 0 hears nothing (the timer aborts it); 1 hears bytes that are no control bytes (no re-arm: aborted at the same
    poll as 0); 2 a NAK, then an EOT while it waits for the ACK (re-armed), then nothing; 3 an ACK in WAIT_NAK (skipped, the timer
    runs on), then nothing; 4 is masked out; 5 is aborted by the caller; 6 runs a whole transfer of two fragments"""
    timeout = 3072
    kind = np.arange(S) % 7
    mask = kind != 4
    aborts = {6: kind == 5}
    after = lambda sent_len: -(-BURST(sent_len) // Q) + 3   # noqa: E731  quanta until a transmission has gone out

    def script(q, streams, events, schedule):
        if q == 0:
            for s in range(S):
                if kind[s] == 1:
                    schedule(s, 2, bursts["xy"])
                elif kind[s] in (2, 6):
                    schedule(s, 2, bursts["nak"])
                elif kind[s] == 3:
                    schedule(s, 2, bursts["ack"])
        for s, e in zip(streams, events):
            sent_len = int(e["sent_len"])
            if sent_len == 0:
                continue
            if kind[s] == 2:
                schedule(int(s), q + after(sent_len) + 6, bursts["eot"])
            elif kind[s] == 6:
                schedule(int(s), q + after(sent_len), bursts["ack"])

    def make(proc):
        tx = wm.XModemSenderBatch(proc, max_payload_size=4, max_retries=2)
        tx.send([b"sixsix"] * S)
        return tx
    seen, when, state, tstate = run_twins(wm, make, False, timeout, 170, script, mask, aborts)
    for s in range(S):
        ev = seen[s]
        if kind[s] in (0, 1):
            assert [int(e["status"]) for e in ev] == [3] and state["packets_sent"][s] == 0, s
        elif kind[s] == 2:   # packet, the EOT returned, then the abort -- later than a timer armed at the packet's end would give
            assert [(int(e["status"]), int(e["control"])) for e in ev] == [(0, NAK), (0, EOT), (3, -1)], s
        elif kind[s] == 3:
            assert [(int(e["status"]), int(e["control"])) for e in ev] == [(0, ACK), (3, -1)], s
        elif kind[s] == 4:
            assert not ev and state["state"][s] == 1 and tstate["waited"][s] == 0 and tstate["mark"][s] == 0, s
        elif kind[s] == 5:
            assert [int(e["status"]) for e in ev] == [3], s
        else:
            assert [int(e["status"]) for e in ev] == [0, 0, 0, 1] and state["packets_sent"][s] == 3 and state["retransmitted"][s] == 0, s
        assert state["state"][s] == (1 if kind[s] == 4 else 0), s
    assert {when[s][-1] for s in range(S) if kind[s] in (0, 1)} == {timeout // Q - 1}   # the first poll at the deadline
    assert all(when[s][-1] > when[s][1] + timeout // Q - 2 for s in range(S) if kind[s] == 2)


@pytest.mark.parametrize("tx_timeout", [8192, 3072])
def test_end_to_end_a_lost_packet(wm, tx_timeout):
    """files of 40 bytes in fragments of 16 through process(), sender and receiver under timers, no mask from the host.  On every
    third stream the quanta that carry the second packet are silence, once.  The receiver's timer (12 288 samples: longer than a
    packet lasts) NAKs; with a sender timeout of 8 192 the NAK is answered and every file arrives, with 3 072 the sender's own
    timer ends the silenced transfers first: ABORTED."""
    rx_timeout, max_payload = 12288, 16
    rng = np.random.default_rng(0x71E)
    files = [bytes(rng.integers(0, 256, 40, dtype=np.uint8)) for _ in range(S)]
    lost = np.arange(S) % 3 == 1
    engs = [wm.FSKEngine(S, BELL, precision=wm.PRECISION_F32) for _ in range(2)]
    A, B = (wm.FSKProcessorBatch(e, rx_capacity=CAP) for e in engs)
    tx, rx = wm.XModemSenderBatch(A, max_payload), wm.XModemFileReceiverBatch(B, 64)
    tt, rt = wm.XModemTimers(tx, tx_timeout), wm.XModemTimers.from_ms(rx, 256, 48000)
    assert rt.timeout_samples == rx_timeout
    tx.send(files)
    rx.start()
    a_out = b_out = np.zeros((S, Q), np.float32)
    silent_until = np.zeros(S, int)
    tx_end, rx_end, rx_naks = {}, {}, np.zeros(S, int)
    try:
        for q in range(1400):
            a_in, b_in = b_out, a_out.copy()
            b_in[silent_until > q] = 0
            a_out, b_out = A.process(a_in, Q), B.process(b_in, Q)
            ts, te = tt.poll(Q)
            for s, e in zip(ts, te):
                if e["sent_len"] and e["fragment_index"] == 1 and lost[s] and not silent_until[s]:
                    silent_until[s] = q + 1 + -(-BURST(int(e["sent_len"])) // Q) + 4
                if e["status"]:
                    tx_end[int(s)] = int(e["status"])
            rs, re_ = rt.poll(Q)
            for s, e in zip(rs, re_):
                rx_naks[s] += e["control"] == NAK
                if e["status"]:
                    rx_end[int(s)] = int(e["status"])
            if len(tx_end) == S and (tx_timeout == 3072 or len(rx_end) == S):
                break
        ts_, rs_ = tx.state(), rx.state()
        got = rx.files()
    finally:
        for x in (tt, rt, tx, rx, A, B, *engs):
            x.close()
    assert lost.sum() > 20 and (silent_until[lost] > 0).all() and not silent_until[~lost].any()
    if tx_timeout == 8192:
        assert tx_end == {s: 1 for s in range(S)} and rx_end == {s: 1 for s in range(S)}, (tx_end, rx_end, q)
        assert got == files
        assert rx_naks.tolist() == lost.astype(int).tolist()                       # exactly one timeout NAK where the packet was lost
        assert ts_["retransmitted"].tolist() == (2 * lost).tolist()                # an answered NAK counts twice (xmodem.ts:146, 155)
        assert ts_["packets_sent"].tolist() == (4 + lost).tolist() and rs_["packets_received"].tolist() == [3] * S
        assert not rs_["dropped"].any() and not rs_["retries"].any()
    else:
        assert tx_end == {s: 3 if lost[s] else 1 for s in range(S)}, (tx_end, q)
        assert all(got[s] == files[s] for s in np.flatnonzero(~lost)) and all(got[s] == files[s][:16] for s in np.flatnonzero(lost))
        assert not ts_["retransmitted"].any()


def test_a_timed_poll_that_stands_down_changes_nothing(wm):
    eng = wm.FSKEngine(S, BELL, precision=wm.PRECISION_F32)
    proc = wm.FSKProcessorBatch(eng, rx_capacity=CAP)
    tx = wm.XModemSenderBatch(proc, 16, 2)
    tx.send([b"file"] * S)
    t = wm.XModemTimers(tx, 1000)
    try:
        assert len(t.poll(600)[0]) == 0
        waited = np.full(S, 600, np.uint32)
        assert t.state()["waited"].tolist() == waited.tolist() and not t.state()["mark"].any()
        before = {k: v.tolist() for k, v in tx.state().items()}
        L, ne = t._L, C.c_uint32(0)
        streams, events = np.zeros(S, np.uint32), np.zeros(S, wm.xmodem.TX_EVENT_DTYPE)
        # 1 200 >= 1 000: every stream would be aborted and listed; the lists hold 69
        assert L.fskhip_xmodem_tx_poll_timed_host(t._h, 600, None, None, streams.ctypes.data, events.ctypes.data, S - 1, C.byref(ne)) == E_OVERFLOW
        assert ne.value == S and "nothing was polled" in L.fskhip_last_error().decode()
        assert t.state()["waited"].tolist() == waited.tolist() and not t.state()["mark"].any()
        assert {k: v.tolist() for k, v in tx.state().items()} == before
        assert L.fskhip_xmodem_tx_poll_timed_host(t._h, 600, None, None, None, None, 0, C.byref(ne)) == E_OVERFLOW and ne.value == S
        assert t.state()["waited"].tolist() == waited.tolist()
        # the receiver's poll refuses a sender's timer; state_set validates; the same poll with room ends every transfer
        assert L.fskhip_xmodem_recv_poll_timed_host(t._h, 600, None, None, None, None, 0, C.byref(ne)) == -1
        assert L.fskhip_last_error().decode() == "fskhip_xmodem_recv_poll_timed_host: the timer was created over a sender"
        with pytest.raises(wm.FskHipError, match=r"mark\[3\] = 8 is not a mark"):
            t.set_state(mark=np.where(np.arange(S) == 3, 8, 0))
        sl, ev = t.poll(600)
        assert sl.tolist() == list(range(S)) and (ev["status"] == 3).all()
        assert not t.state()["waited"].any() and not tx.state()["state"].any()
        t.set_state(waited=np.arange(S), mark=np.full(S, 4))
        assert t.state()["waited"].tolist() == list(range(S)) and (t.state()["mark"] == 4).all()
        t.reset(5)
        assert t.state()["waited"][5] == 0 and t.state()["mark"][5] == 0 and t.state()["waited"][6] == 6
        # a timer whose sender is gone refuses, and says so
        tx.close()
        with pytest.raises(ValueError, match="handle has been closed"):
            t.poll(1)
        assert L.fskhip_xmodem_timer_reset(t._h, -1) == -1
        assert L.fskhip_last_error().decode() == "fskhip_xmodem_timer_reset: the timer's sender has been destroyed"
    finally:
        for x in (t, tx, proc, eng):
            x.close()
