"""What the resident XModem file receiver's tests share (no test in here): `step_ref`, the expectation of one
fskhip_xmodem_recv_poll_* over tests/drain_ref.py's Rings -- the contract in include/fskhip_next.h written after the reference's own
control flow (receiveAllPackets / receiveAndProcessPacket over a receive buffer, stopping where a control byte's modulation is
awaited) and pinned to the real XModemTransport by tests/golden/golden_xmodem_recv.npz, which tests/test_xmodem_recv_cpu.py replays
through it --, the golden set's loader, and a generator of random receiver states and ring contents.  Nothing here calls the code
under test."""
import json
import os

import numpy as np

from conftest import GOLDEN_DIR, load_npz
from drain_ref import Rings
from oracle import next_oracle as no

SOH, ACK, NAK, EOT = 0x01, 0x06, 0x15, 0x04
IDLE, SEND_NAK, WAIT_BLOCK, SEND_ACK = 0, 1, 2, 3
PROGRESS, DONE, MAX_RETRIES, ABORTED, FILE_FULL = 0, 1, 2, 3, 4
STATE_NAMES = {IDLE: "IDLE", SEND_NAK: "RECEIVING_SEND_NAK", WAIT_BLOCK: "RECEIVING_WAIT_BLOCK", SEND_ACK: "RECEIVING_SEND_ACK"}
FIELDS = ("status", "state_after", "control", "step", "seq", "len", "accepted_len", "file_len", "expected", "retries", "crc_rx", "crc_calc")
EVENT_DTYPE = np.dtype([(k, "<i4" if k in ("control", "seq", "len", "crc_rx", "crc_calc") else "<u4") for k in FIELDS])
WORDS = ("state", "expected", "retries", "file_len", "packets_received", "dropped", "packets_sent")
ERRORS = (no.XM_INVALID_SEQUENCE, no.XM_INVALID_CRC, no.XM_UNEXPECTED_SEQUENCE)


def packet(seq, payload, crc_xor=0, inv=None):
    crc = no.crc16(bytes(payload)) ^ crc_xor
    return bytes([SOH, seq, 255 - seq if inv is None else inv, len(payload)]) + bytes(payload) + bytes([crc >> 8, crc & 0xFF])


def first_step(buf, expected):
    """the receive loop over the receive buffer `buf` up to the first step that owes a reply.  Returns a dict: kind ('accepted',
    'duplicate', 'error', 'eot' or None), step (XM_*), removed (bytes the loop took out of the buffer), seq, len, payload, crc_rx,
    crc_calc, packets, dropped (the statistics' increments)."""
    out = dict(kind=None, step=no.XM_NEED_MORE, removed=0, seq=-1, len=-1, payload=b"", crc_rx=-1, crc_calc=-1, packets=0, dropped=0)
    pos, n = 0, len(buf)
    while pos < n:
        b = buf[pos]
        if b == EOT:
            return dict(out, kind="eot", step=no.XM_EOT, removed=pos + 1)
        if b != SOH:
            pos += 1   # ignored
            continue
        if pos + 4 > n:   # waitForBytes(3) still waits
            break
        seq, nseq, ln = buf[pos + 1], buf[pos + 2], buf[pos + 3]
        prev = 255 if expected == 1 else expected - 1
        if seq + nseq != 255:
            return dict(out, kind="error", step=no.XM_INVALID_SEQUENCE, seq=seq, len=ln, dropped=1)
        if seq != expected and seq != prev:
            return dict(out, kind="error", step=no.XM_UNEXPECTED_SEQUENCE, seq=seq, len=ln, dropped=1)
        end = pos + 4 + ln + 2
        if end > n:   # waitForBytes(len + 2) still waits
            break
        if seq == prev:
            return dict(out, kind="duplicate", removed=end, seq=seq, len=ln, dropped=1)
        payload = bytes(buf[pos + 4:pos + 4 + ln])
        rx, calc = (buf[end - 2] << 8) | buf[end - 1], no.crc16(payload)
        if rx != calc:
            return dict(out, kind="error", step=no.XM_INVALID_CRC, seq=seq, len=ln, crc_rx=rx, crc_calc=calc, packets=1, dropped=1)
        return dict(out, kind="accepted", removed=end, seq=seq, len=ln, payload=payload, packets=1, start=pos)
    return dict(out, removed=pos)   # noise has left; an incomplete packet waits, SOH included


def step_one(w, data, buf, abort, pending, timeout, max_retries, file_capacity):
    """one stream of one poll.  w: dict of the seven WORDS (updated in place); data: the file so far; buf: the live ring bytes.
    Returns (event dict or None where no word is touched, the control byte transmitted or None, bytes removed from the ring, the
    file afterwards)."""
    assert w["state"] != IDLE
    status, control, removed = PROGRESS, None, 0
    ev = dict(step=no.XM_NEED_MORE, seq=-1, len=-1, accepted_len=0, crc_rx=-1, crc_calc=-1)
    if abort:
        status, w["state"] = ABORTED, IDLE
    elif pending:
        return None, None, 0, data
    else:
        w["state"] = WAIT_BLOCK
        f = first_step(buf, w["expected"])
        removed, failed = f["removed"], False
        ev.update(step=f["step"], seq=f["seq"], len=f["len"], crc_rx=f["crc_rx"], crc_calc=f["crc_calc"])
        if f["kind"] == "eot":
            control, status, w["state"] = ACK, DONE, IDLE
        elif f["kind"] == "error":
            w["packets_received"] += f["packets"]
            w["dropped"] += f["dropped"]
            failed = True
        elif f["kind"] == "accepted":
            if len(data) + f["len"] > file_capacity:
                status, w["state"], removed = FILE_FULL, IDLE, f["start"]
            else:
                data = data + f["payload"]
                ev["accepted_len"] = f["len"]
                w["expected"] = w["expected"] % 255 + 1
                w["retries"] = 0
                w["packets_received"] += 1
                control, w["state"] = ACK, SEND_ACK
        elif f["kind"] == "duplicate":
            w["dropped"] += 1
            control = ACK
        elif timeout:
            failed = True
        if failed:
            removed = len(buf)
            w["retries"] += 1
            if w["retries"] > max_retries:
                status, w["state"] = MAX_RETRIES, IDLE
            else:
                control = NAK
        if control is not None:
            w["packets_sent"] += 1
    w["file_len"] = len(data)
    ev.update(status=status, state_after=w["state"], control=-1 if control is None else control, file_len=len(data), expected=w["expected"],
              retries=w["retries"])
    return ev, control, removed, data


def listed(ev):
    return ev["status"] != PROGRESS or ev["control"] != -1


def step_ref(rings, words, files, file_capacity, max_retries, mask=None, timeout=None, abort=None, pending=None):
    """(streams, events, Rings afterwards, words afterwards, files afterwards, {stream: the control byte handed to its modulator, as
    bytes}) of one poll.  words: dict of the seven WORDS as arrays; files: one bytes per stream, len(files[s]) == file_len[s]; pending:
    the processor's tx_pending per stream (None: none)."""
    S = rings.n_streams
    after = {k: np.array(words[k], np.int64).reshape(S) for k in WORDS}
    r_after, n_after = rings.r.copy(), rings.n.copy()
    files_after = [bytes(f) for f in files]
    streams, events, sent = [], [], {}
    for s in range(S):
        if after["state"][s] == IDLE or (mask is not None and not mask[s]):
            continue
        assert len(files[s]) == after["file_len"][s]
        w = {k: int(after[k][s]) for k in WORDS}
        ev, control, removed, data = step_one(w, files_after[s], rings.stream_bytes(s), abort is not None and bool(abort[s]),
                                              pending is not None and bool(pending[s]), timeout is not None and bool(timeout[s]), max_retries,
                                              file_capacity)
        if ev is None:
            continue
        for k in WORDS:
            after[k][s] = w[k]
        files_after[s] = data
        r_after[s], n_after[s] = (rings.r[s] + removed) % rings.cap, rings.n[s] - removed
        if control is not None:
            sent[s] = bytes([control])
        if listed(ev):
            streams.append(s)
            events.append(tuple(ev[k] for k in FIELDS))
    return (np.array(streams, np.uint32), np.array(events, EVENT_DTYPE), Rings(r_after, n_after, rings.ring),
            {k: v.astype(np.uint32) for k, v in after.items()}, files_after, sent)


def fresh_words(n_streams):
    """the words of a newly created receiver"""
    w = {k: np.zeros(n_streams, np.uint32) for k in WORDS}
    w["expected"][:] = 1
    return w


def started_words(words, mask=None):
    """the words after start(): initializeReceive and the initial NAK for the selected streams"""
    w = {k: v.copy() for k, v in words.items()}
    sel = np.ones(len(w["state"]), bool) if mask is None else np.asarray(mask, bool)
    w["state"][sel], w["expected"][sel], w["retries"][sel], w["file_len"][sel] = SEND_NAK, 1, 0, 0
    w["packets_sent"][sel] += 1
    return w


# ---- the recorded reference ------------------------------------------------------------------------------------------------------
class GoldenRecv:
    """tests/golden/golden_xmodem_recv.npz + manifest_xmodem_recv.json (tools/xmodem_recv_golden/): per scenario the settings, the
    demodulate() replies (bytes, or None for a wait that timed out), every modulate() call as (replies handed out before it, bytes),
    the outcome (the returned bytes, or the error's text), getStatistics(), expectedSequence and the state afterwards"""

    def __init__(self):
        with open(os.path.join(GOLDEN_DIR, "manifest_xmodem_recv.json")) as fh:
            self.manifest = json.load(fh)
        a = load_npz("golden_xmodem_recv.npz")

        def ragged(name):
            data, off = a[name + ".data"], a[name + ".off"]
            return [bytes(data[off[i]:off[i + 1]]) for i in range(len(off) - 1)]
        results, replies, sent = ragged("result"), ragged("reply"), ragged("sent")
        timeout, sent_after = a["reply.timeout"], a["sent.after"]
        self.busy = self.manifest["busy"]
        self.cases = []
        for c in self.manifest["cases"]:
            rf, rn, sf, sn = c["reply_first"], c["reply_count"], c["sent_first"], c["sent_count"]
            self.cases.append(dict(c, result=None if c["result"] < 0 else results[c["result"]],
                                   replies=[None if timeout[i] else replies[i] for i in range(rf, rf + rn)],
                                   sent=[(int(sent_after[i]), sent[i]) for i in range(sf, sf + sn)]))

    def case(self, name):
        return [c for c in self.cases if c["name"] == name][0]


_GOLDEN = None


def golden_recv():
    global _GOLDEN
    if _GOLDEN is None:
        _GOLDEN = GoldenRecv()
    return _GOLDEN


def replay(case, poll, cap, r0, file_capacity=4096):
    """one golden scenario through `poll(rings, timeout, abort) -> (events by stream {0: ev} or {}, Rings afterwards, control bytes
    sent by this poll as a list)`, on one stream whose ring has `cap` bytes and starts at readIndex r0.  Each reply is planted behind
    what the ring holds, then polls run until nothing is listed (pending modulations are the caller's to clear between polls); a
    reply of None is a poll with the timeout flag; an abort after the last reply is a poll with the abort flag.  Returns (the
    modulate() calls as (replies handed out before, bytes), the last status)."""
    rings = Rings([r0], [0], np.zeros((1, cap), np.uint8))
    sent, status = [(0, bytes([NAK]))], PROGRESS   # start(): the initial NAK, before any reply

    def run(taken, timeout=False, abort=False):
        nonlocal rings, status
        first = True
        while True:
            evs, rings, tx = poll(rings, timeout and first, abort and first)
            first = False
            sent.extend((taken, b) for b in tx)
            if 0 in evs:
                status = int(evs[0]["status"])
            if 0 not in evs or status != PROGRESS:
                return
    for i, reply in enumerate(case["replies"]):
        if status != PROGRESS:
            break
        if reply is None:
            run(i + 1, timeout=True)
            continue
        w = (rings.r[0] + rings.n[0]) % cap
        assert rings.n[0] + len(reply) <= cap
        rings.ring[0, (w + np.arange(len(reply))) % cap] = np.frombuffer(reply, np.uint8)
        rings.n[0] += len(reply)
        run(i + 1)
    if case.get("abort") and status == PROGRESS:
        run(len(case["replies"]), abort=True)
    return sent, status


# ---- random states and rings -------------------------------------------------------------------------------------------------------
NOISE_ARR = np.array([b for b in range(256) if b not in (SOH, EOT)], np.uint8)


def random_content(rng, budget, expected, max_payload):
    """at most `budget` ring bytes for a receiver that expects `expected`: noise, good packets, duplicates, the three errors, an EOT
    and a packet cut short, in random order"""
    prev = 255 if expected == 1 else expected - 1
    out = b""
    noise = lambda n: bytes(rng.choice(NOISE_ARR, size=int(n)))   # noqa: E731
    payload = lambda: bytes(rng.integers(0, 256, int(rng.integers(0, max_payload + 1)), dtype=np.uint8))   # noqa: E731
    for _ in range(int(rng.integers(0, 4))):
        kind = rng.choice(["noise", "good", "good", "good", "dup", "badinv", "badcrc", "unexpected", "eot", "cut", "cuthdr"])
        if kind == "noise":
            piece = noise(rng.integers(1, 6))
        elif kind == "good":
            piece = packet(expected, payload())
        elif kind == "dup":
            piece = packet(prev, payload())
        elif kind == "badinv":
            piece = packet(expected, payload(), inv=(255 - expected) ^ int(rng.integers(1, 256)))
        elif kind == "badcrc":
            piece = packet(expected, payload(), crc_xor=int(rng.integers(1, 65536)))
        elif kind == "unexpected":
            piece = packet((expected + int(rng.integers(1, 254))) % 255 + 1, payload())
            if piece[1] in (expected, prev):
                piece = packet(expected % 255 + 1, payload())
        elif kind == "eot":
            piece = bytes([EOT])
        elif kind == "cut":
            p = packet(int(rng.choice([expected, prev])), payload())
            piece = p[:int(rng.integers(4, len(p)))]
        else:
            piece = packet(expected, payload())[:int(rng.integers(1, 4))]
        if len(out) + len(piece) > budget:
            break
        out += piece
        if kind in ("cut", "cuthdr"):
            break
    return out


def random_case(rng, n_streams, cap, max_payload, max_retries, file_capacity, idle=0.15):
    """(Rings, words, files): every state with random words and a random file so far, and random content in every ring, from a
    random readIndex (so about half the spans wrap).  A share `idle` of the streams are IDLE; retries sit at, below and above
    max_retries - 1, so that an error ends some transfers; some files are within a packet of file_capacity, so that some are full."""
    words, files = fresh_words(n_streams), []
    r = rng.integers(0, cap, n_streams)
    ring = rng.integers(0, 256, (n_streams, cap), dtype=np.uint8)
    n = np.zeros(n_streams, np.int64)
    for s in range(n_streams):
        state = IDLE if rng.random() < idle else int(rng.choice([SEND_NAK, WAIT_BLOCK, WAIT_BLOCK, SEND_ACK]))
        expected = int(rng.choice([1, 2, 254, 255, int(rng.integers(1, 256))]))
        flen = int(rng.choice([0, min(1, file_capacity), file_capacity, max(file_capacity - 1, 0), max(file_capacity - max_payload, 0), int(rng.integers(0, file_capacity + 1))]))
        files.append(bytes(rng.integers(0, 256, flen, dtype=np.uint8)))
        words["state"][s], words["expected"][s], words["file_len"][s] = state, expected, flen
        words["retries"][s] = int(rng.choice([0, max(max_retries - 1, 0), max_retries, int(rng.integers(0, max_retries + 1))]))
        for k in ("packets_received", "dropped", "packets_sent"):
            words[k][s] = int(rng.integers(0, 1000))
        b = random_content(rng, cap, expected, max_payload)
        n[s] = len(b)
        ring[s, (r[s] + np.arange(len(b))) % cap] = np.frombuffer(b, np.uint8)
    return Rings(r, n, ring), words, files
