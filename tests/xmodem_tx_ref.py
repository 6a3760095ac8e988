"""What the resident XModem sender's tests share (no test in here): `step_ref`, the expectation of one fskhip_xmodem_tx_poll_* over
tests/drain_ref.py's Rings -- the contract in include/fskhip_next.h written after the reference's own control flow (sendData's three
waits, one demodulate() reply per poll) and pinned to the real XModemTransport by tests/golden/golden_xmodem_tx.npz, which
tests/test_xmodem_tx_cpu.py replays through it --, the golden set's loader, and a generator of random sender states and replies.
Nothing here calls the code under test."""
import json
import os

import numpy as np

from conftest import GOLDEN_DIR, load_npz
from drain_ref import Rings
from oracle import next_oracle as no

ACK, NAK, EOT = 0x06, 0x15, 0x04
IDLE, WAIT_NAK, WAIT_ACK, WAIT_FINAL_ACK = 0, 1, 2, 3
PROGRESS, DONE, MAX_RETRIES, ABORTED = 0, 1, 2, 3
STATE_NAMES = {IDLE: "IDLE", WAIT_NAK: "SENDING_WAIT_NAK", WAIT_ACK: "SENDING_WAIT_ACK", WAIT_FINAL_ACK: "SENDING_WAIT_FINAL_ACK"}
FIELDS = ("status", "state_after", "control", "sent_len", "sequence", "fragment_index", "n_fragments", "retries")
EVENT_DTYPE = np.dtype([(k, "<i4" if k == "control" else "<u4") for k in FIELDS])
WORDS = ("state", "sequence", "fragment_index", "retries", "packets_sent", "retransmitted")


def fragments(data, max_payload):
    """createFragments: slices of max_payload; an empty file is ONE empty fragment"""
    data = bytes(data)
    return [data[i:i + max_payload] for i in range(0, len(data), max_payload)] or [b""]


def packet(seq, payload):
    crc = no.crc16(bytes(payload))
    return bytes([no.SOH, seq, 255 - seq, len(payload)]) + bytes(payload) + bytes([crc >> 8, crc & 0xFF])


def wait_for_control_byte(reply):
    """the first of ACK / NAK / EOT in one reply, or None (the wait would ask for the next reply)"""
    for b in reply:
        if b in (ACK, NAK, EOT):
            return b
    return None


def step_one(w, frags, reply, abort, pending, max_retries):
    """one stream of one poll.  w: dict of the six WORDS (updated in place); frags: the file's fragments; reply: the live ring bytes.
    Returns (event dict, bytes handed to the modulator or None, whether the reply was taken out of the ring)."""
    assert w["state"] != IDLE
    status, control, tx, drained = PROGRESS, -1, None, False
    if abort:
        status, w["state"] = ABORTED, IDLE
    elif not pending:
        drained = True
        if w["state"] == WAIT_NAK:
            c = wait_for_control_byte(reply)
            control = -1 if c is None else c
            if c == NAK:
                tx = packet(w["sequence"], frags[w["fragment_index"]])
                w["state"] = WAIT_ACK
        elif w["state"] == WAIT_ACK:
            c = wait_for_control_byte(reply)
            control = -1 if c is None else c
            if c == ACK:
                w["retries"] = 0
                w["fragment_index"] += 1
                w["sequence"] = w["sequence"] % 255 + 1
                if w["fragment_index"] < len(frags):
                    tx = packet(w["sequence"], frags[w["fragment_index"]])
                else:
                    tx = bytes([EOT])
                    w["state"] = WAIT_FINAL_ACK
            elif c == NAK:
                w["retransmitted"] += 1
                w["retries"] += 1
                if w["retries"] > max_retries:
                    status, w["state"] = MAX_RETRIES, IDLE
                else:
                    w["retransmitted"] += 1
                    tx = packet(w["sequence"], frags[w["fragment_index"]])
        else:
            if ACK in bytes(reply):
                control, status, w["state"] = ACK, DONE, IDLE
        if tx is not None:
            w["packets_sent"] += 1
    ev = {"status": status, "state_after": w["state"], "control": control, "sent_len": 0 if tx is None else len(tx), "sequence": w["sequence"],
          "fragment_index": w["fragment_index"], "n_fragments": len(frags), "retries": w["retries"]}
    return ev, tx, drained


def listed(ev):
    return ev["status"] != PROGRESS or ev["sent_len"] != 0 or ev["control"] != -1


def step_ref(rings, words, files, max_payload, max_retries, mask=None, abort=None, pending=None):
    """(streams, events, Rings afterwards, words afterwards, {stream: bytes handed to its modulator}) of one poll.  words: dict of
    the six WORDS as arrays; files: one bytes per stream (None: no file, such a stream must be IDLE); pending: the processor's
    tx_pending per stream (None: none)."""
    S = rings.n_streams
    after = {k: np.array(words[k], np.int64).reshape(S) for k in WORDS}
    r_after, n_after = rings.r.copy(), rings.n.copy()
    streams, events, sent = [], [], {}
    for s in range(S):
        if after["state"][s] == IDLE or (mask is not None and not mask[s]):
            continue
        w = {k: int(after[k][s]) for k in WORDS}
        ev, tx, drained = step_one(w, fragments(files[s], max_payload), rings.stream_bytes(s), abort is not None and bool(abort[s]),
                                   pending is not None and bool(pending[s]), max_retries)
        for k in WORDS:
            after[k][s] = w[k]
        if drained:
            r_after[s], n_after[s] = (rings.r[s] + rings.n[s]) % rings.cap, 0
        if tx is not None:
            sent[s] = tx
        if listed(ev):
            streams.append(s)
            events.append(tuple(ev[k] for k in FIELDS))
    return (np.array(streams, np.uint32), np.array(events, EVENT_DTYPE), Rings(r_after, n_after, rings.ring),
            {k: v.astype(np.uint32) for k, v in after.items()}, sent)


def fresh_words(n_streams):
    """the words of a newly created sender"""
    w = {k: np.zeros(n_streams, np.uint32) for k in WORDS}
    w["sequence"][:] = 1
    return w


def sent_words(words, mask=None):
    """the words after send(): initializeSend for the selected streams"""
    w = {k: v.copy() for k, v in words.items()}
    sel = np.ones(len(w["state"]), bool) if mask is None else np.asarray(mask, bool)
    w["state"][sel], w["sequence"][sel], w["fragment_index"][sel], w["retries"][sel] = WAIT_NAK, 1, 0, 0
    return w


# ---- the recorded reference ------------------------------------------------------------------------------------------------------
class GoldenTx:
    """tests/golden/golden_xmodem_tx.npz + manifest_xmodem_tx.json (tools/xmodem_tx_golden/): per scenario the file, the settings,
    the demodulate() replies (bytes, or None for a wait that timed out), every modulate() call as (replies handed out before it,
    bytes), the outcome (None: resolved; else the error's text) and getStatistics()"""

    def __init__(self):
        with open(os.path.join(GOLDEN_DIR, "manifest_xmodem_tx.json")) as fh:
            self.manifest = json.load(fh)
        a = load_npz("golden_xmodem_tx.npz")

        def ragged(name):
            data, off = a[name + ".data"], a[name + ".off"]
            return [bytes(data[off[i]:off[i + 1]]) for i in range(len(off) - 1)]
        files, replies, sent = ragged("file"), ragged("reply"), ragged("sent")
        timeout, sent_after = a["reply.timeout"], a["sent.after"]
        self.busy = self.manifest["busy"]
        self.cases = []
        for c in self.manifest["cases"]:
            rf, rn, sf, sn = c["reply_first"], c["reply_count"], c["sent_first"], c["sent_count"]
            self.cases.append(dict(c, data=files[c["file"]], replies=[None if timeout[i] else replies[i] for i in range(rf, rf + rn)],
                                   sent=[(int(sent_after[i]), sent[i]) for i in range(sf, sf + sn)]))


_GOLDEN = None


def golden_tx():
    global _GOLDEN
    if _GOLDEN is None:
        _GOLDEN = GoldenTx()
    return _GOLDEN


# ---- random states and replies -----------------------------------------------------------------------------------------------------
NOISE_ARR = np.array([b for b in range(256) if b not in (ACK, NAK, EOT)], np.uint8)


def random_reply(rng, budget):
    """at most `budget` bytes: empty, noise only, one control byte alone / behind noise / in front of noise, or several control bytes"""
    kind = rng.choice(["empty", "noise", "alone", "behind", "front", "many", "many", "deep"])
    ctl = lambda: int(rng.choice([ACK, ACK, NAK, NAK, EOT]))   # noqa: E731
    noise = lambda n: bytes(rng.choice(NOISE_ARR, size=int(n)))   # noqa: E731
    if kind == "empty" or budget == 0:
        return b""
    if kind == "noise":
        return noise(rng.integers(1, budget + 1))
    if kind == "alone" or budget == 1:
        return bytes([ctl()])
    if kind == "behind":
        return noise(rng.integers(1, budget)) + bytes([ctl()])
    if kind == "front":
        return bytes([ctl()]) + noise(rng.integers(1, budget))
    if kind == "deep":   # a control byte as the very last byte of a full ring
        return noise(budget - 1) + bytes([ctl()])
    n = int(rng.integers(2, budget + 1))
    out = bytearray(noise(n))
    for i in rng.choice(n, size=int(rng.integers(2, min(n, 5) + 1)), replace=False):
        out[int(i)] = ctl()
    return bytes(out)


def random_case(rng, n_streams, cap, max_payload, max_retries, idle=0.15):
    """(Rings, words, files): every state with random words inside a random file, and a random reply in every ring, from a random
    readIndex (so about half the spans wrap).  A share `idle` of the streams are IDLE (a file or none); retries sit at, below
    and above max_retries - 1, so that a NAK ends some transfers."""
    files, words = [], fresh_words(n_streams)
    r = rng.integers(0, cap, n_streams)
    ring = rng.integers(0, 256, (n_streams, cap), dtype=np.uint8)
    n = np.zeros(n_streams, np.int64)
    for s in range(n_streams):
        ln = int(rng.choice([0, 1, max_payload - 1, max_payload, max_payload + 1, 3 * max_payload, int(rng.integers(0, 5 * max_payload + 1))]))
        data = bytes(rng.integers(0, 256, max(ln, 0), dtype=np.uint8))
        nf = len(fragments(data, max_payload))
        u = rng.random()
        state = IDLE if u < idle else int(rng.choice([WAIT_NAK, WAIT_ACK, WAIT_ACK, WAIT_FINAL_ACK]))
        idx = nf if state == WAIT_FINAL_ACK else (0 if state == WAIT_NAK else int(rng.integers(0, nf)))
        if state == IDLE and rng.random() < 0.5:
            data, idx = None, 0
        files.append(data)
        words["state"][s], words["fragment_index"][s] = state, idx
        words["sequence"][s] = int(rng.choice([1, 254, 255, idx % 255 + 1, int(rng.integers(1, 256))]))
        words["retries"][s] = int(rng.choice([0, max(max_retries - 1, 0), max_retries, int(rng.integers(0, max_retries + 1))])) if state == WAIT_ACK else 0
        words["packets_sent"][s], words["retransmitted"][s] = int(rng.integers(0, 1000)), int(rng.integers(0, 1000))
        b = random_reply(rng, cap)
        n[s] = len(b)
        ring[s, (r[s] + np.arange(len(b))) % cap] = np.frombuffer(b, np.uint8)
    return Rings(r, n, ring), words, files
