"""What the resident XModem receiver's tests share (no test in here): the expectation of one fskhip_xmodem_rx_poll_* over
tests/drain_ref.py's Rings -- steps 1-7 of the contract in include/fskhip_next.h, on top of oracle.next_oracle.scan_burst, which is
pinned to the real XModemTransport -- and a traffic generator that writes every kind of grammar step into a stream and cuts it at a
random byte.  Nothing here calls the code under test."""
import numpy as np

from drain_ref import Rings
from oracle import next_oracle as no

FIELDS = ("status", "expected_after", "packets", "dropped", "consumed", "data_len", "err_seq", "err_len", "crc_rx", "crc_calc")
RESULT_DTYPE = np.dtype([(k, "<u4" if i < 6 else "<i4") for i, k in enumerate(FIELDS)])
ERRORS = (no.XM_INVALID_SEQUENCE, no.XM_INVALID_CRC, no.XM_UNEXPECTED_SEQUENCE)


def poll_one(live, expected):
    """one stream of one poll: (R' as a dict with `data`, bytes that leave the ring)"""
    live = bytes(live)
    r = no.scan_burst(live, expected)
    if r["status"] == no.XM_TRUNCATED:   # an incomplete packet waits: the result of the bytes before its SOH
        c = r["consumed"] - (1 if r["err_seq"] < 0 else 4)
        assert live[c] == no.SOH
        r = no.scan_burst(live[:c], expected)
        assert r["status"] == no.XM_NEED_MORE and r["consumed"] == c and r["err_seq"] == r["err_len"] == -1
        removed = c
    elif r["status"] in ERRORS:          # an error clears the ring
        removed = len(live)
    else:                                # NEED_MORE or EOT: what the grammar consumed; bytes behind an EOT stay
        removed = r["consumed"]
    r["data_len"] = len(r["data"])
    return r, removed


def listed(r):
    return r["status"] != no.XM_NEED_MORE or r["packets"] + r["dropped"] > 0


def record(r):
    return tuple(r[k] for k in FIELDS)


def poll_ref(rings, expected, mask=None, packets=None, dropped=None):
    """(streams, results, offsets, data, Rings afterwards, state afterwards) of one poll.  expected / packets / dropped: the
    receiver's state per stream (the counters default to 0); the state afterwards is a dict of the three as uint32 arrays."""
    S = rings.n_streams
    exp = np.array(expected, np.int64).reshape(S)
    pk = np.zeros(S, np.int64) if packets is None else np.array(packets, np.int64)
    dr = np.zeros(S, np.int64) if dropped is None else np.array(dropped, np.int64)
    r_after, n_after = rings.r.copy(), rings.n.copy()
    streams, results, offsets, data = [], [], [0], bytearray()
    for s in range(S):
        if rings.n[s] == 0 or (mask is not None and not mask[s]):
            continue
        r, removed = poll_one(rings.stream_bytes(s), int(exp[s]))
        r_after[s] = (rings.r[s] + removed) % rings.cap
        n_after[s] = rings.n[s] - removed
        exp[s] = r["expected_after"]
        pk[s] += r["packets"]
        dr[s] += r["dropped"]
        if listed(r):
            streams.append(s)
            results.append(record(r))
            data += r["data"]
            offsets.append(len(data))
    state = {"expected": exp.astype(np.uint32), "packets": pk.astype(np.uint32), "dropped": dr.astype(np.uint32)}
    return (np.array(streams, np.uint32), np.array(results, RESULT_DTYPE), np.array(offsets, np.uint32), np.frombuffer(bytes(data), np.uint8),
            Rings(r_after, n_after, rings.ring), state)


# ---- traffic -------------------------------------------------------------------------------------------------------------------
NOISE = bytes(b for b in range(256) if b not in (no.SOH, no.EOT))
NOISE_ARR = np.frombuffer(NOISE, np.uint8)


def packet(seq, payload, nseq=None, bad_crc=False):
    crc = no.crc16(bytes(payload)) ^ (0x0100 if bad_crc else 0)
    return bytes([no.SOH, seq, (255 - seq) if nseq is None else nseq, len(payload)]) + bytes(payload) + bytes([crc >> 8, crc & 0xFF])


def traffic(rng, budget, expected, p_error=0.35, max_payload=None):
    """a byte string of at most `budget` bytes for a receiver that expects `expected`: a random concatenation of noise, valid packets
    with the running sequence, duplicates, empty and longest payloads, payloads made of SOH / EOT bytes, and -- each at most once,
    and only with probability p_error per stream -- a bad CRC, a bad seq / nseq pair, an unexpected sequence and an EOT; then cut at
    a uniformly random byte, so that every truncation point occurs.  Bytes behind an error or an EOT are kept: the poll must leave
    or clear them as the contract says."""
    top = min(255, budget - 6) if max_payload is None else min(max_payload, budget - 6)
    out = bytearray()
    e = int(expected)
    once = ["bad_crc", "bad_pair", "unexpected", "eot"] if rng.random() < p_error else []
    rng.shuffle(once)
    while True:
        kind = rng.choice(["noise", "packet", "packet", "packet", "dup", "special", "once"])
        if kind == "noise":
            item = bytes(rng.choice(NOISE_ARR, size=int(rng.integers(1, 6))))
        elif kind == "once":
            if not once:
                continue
            which = once.pop()
            ln = int(rng.integers(0, min(top, 12) + 1)) if top >= 0 else 0
            body = bytes(rng.integers(0, 256, ln, dtype=np.uint8))
            if which == "bad_crc":
                item = packet(e, body, bad_crc=True)
            elif which == "bad_pair":
                item = packet(e, body, nseq=(255 - e) ^ 0x10)
            elif which == "unexpected":
                item = packet((e + int(rng.integers(1, 200))) % 255 + 1, body)   # neither e nor the one before it
            else:
                item = bytes([no.EOT])
        else:
            if top < 0:
                item = bytes([NOISE[int(rng.integers(0, len(NOISE)))]])
            else:
                if kind == "special":
                    ln = [0, top, min(top, 3)][int(rng.integers(0, 3))]
                    body = bytes([no.SOH, no.EOT, no.SOH][:ln]) if ln <= 3 else bytes(rng.integers(0, 256, ln, dtype=np.uint8))
                else:
                    ln = int(rng.integers(0, min(top, 24) + 1))
                    body = bytes(rng.integers(0, 256, ln, dtype=np.uint8))
                if kind == "dup":
                    item = packet(255 if e == 1 else e - 1, body)
                else:
                    item = packet(e, body)
                    e = e % 255 + 1
        if len(out) + len(item) > budget:
            break
        out += item
    return bytes(out[:int(rng.integers(0, len(out) + 1))])


def start_sequences(rng, n_streams):
    """mostly 1; a fifth start at 254, so that 255 -> 1 occurs; a fifth anywhere"""
    u = rng.random(n_streams)
    return np.where(u < 0.6, 1, np.where(u < 0.8, 254, rng.integers(1, 256, n_streams))).astype(np.uint32)


def traffic_rings(rng, n_streams, cap, expected, idle=0.3, full=0.15, p_error=0.35):
    """Rings whose live spans hold traffic(): a share `idle` of the streams are empty, a share `full` hold exactly cap bytes (noise in
    front of the traffic), from a random readIndex (so about half the spans wrap).  Returns (Rings, the byte string per stream)."""
    r = rng.integers(0, cap, n_streams)
    ring = rng.integers(1, 256, (n_streams, cap), dtype=np.uint8)
    n = np.zeros(n_streams, np.int64)
    strings = []
    max_payload = 10 if cap == 16 else None
    for s in range(n_streams):
        u = rng.random()
        if u < idle:
            b = b""
        else:
            b = traffic(rng, cap, int(expected[s]), p_error, max_payload)
            if u > 1.0 - full:
                b = bytes(rng.choice(NOISE_ARR, size=cap - len(b))) + b
        strings.append(b)
        n[s] = len(b)
        ring[s, (r[s] + np.arange(len(b))) % cap] = np.frombuffer(b, np.uint8)
    return Rings(r, n, ring), strings
