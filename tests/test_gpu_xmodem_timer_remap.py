"""The XModem wait timers through remap, snapshot and restore on the GPU (include/fskhip_next.h: fskhip_xmodem_timer_remap,
_snapshot, _restore; XModemTimers.remapped / snapshot / from_snapshot).  70 streams -- one full wave and a partial one --, Bell 202
at 1 200 baud, rx_capacity 1 024, quanta of 128 samples, as tests/test_gpu_xmodem_timer.py.

Words through every map: random valid words set with set_state reach the destination as the numpy take says, 0 and 0 at -1, by
remapped and by snapshot -> from_snapshot, for both kinds, and once at 3 000 streams (twelve workgroups, the last one partial).
Canonical image: the bytes depend on the words alone.
A wait interrupted mid-way: the looped-back transfer of test_gpu_xmodem_timer.py that loses a packet, stopped half way through
the receiver's wait for the lost packet, carried under a random map that grows the batch, and continued: every event of both
sides at the quantum the uninterrupted run has it.  With fresh timers in the carried ones' place the timeout NAK comes later.
Refusals leave the destination as it was."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BELL = dict(baudRate=1200, markFrequency=1200, spaceFrequency=2200)   # 40 samples per bit at 48 kHz
S, Q, CAP = 70, 128, 1024
NAK = 0x15
E_INVALID = -1
TIMEOUT = {"recv": 12288, "tx": 8192}
MARKS = {"recv": (0, 1, 2, 4, 5, 6), "tx": (0, 4)}
KIND_NUMBER = {"tx": 2, "recv": 3}
BURST = lambda n_bytes: (n_bytes + 3) * 400   # noqa: E731  samples of a transmission: preamble (2), SFD (1) and the bytes, 10 bits each


@pytest.fixture(scope="module")
def wm():
    import __graft_entry__ as ge
    ge.build()
    import webaudio_modem_amd as wm
    return wm


class Stack:
    """an engine, a processor over it and a file receiver or a sender over that: what a timer stands beside"""

    def __init__(self, wm, n, kind):
        self.eng = wm.FSKEngine(n, BELL, precision=wm.PRECISION_F32)
        self.proc = wm.FSKProcessorBatch(self.eng, rx_capacity=CAP)
        self.h = wm.XModemFileReceiverBatch(self.proc, 64) if kind == "recv" else wm.XModemSenderBatch(self.proc, 16)

    def close(self):
        for x in (self.h, self.proc, self.eng):
            x.close()


@pytest.fixture(scope="module")
def stacks(wm):
    """handles by (kind, streams), made once: several timers over one handle are independent, and no test here polls these"""
    made = {}

    def get(kind, n):
        if (kind, n) not in made:
            made[kind, n] = Stack(wm, n, kind)
        return made[kind, n].h
    yield get
    for st in made.values():
        st.close()


def random_words(rng, n, kind):
    timeout = TIMEOUT[kind]
    edge = np.array([0, 1, timeout - 1, timeout, 0xFFFFFFFF], np.uint32)
    waited = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    at = rng.choice(n, min(n, 2 * len(edge)), replace=False)
    waited[at] = np.resize(edge, len(at))
    mark = rng.choice(np.array(MARKS[kind], np.uint32), n)
    if n >= len(MARKS[kind]):
        mark[rng.choice(n, len(MARKS[kind]), replace=False)] = MARKS[kind]
    return waited, mark


def take(words, m):
    m = np.asarray(m, np.int64)
    return [np.where(m >= 0, w[np.maximum(m, 0)], 0).astype(np.uint32).tolist() for w in words]


def words_of(t):
    st = t.state()
    return [st["waited"].tolist(), st["mark"].tolist()]


def maps_for(rng, n_src):
    """the five shapes of tests/test_gpu_xmodem_remap.py, and the identity with one stream replaced"""
    if n_src == 1:
        return {"identity-1": np.array([0], np.int64)}
    shrink = np.sort(rng.choice(n_src, 50, replace=False)).astype(np.int64)
    grow = np.concatenate([np.arange(n_src), -np.ones(14)]).astype(np.int64)
    rng.shuffle(grow)
    perm = rng.integers(0, n_src, n_src).astype(np.int64)          # with replacement: clones and drops
    assert len(set(perm)) < n_src
    but_one = np.arange(n_src, dtype=np.int64)
    but_one[int(rng.integers(0, n_src))] = -1
    return {"shrink": shrink, "grow": grow, "clones": perm, "all-new": -np.ones(n_src, np.int64), "identity-but-one": but_one}


MAP_NAMES = ("shrink", "grow", "clones", "all-new", "identity-1", "identity-but-one")


def both_ways(wm, stacks, kind, src, words, m):
    """the destination's words by remapped and by snapshot -> from_snapshot against the take; the two images"""
    dst_h = stacks(kind, len(m))
    want = take(words, m)
    images = []
    for how in ("remap", "restore"):
        if how == "remap":
            nxt = src.remapped(dst_h, m)
        else:
            nxt = wm.XModemTimers.from_snapshot(dst_h, src.snapshot(), stream_map=m)
        try:
            assert nxt.n_streams == len(m) and nxt.timeout_samples == src.timeout_samples
            assert words_of(nxt) == want, how
            images.append(nxt.snapshot())
        finally:
            nxt.close()
    assert images[0] == images[1]
    assert words_of(src) == [w.tolist() for w in words]   # the source is read only
    return images[0]


@pytest.mark.parametrize("name", MAP_NAMES)
@pytest.mark.parametrize("kind", ["recv", "tx"])
def test_words_through_every_map(wm, stacks, kind, name):
    rng = np.random.default_rng(0x71A0 + 16 * MAP_NAMES.index(name) + (kind == "tx"))
    n_src = 1 if name == "identity-1" else S
    words = random_words(rng, n_src, kind)
    m = maps_for(rng, n_src)[name]
    src = wm.XModemTimers(stacks(kind, n_src), TIMEOUT[kind])
    try:
        src.set_state(*words)
        image = both_ways(wm, stacks, kind, src, words, m)
        info = wm.xmodem_timer_snapshot_info(image)
        assert info == dict(kind=KIND_NUMBER[kind], n_streams=len(m), timeout_samples=TIMEOUT[kind], reserved=0)
        assert len(image) == (48 + 8 * len(m) + 15) // 16 * 16
        got = np.frombuffer(image, "<u4", 2 * len(m), 48).reshape(-1, 2)
        assert [got[:, 0].tolist(), got[:, 1].tolist()] == take(words, m)   # the documented layout
        if (m >= 0).all():
            assert image == src.snapshot(streams=m)
    finally:
        src.close()


def test_words_at_3000_streams(wm, stacks):
    """twelve workgroups of 256 with a partial last one, both ways, into 3 000 and into 2 999 streams"""
    rng = np.random.default_rng(0x3000)
    n = 3000
    words = random_words(rng, n, "recv")
    src = wm.XModemTimers(stacks("recv", n), TIMEOUT["recv"])
    try:
        src.set_state(*words)
        m = rng.integers(0, n, n).astype(np.int64)                  # with replacement: clones and drops
        m[rng.choice(n, 100, replace=False)] = -1
        m[[0, 255, 256, 2815, 2816, n - 1]] = [n - 1, 256, 255, -1, 2816, 0]   # the workgroups' edges, the last one's first lane
        both_ways(wm, stacks, "recv", src, words, m)
        both_ways(wm, stacks, "recv", src, words, rng.permutation(n)[:n - 1].astype(np.int64))
    finally:
        src.close()


def test_the_image_is_canonical(wm, stacks):
    rng = np.random.default_rng(0xCA70)
    for kind in ("recv", "tx"):
        words = random_words(rng, S, kind)
        a = wm.XModemTimers(stacks(kind, S), TIMEOUT[kind])
        a.set_state(*words)
        full = a.snapshot()
        b = wm.XModemTimers.from_snapshot(stacks(kind, S), full)
        sel = rng.integers(0, S, 33).astype(np.int64)   # an odd count (padding), streams named twice
        c = wm.XModemTimers.from_snapshot(stacks(kind, len(sel)), full, stream_map=sel)
        try:
            assert b.snapshot() == full
            assert a.snapshot(sel) == c.snapshot() and len(c.snapshot()) == 48 + 8 * 33 + 8
            assert a.snapshot([]) == b.snapshot([]) and len(a.snapshot([])) == 48
            # the size query and a buffer that is too small
            L, w = a._L, C.c_size_t(0)
            buf = (C.c_char * len(full))()
            assert L.fskhip_xmodem_timer_snapshot(a._h, None, 0, buf, len(full) - 1, C.byref(w)) == -7 and w.value == len(full) and not any(buf.raw)
            assert L.fskhip_xmodem_timer_snapshot(a._h, None, 0, None, 0, None) == -7
            assert L.fskhip_xmodem_timer_snapshot_bytes(a._h, None, 0) == len(full)
            assert L.fskhip_xmodem_timer_snapshot(a._h, None, 0, buf, len(full), None) == 0 and buf.raw == full
        finally:
            for t in (a, b, c):
                t.close()


def test_words_reached_through_polls_give_the_bytes_set_state_gives(wm):
    """a receiver's timers after start() (its NAK pending: the was-pending bit) and a sender's after send() (waiting: waited
    grows), polled under two masks so that the words differ by stream"""
    for kind in ("recv", "tx"):
        st = Stack(wm, S, kind)
        if kind == "recv":
            st.h.start(np.arange(S) % 4 != 3)
        else:
            st.h.send([b"file"] * S, np.arange(S) % 4 != 3)
        polled, given = wm.XModemTimers(st.h, 100000), wm.XModemTimers(st.h, 100000)
        try:
            for elapsed, mask in ((600, np.arange(S) % 2 == 0), (77, np.arange(S) % 3 == 0)):
                polled.poll(elapsed, mask=mask)
            words = polled.state()
            if kind == "recv":
                assert set(words["mark"].tolist()) == {0, 4} and not words["waited"].any()
            else:
                assert set(words["waited"].tolist()) == {0, 77, 600, 677} and not words["mark"].any()
            given.set_state(**words)
            assert polled.snapshot() == given.snapshot()
            assert wm.xmodem_timer_snapshot_info(polled.snapshot())["timeout_samples"] == 100000
        finally:
            polled.close()
            given.close()
            st.close()


# ---- a wait interrupted mid-way ---------------------------------------------------------------------------------------------------
RX_TIMEOUT, TX_TIMEOUT, MAX_PAYLOAD, LIMIT = 12288, 8192, 16, 1400


class Transfer:
    """test_end_to_end_a_lost_packet's loop (tests/test_gpu_xmodem_timer.py): files of 40 bytes in fragments of 16 through
    process(), a sender on processor A and a file receiver on processor B, both under timers, no mask from the host; the quanta
    that carry the second packet are silence, once, on every stream s with s % 3 == 1.  `origin[i]` is the stream of the
    uninterrupted run that stream i continues (-1: a new stream); events are kept by origin."""

    def __init__(self, wm, files):
        self.wm = wm
        self.files = files
        self.origin = np.arange(S)
        self.lost = np.arange(S) % 3 == 1
        self.engs = [wm.FSKEngine(S, BELL, precision=wm.PRECISION_F32) for _ in range(2)]
        self.A, self.B = (wm.FSKProcessorBatch(e, rx_capacity=CAP) for e in self.engs)
        self.tx, self.rx = wm.XModemSenderBatch(self.A, MAX_PAYLOAD), wm.XModemFileReceiverBatch(self.B, 64)
        self.tt, self.rt = wm.XModemTimers(self.tx, TX_TIMEOUT), wm.XModemTimers(self.rx, RX_TIMEOUT)
        self.tx.send(files)
        self.rx.start()
        self.a_out = self.b_out = np.zeros((S, Q), np.float32)
        self.silent_until = np.zeros(S, int)
        self.events = {s: [] for s in range(S)}   # by origin: (quantum, "tx" / "rx", the event record)
        self.ended = {"tx": set(), "rx": set()}
        self.q = 0

    def objects(self):
        return (self.tt, self.rt, self.tx, self.rx, self.A, self.B, *self.engs)

    def close(self):
        for x in self.objects():
            x.close()

    def quantum(self):
        q = self.q
        a_in, b_in = self.b_out, self.a_out.copy()
        b_in[self.silent_until > q] = 0
        self.a_out, self.b_out = self.A.process(a_in, Q), self.B.process(b_in, Q)
        for side, timers in (("tx", self.tt), ("rx", self.rt)):
            for s, e in zip(*timers.poll(Q)):
                assert self.origin[s] >= 0, (q, side, int(s))   # a new stream stays IDLE: it is never listed
                if side == "tx" and e["sent_len"] and e["fragment_index"] == 1 and self.lost[s] and not self.silent_until[s]:
                    self.silent_until[s] = q + 1 + -(-BURST(int(e["sent_len"])) // Q) + 4
                self.events[int(self.origin[s])].append((q, side, e.item()))
                if e["status"]:
                    self.ended[side].add(int(self.origin[s]))
        self.q += 1

    def done(self):
        return len(self.ended["tx"]) == S and len(self.ended["rx"]) == S

    def mid_wait(self):
        """what the stop asks for, each a mask over the streams: a receiver's wait for its silenced packet at least half and not
        yet all over; a was-pending bit on either side; a receiver armed for stage 2"""
        r, t = self.rt.state(), self.tt.state()
        half = self.lost & (self.silent_until > 0) & (r["waited"] >= RX_TIMEOUT // 2) & (r["waited"] < RX_TIMEOUT) & ((r["mark"] & 4) == 0)
        return half, ((r["mark"] | t["mark"]) & 4) != 0, (r["mark"] & 3) == 2

    def carry(self, m, how):
        """engines, processors, sender, receiver and both timers under one map, the samples in flight with them; `how`: "remap",
        "snapshot", or "fresh" -- the remap calls with fresh timers in the carried ones' place"""
        wm, old = self.wm, self.objects()
        if how == "snapshot":
            snaps = self.A.snapshot(), self.B.snapshot(), self.tx.snapshot(), self.rx.snapshot(), self.tt.snapshot(), self.rt.snapshot()
            self.A, self.B = (wm.FSKProcessorBatch.from_snapshot(s, stream_map=m) for s in snaps[:2])
            self.tx, self.rx = wm.XModemSenderBatch.from_snapshot(self.A, snaps[2], m), wm.XModemFileReceiverBatch.from_snapshot(self.B, snaps[3], m)
            self.tt, self.rt = wm.XModemTimers.from_snapshot(self.tx, snaps[4], m), wm.XModemTimers.from_snapshot(self.rx, snaps[5], m)
        else:
            A, B = self.A.remapped(m), self.B.remapped(m)
            tx, rx = self.tx.remapped(A, m), self.rx.remapped(B, m)
            if how == "remap":
                self.tt, self.rt = self.tt.remapped(tx, m), self.rt.remapped(rx, m)
            else:
                self.tt, self.rt = wm.XModemTimers(tx, TX_TIMEOUT), wm.XModemTimers(rx, RX_TIMEOUT)
            self.A, self.B, self.tx, self.rx = A, B, tx, rx
        assert (self.tt.timeout_samples, self.rt.timeout_samples) == (TX_TIMEOUT, RX_TIMEOUT)
        self.engs = [self.A.engine, self.B.engine]
        for x in old:
            x.close()
        old_of = np.maximum(m, 0)
        self.a_out, self.b_out = (np.where((m >= 0)[:, None], x[old_of], 0).astype(np.float32) for x in (self.a_out, self.b_out))
        self.silent_until = np.where(m >= 0, self.silent_until[old_of], 0)
        self.lost = np.where(m >= 0, self.lost[old_of], False)
        self.origin = np.where(m >= 0, self.origin[old_of], -1)

    def final(self):
        """by origin: the words of all four objects and the file; and the words of the new streams"""
        words = [x.state() for x in (self.tx, self.rx, self.tt, self.rt)]
        files = self.rx.files()
        row = lambda i: ([{k: int(v[i]) for k, v in w.items()} for w in words], files[i])   # noqa: E731
        return {int(o): row(i) for i, o in enumerate(self.origin) if o >= 0}, [row(i) for i, o in enumerate(self.origin) if o < 0]


def nak_quanta(events):
    return {s: [q for q, side, e in ev if side == "rx" and e[2] == NAK] for s, ev in events.items()}   # (an event's third word is its control byte)


@pytest.fixture(scope="module")
def files():
    rng = np.random.default_rng(0x71E)
    return [bytes(rng.integers(0, 256, 40, dtype=np.uint8)) for _ in range(S)]


@pytest.fixture(scope="module")
def uninterrupted(wm, files):
    """the whole transfer with nothing carried: the events by stream, the final words and files, its quanta, and the quantum
    after which an interrupted run stops -- the first at which the three conditions of Transfer.mid_wait hold together"""
    assert wm.xmodem.RECV_EVENT_DTYPE.names[2] == "control"
    t = Transfer(wm, files)
    stop = None
    try:
        while not t.done():
            assert t.q < LIMIT
            t.quantum()
            if stop is None and all(c.any() for c in t.mid_wait()):
                stop = t.q
        carried, new = t.final()
        assert stop is not None, "the three conditions never held together"
        assert not new and [carried[s][1] for s in range(S)] == files
        return dict(events=t.events, final=carried, quanta=t.q, stop=stop, lost=t.lost.copy())
    finally:
        t.close()


def interrupted(wm, files, ref, m, how, quanta):
    t = Transfer(wm, files)
    try:
        while t.q < ref["stop"]:
            t.quantum()
        # the stop is where a carry can go wrong: a wait for a lost packet half over, a was-pending bit, a stage-2 mark
        half, was_pending, stage2 = t.mid_wait()
        assert half.any() and was_pending.any() and stage2.any()
        assert t.events == {s: [e for e in ev if e[0] < ref["stop"]] for s, ev in ref["events"].items()}
        t.carry(m, how)
        # (the control goes on until every stream that lost its packet has sent a NAK: with fresh timers the sender's own timer
        # may end the transfer first, and the receiver's further retries say nothing)
        while t.q < quanta and not (how == "fresh" and all(nak_quanta(t.events)[s] for s in np.flatnonzero(ref["lost"]))):
            t.quantum()
        return t.events, t.final()
    finally:
        t.close()


@pytest.fixture(scope="module")
def carry_map():
    rng = np.random.default_rng(0xCA44)
    m = np.concatenate([rng.permutation(S), -np.ones(13)]).astype(np.int64)
    rng.shuffle(m)
    return m


@pytest.fixture(scope="module")
def with_fresh_timers(wm, files, uninterrupted, carry_map):
    """the control: the same stop and the same carry, but new timers over the carried handles"""
    return interrupted(wm, files, uninterrupted, carry_map, "fresh", LIMIT)[0]


@pytest.mark.parametrize("how", ["remap", "snapshot"])
def test_a_wait_interrupted_mid_way_continues_sample_for_sample(wm, files, uninterrupted, carry_map, with_fresh_timers, how):
    """The stop: the issue's three conditions (some receiver timer with 0 < waited < timeout, some was-pending bit, some receiver
    mark of stage 2), with the first one narrowed to a lost-packet stream whose wait for the silenced packet is at least half
    over.  Unnarrowed, the three first hold together while the FIRST packet is received, before anything is lost; timers
    re-armed there re-arm again at that packet's ACK, and the control below could not tell a carried timer from a fresh one."""
    ref = uninterrupted
    lost = np.flatnonzero(ref["lost"])
    assert ref["stop"] is not None and len(lost) > 20
    events, (final, new) = interrupted(wm, files, ref, carry_map, how, ref["quanta"])
    # every carried stream lists the same events at the same quanta, and ends with the same words -- timers' included -- and file
    assert sorted(final) == list(range(S))
    for s in range(S):
        assert events[s] == ref["events"][s], (s, events[s], ref["events"][s])
        assert final[s] == ref["final"][s], s
    naks = nak_quanta(events)
    assert [len(naks[s]) for s in range(S)] == ref["lost"].astype(int).tolist()   # exactly one timeout NAK where the packet was lost
    assert all(ref["stop"] <= naks[s][0] for s in lost)                           # and it came after the carry
    # the 13 new streams stay IDLE with timers 0 and 0
    assert len(new) == 13
    for words, data in new:
        assert words[0]["state"] == 0 and words[1]["state"] == 0 and words[2] == dict(waited=0, mark=0) and words[3] == dict(waited=0, mark=0) and data == b""
    # the control: fresh timers start the interrupted wait again, so the timeout NAK comes later
    ref_naks, fresh_naks = nak_quanta(ref["events"]), nak_quanta(with_fresh_timers)
    later = [s for s in lost if fresh_naks[s] and fresh_naks[s][0] > ref_naks[s][0]]
    assert later, (ref_naks, fresh_naks)
    assert all(fresh_naks[s][0] - ref_naks[s][0] >= RX_TIMEOUT // 2 // Q - 1 for s in later)   # by the half of the wait that was lost


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def c_remap(dst, src, m):
    m = np.ascontiguousarray(m, np.int64)
    L = dst._L
    rc = L.fskhip_xmodem_timer_remap(dst._h, src._h, m.ctypes.data if len(m) else None, len(m))
    return rc, L.fskhip_last_error().decode()


def c_restore(dst, image, m):
    m = np.ascontiguousarray(m, np.int64)
    L = dst._L
    rc = L.fskhip_xmodem_timer_restore(dst._h, image, len(image), m.ctypes.data if len(m) else None, len(m))
    return rc, L.fskhip_last_error().decode()


def test_refusals_leave_the_destination_as_it_was(wm, stacks):
    rng = np.random.default_rng(0x4EF)
    ident = np.arange(S, dtype=np.int64)
    made = []

    def timers(kind, words=None, n=S):
        t = wm.XModemTimers(stacks(kind, n), TIMEOUT[kind])
        made.append(t)
        if words is not None:
            t.set_state(*words)
        return t
    try:
        words = {k: random_words(rng, S, k) for k in ("recv", "tx")}
        src = {k: timers(k, words[k]) for k in ("recv", "tx")}
        image = {k: src[k].snapshot() for k in ("recv", "tx")}
        # a fresh destination that holds words: remapped into once (it is still fresh), under a map that is not the identity
        first = rng.permutation(S).astype(np.int64)
        dst = {k: timers(k) for k in ("recv", "tx")}
        for k in dst:
            assert c_remap(dst[k], src[k], first)[0] == 0
        held = {k: take(words[k], first) for k in dst}

        def refused(k, got, *texts):
            rc, msg = got
            assert rc == E_INVALID and all(t in msg for t in texts), msg
            assert words_of(dst[k]) == held[k], msg
        for k, other in (("recv", "tx"), ("tx", "recv")):
            d = dst[k]
            # a kind mismatch, both ways, for remap and for restore
            refused(k, c_remap(d, src[other], ident), "different kinds", "receiver", "sender")
            refused(k, c_restore(d, image[other], ident), "the snapshot is of kind %d (%s), this timer's is %d (%s)" % (KIND_NUMBER[other], other, KIND_NUMBER[k], k))
            with pytest.raises(ValueError, match="the snapshot is of kind %r, the handle's is %r" % (other, k)):
                wm.XModemTimers.from_snapshot(stacks(k, S), image[other])
            # n_map off by one, either way
            refused(k, c_remap(d, src[k], ident[:-1]), "n_map 69 != the destination's 70 streams")
            refused(k, c_remap(d, src[k], np.append(ident, 0)), "n_map 71 != the destination's 70 streams")
            refused(k, c_restore(d, image[k], ident[:-1]), "n_map 69 != the destination's 70 streams")
            # an entry equal to the source's stream count; one below -1
            bad = ident.copy()
            bad[41] = S
            refused(k, c_remap(d, src[k], bad), "map[41] = 70, the source has 70 streams")
            refused(k, c_restore(d, image[k], bad), "map[41] = 70, the snapshot has 70 records")
            bad[7] = -2
            refused(k, c_remap(d, src[k], bad), "map[7] = -2")
            # dst is src
            refused(k, c_remap(d, d, ident), "dst and src are the same timer")
            # a damaged image
            refused(k, c_restore(d, image[k][:-16], ident), "do not match the layout")
            # a second remap into the still-fresh destination replaces the first as a whole; so does a restore
            second = rng.integers(-1, S, S).astype(np.int64)
            assert c_remap(d, src[k], second)[0] == 0 and words_of(d) == take(words[k], second)
            assert c_restore(d, image[k], first)[0] == 0 and words_of(d) == held[k]
        # a destination that has polled, been reset, been given words: no longer fresh
        # (a sender that waits on every stream, and words that a poll moves in a known way: 5 samples waited, no mark)
        five = timers("tx", (np.full(S, 5, np.uint32), np.zeros(S, np.uint32)))
        for how in ("poll", "overflowing poll", "reset", "set_state"):
            sender = Stack(wm, S, "tx")
            made.append(sender)
            sender.h.send([b"file"] * S)
            d = dst["tx"] = wm.XModemTimers(sender.h, 1000)
            made.insert(0, d)
            assert c_remap(d, five, ident)[0] == 0
            held["tx"] = [[5] * S, [0] * S]
            if how == "poll":
                assert len(d.poll(600)[0]) == 0
                held["tx"][0] = [605] * S
            elif how == "overflowing poll":   # every stream would be aborted and listed, the lists hold none: nothing was polled -- but a call was made
                ne = C.c_uint32(0)
                assert d._L.fskhip_xmodem_tx_poll_timed_host(d._h, 2000, None, None, None, None, 0, C.byref(ne)) == -7 and ne.value == S
            elif how == "reset":
                d.reset(3)
                held["tx"][0][3] = 0
            else:
                d.set_state(mark=np.full(S, 4, np.uint32))
                held["tx"][1] = [4] * S
            assert words_of(d) == held["tx"], how
            refused("tx", c_remap(d, src["tx"], ident), "used already", "timed poll, reset or state_set", "remap into a freshly created timer")
            refused("tx", c_restore(d, image["tx"], ident), "used already", "restore into a freshly created timer")
        # a timer whose handle was closed first, as the source and as the destination
        gone = Stack(wm, S, "tx")
        made.append(gone)
        orphan = wm.XModemTimers(gone.h, 1000)
        made.insert(0, orphan)
        gone.h.close()
        d = dst["tx"] = timers("tx")
        held["tx"] = [[0] * S, [0] * S]
        refused("tx", c_remap(d, orphan, ident), "the timer's sender has been destroyed")
        rc, msg = c_remap(orphan, src["tx"], ident)
        assert rc == E_INVALID and "the timer's sender has been destroyed" in msg
        rc, msg = c_restore(orphan, image["tx"], ident)
        assert rc == E_INVALID and "the timer's sender has been destroyed" in msg
        w = C.c_size_t(0)
        assert orphan._L.fskhip_xmodem_timer_snapshot(orphan._h, None, 0, None, 0, C.byref(w)) == E_INVALID
        with pytest.raises(ValueError, match="handle has been closed"):
            orphan.remapped(stacks("tx", S), ident)
    finally:
        for x in made:
            x.close()
