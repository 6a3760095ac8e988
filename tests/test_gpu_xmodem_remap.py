"""The resident XModem handles through remap, snapshot and restore on the GPU (include/fskhip_next.h: fskhip_xmodem_{rx,tx,recv}_remap,
_snapshot, _restore; remapped / snapshot / from_snapshot of the three Python classes).

The oracle is the Python models of the three handles (tests/xmodem_rx_ref.py, xmodem_tx_ref.py, xmodem_recv_ref.py over
drain_ref.Rings): a batch is (words, files), a remap of it is plain re-indexing -- a copy for a clone, a new transport's words and no
file for -1 --, and nothing in the expectation calls the code under test.  Ring states are planted as the other XModem tests plant
them (a fresh processor image rewritten in numpy and restored), so every poll of a schedule runs on a processor of its own, which the
handle reaches through one more identity remap: the carried state is re-examined against the model at every step, the sender's file
through the packets it goes on transmitting (the pending payloads in the processor image against a twin that modulated the model's
packets).  Every carry -- each kind, each map, by remap and by snapshot + from_snapshot -- is followed by POLLS (20) such polls.
All comparisons are exact."""
import copy
import struct

import numpy as np
import pytest

import xmodem_recv_ref as recv_ref
import xmodem_rx_ref as rx_ref
import xmodem_tx_ref as tx_ref
from drain_ref import Rings
from test_gpu_rx_drain_sparse import Bench
from test_processor_snapshot_cpu import _checksum

pytestmark = pytest.mark.gpu

E_INVALID, E_OVERFLOW = -1, -7
CAP, FILE_CAP, MAX_RETRIES = 300, 600, 3
POLLS = 20   # further polls after every carry, on either path
LENGTHS = [0, 1, 15, 16, 17, 127, 128, 129, 600]
KINDS = ("rx", "tx", "recv")


def rings_of(contents, cap, rng):
    """Rings holding contents[s], from a random readIndex (so about half the spans wrap)"""
    S = len(contents)
    r = rng.integers(0, cap, S)
    ring = rng.integers(1, 256, (S, cap), dtype=np.uint8)
    n = np.array([len(b) for b in contents], np.int64)
    for s, b in enumerate(contents):
        ring[s, (r[s] + np.arange(len(b))) % cap] = np.frombuffer(b, np.uint8)
    return Rings(r, n, ring)


def modulate_rows(proc, rows):
    if rows:
        proc.modulate([rows.get(s, b"") for s in range(proc.n_streams)], mask=[s in rows for s in range(proc.n_streams)])


class Model:
    """one kind of handle as its Python model: words (dict of arrays), files (list; None: the sender holds none), parameters"""

    def __init__(self, kind, words, files, max_payload=128):
        self.kind, self.words, self.files, self.max_payload = kind, {k: np.array(v, np.uint32) for k, v in words.items()}, list(files), max_payload
        self.n = len(self.files)

    # ---- generators (the ref modules'), with the issue's file lengths
    @classmethod
    def random(cls, kind, rng, n, max_payload=128):
        if kind == "rx":
            words = {"expected": rx_ref.start_sequences(rng, n), "packets": rng.integers(0, 1000, n), "dropped": rng.integers(0, 1000, n)}
            return cls(kind, words, [None] * n, max_payload)
        if kind == "tx":
            _, words, files = tx_ref.random_case(rng, n, 16, max_payload, MAX_RETRIES)
            for s in range(n):   # the lengths that put spans at every alignment; the words stay inside the new file
                if files[s] is not None:
                    files[s] = bytes(rng.integers(0, 256, LENGTHS[int(rng.integers(0, len(LENGTHS)))], dtype=np.uint8))
                    nf = len(tx_ref.fragments(files[s], max_payload))
                    st = words["state"][s]
                    words["fragment_index"][s] = nf if st == tx_ref.WAIT_FINAL_ACK else 0 if st == tx_ref.WAIT_NAK else int(rng.integers(0, nf))
            return cls(kind, words, files, max_payload)
        _, words, files = recv_ref.random_case(rng, n, CAP, max_payload, MAX_RETRIES, FILE_CAP)
        for s in range(n):
            if rng.random() < 0.7:
                files[s] = bytes(rng.integers(0, 256, LENGTHS[int(rng.integers(0, len(LENGTHS)))], dtype=np.uint8))
                words["file_len"][s] = len(files[s])
        return cls(kind, words, files, max_payload)

    def fresh(self, n):
        words = {"rx": lambda: {"expected": np.ones(n), "packets": np.zeros(n), "dropped": np.zeros(n)}, "tx": lambda: tx_ref.fresh_words(n),
                 "recv": lambda: recv_ref.fresh_words(n)}[self.kind]()
        return Model(self.kind, words, [None if self.kind != "recv" else b""] * n, self.max_payload)

    def remapped(self, m):
        """plain re-indexing: a copy per clone, a new transport for -1"""
        new = self.fresh(len(m))
        for i, src in enumerate(m):
            if src >= 0:
                for k in self.words:
                    new.words[k][i] = self.words[k][src]
                new.files[i] = copy.deepcopy(self.files[src])
        return new

    def contents(self, rng, cap=CAP, share=1.0):
        """what the line delivers to each stream next, from the ref modules' generators; share: the part of the streams that hears
        anything this time (drawn anew at every call)"""
        on = rng.random(self.n) < share
        if self.kind == "rx":
            return [rx_ref.traffic(rng, cap, int(e)) if on[s] and rng.random() < 0.8 else b"" for s, e in enumerate(self.words["expected"])]
        if self.kind == "tx":
            return [tx_ref.random_reply(rng, cap) if on[s] else b"" for s in range(self.n)]
        return [recv_ref.random_content(rng, cap, int(e), self.max_payload) if on[s] else b"" for s, e in enumerate(self.words["expected"])]

    def poll(self, rings):
        """(streams, events as a list, {stream: bytes handed to the modulator}); the model moves on"""
        if self.kind == "rx":
            streams, results, offsets, data, _, state = rx_ref.poll_ref(rings, self.words["expected"], None, self.words["packets"], self.words["dropped"])
            self.words = state
            return streams, (results.tolist(), offsets.tolist(), data.tobytes()), {}
        if self.kind == "tx":
            streams, events, _, self.words, sent = tx_ref.step_ref(rings, self.words, self.files, self.max_payload, MAX_RETRIES)
            return streams, events.tolist(), sent
        streams, events, _, self.words, self.files, sent = recv_ref.step_ref(rings, self.words, self.files, FILE_CAP, MAX_RETRIES)
        return streams, events.tolist(), sent


class Device:
    """the handle under test over planted processors"""

    def __init__(self, wm, benches):
        self.wm, self.benches, self.open = wm, benches, []

    def bench(self, n):
        if n not in self.benches:
            self.benches[n] = Bench(n, CAP)
        return self.benches[n]

    def plant(self, model, rings):
        """a processor with these rings and a handle over it that was given the model's state by hand: send / set_files + set_state"""
        proc = self.bench(model.n).clone(rings)
        if model.kind == "rx":
            h = self.wm.XModemReceiverBatch(proc)
            h.set_state(**model.words)
        elif model.kind == "tx":
            h = self.wm.XModemSenderBatch(proc, model.max_payload, MAX_RETRIES)
            has = np.array([f is not None for f in model.files])
            # two send calls, the first with files that are replaced: the packed store holds dead bytes and spans start anywhere
            first = has & (np.arange(model.n) % 3 != 0)
            if first.any():
                h.send([None if f is None else bytes(len(f) + 5) for f in model.files], mask=first)
                h.set_state(state=np.zeros(model.n, np.uint32))
            if has.any():
                h.send(model.files, mask=has)
            h.set_state(**model.words)
        else:
            h = self.wm.XModemFileReceiverBatch(proc, FILE_CAP, MAX_RETRIES)
            h.set_files(model.files)
            h.set_state(**model.words)
        self.open.append(h)
        return proc, h

    def poll(self, kind, h):
        if kind == "rx":
            streams, results, offsets, data = h.poll()
            return streams, (results.tolist(), offsets.tolist(), data.tobytes())
        streams, events = h.poll()
        return streams, events.tolist()

    def release(self, proc):
        """closes a planted processor (and its engine) that no handle polls any more"""
        for b in self.benches.values():
            if proc in b.made:
                b.made.remove(proc)
        proc.close()
        proc.engine.close()

    def close(self):
        for h in self.open:
            h.close()
        self.open = []
        for b in self.benches.values():
            b.close()
            b.made = []


@pytest.fixture
def dev():
    import webaudio_modem_amd as wm
    d = Device(wm, {})
    yield d
    d.close()
    for b in d.benches.values():
        b.close()


def same_state(h, model):
    st = h.state()
    assert set(st) == set(model.words)
    for k in st:
        assert np.array_equal(st[k], model.words[k]), (k, np.flatnonzero(st[k] != model.words[k])[:8])
    if model.kind == "recv":
        assert h.files() == model.files


def pending_image(dev, n, rings_after, sent):
    twin = dev.bench(n).clone(rings_after)
    modulate_rows(twin, sent)
    image = twin.snapshot().processor
    dev.release(twin)
    return image


def run_polls(dev, h, model, rng, polls=POLLS, share=1.0):
    """`polls` polls, each on a processor of its own with fresh line content for a part `share` of the streams; the handle of each
    step is closed, with its processor, once the next has taken over"""
    ident = np.arange(model.n, dtype=np.int64)
    mine = None
    for _ in range(polls):
        rings = rings_of(model.contents(rng, share=share), CAP, rng)
        proc = dev.bench(model.n).clone(rings)
        nxt = h.remapped(proc, ident)
        if mine is not None:
            mine[0].close()
            dev.release(mine[1])
        h, mine = nxt, (nxt, proc)
        before = copy.deepcopy(model)
        want_streams, want_events, sent = model.poll(rings)
        got_streams, got_events = dev.poll(model.kind, h)
        assert np.array_equal(got_streams, want_streams) and got_events == want_events
        same_state(h, model)
        if model.kind != "rx":   # what was transmitted: the pending payloads, against a twin that modulated the model's bytes
            after = {"tx": lambda: tx_ref.step_ref(rings, before.words, before.files, model.max_payload, MAX_RETRIES)[2],
                     "recv": lambda: recv_ref.step_ref(rings, before.words, before.files, FILE_CAP, MAX_RETRIES)[2]}[model.kind]()
            assert proc.snapshot().processor == pending_image(dev, model.n, after, sent)
    if mine is not None:
        mine[0].close()
        dev.release(mine[1])


def sender_files(dev, h, model):
    """the sender's files as it would transmit them: fragment k of every stream that has one, for every k, each from a handle carried
    onto a processor whose rings hold one NAK"""
    ident = np.arange(model.n, dtype=np.int64)
    frags = [[] if f is None else tx_ref.fragments(f, model.max_payload) for f in model.files]
    for k in range(max(len(f) for f in frags) if frags else 0):
        sel = np.array([k < len(f) for f in frags])
        rings = rings_of([bytes([tx_ref.NAK]) if x else b"" for x in sel], CAP, np.random.default_rng(k))
        proc = dev.bench(model.n).clone(rings)
        hk = h.remapped(proc, ident)
        dev.open.append(hk)
        words = {q: v.copy() for q, v in model.words.items()}
        words["state"] = np.where(sel, tx_ref.WAIT_NAK, tx_ref.IDLE).astype(np.uint32)
        words["fragment_index"] = np.where(sel, k, 0).astype(np.uint32)
        hk.set_state(**words)
        hk.poll()
        _, _, after, _, sent = tx_ref.step_ref(rings, words, model.files, model.max_payload, MAX_RETRIES)
        assert all(sent[s][4:-2] == frags[s][k] for s in np.flatnonzero(sel))
        assert proc.snapshot().processor == pending_image(dev, model.n, after, sent)
        hk.close()
        dev.open.remove(hk)
        dev.release(proc)


def maps_for(rng, n_src):
    if n_src == 1:
        return {"identity-1": np.array([0], np.int64)}
    shrink = np.sort(rng.choice(n_src, 50, replace=False)).astype(np.int64)
    grow = np.concatenate([np.arange(n_src), -np.ones(14)]).astype(np.int64)
    rng.shuffle(grow)
    perm = rng.integers(0, n_src, n_src).astype(np.int64)          # with replacement: clones and drops
    assert len(set(perm)) < n_src
    return {"shrink": shrink, "grow": grow, "clones": perm, "all-new": -np.ones(n_src, np.int64)}


def carried(dev, h, src_proc, model, m, how):
    """the handle carried through `m` onto the processor the engine and the processor were carried onto first"""
    if how == "remap":
        proc = src_proc.remapped(m)
        dev.bench(model.n).made.append(proc)
        nxt = h.remapped(proc, m)
    else:
        snaps = (src_proc.snapshot(), h.snapshot())
        proc = dev.wm.FSKProcessorBatch.from_snapshot(snaps[0], stream_map=m)
        dev.bench(model.n).made.append(proc)
        nxt = type(h).from_snapshot(proc, snaps[1], stream_map=m)
    dev.open.append(nxt)
    return nxt


MAP_NAMES = ("shrink", "grow", "clones", "all-new", "identity-1")


@pytest.mark.parametrize("name", MAP_NAMES)
@pytest.mark.parametrize("kind,max_payload", [("rx", 128), ("tx", 128), ("tx", 7), ("recv", 128), ("recv", 7)])
def test_remap_and_restore_continue_the_model_through_every_map(dev, kind, max_payload, name):
    """one map per case: the carried state against the re-indexed model, by remap and by snapshot + from_snapshot, POLLS further polls
    behind each, the two images byte for byte, and the source as it was"""
    rng = np.random.default_rng(0x5E0 + max_payload + KINDS.index(kind) + 16 * MAP_NAMES.index(name))
    n_src = 1 if name == "identity-1" else 70
    model = Model.random(kind, rng, n_src, max_payload)
    src_rings = rings_of(model.contents(rng), CAP, rng)
    src_proc, h = dev.plant(model, src_rings)
    same_state(h, model)
    m = maps_for(rng, n_src)[name]
    want = model.remapped(m)
    digests = []
    for how in ("remap", "restore"):
        nxt = carried(dev, h, src_proc, model, m, how)
        assert nxt.n_streams == len(m)
        same_state(nxt, want)
        digests.append(nxt.snapshot())
        if kind == "tx" and max_payload == 128:
            sender_files(dev, nxt, want)
        run_polls(dev, nxt, copy.deepcopy(want), np.random.default_rng(7))   # (the same line content on either path)
    assert digests[0] == digests[1]       # snapshot -> from_snapshot lands where the remap does
    if (m >= 0).all():
        assert digests[0] == h.snapshot(streams=m)
    info = dev.wm.xmodem_snapshot_info(digests[0])
    assert info["kind"] == 1 + KINDS.index(kind) and info["n_streams"] == len(m)
    assert info["file_bytes"] == sum(len(f) for f in want.files if f)
    assert (info["param0"], info["param1"]) == {"rx": (0, 0), "tx": (max_payload, MAX_RETRIES), "recv": (FILE_CAP, MAX_RETRIES)}[kind]
    # src, polled after all of this, is unchanged
    same_state(h, model)
    want_streams, want_events, _ = model.poll(src_rings)
    got_streams, got_events = dev.poll(kind, h)
    assert np.array_equal(got_streams, want_streams) and got_events == want_events
    same_state(h, model)


@pytest.mark.parametrize("kind", KINDS)
def test_3000_streams_take_more_than_one_round_of_workgroups(dev, kind):
    rng = np.random.default_rng(0x3000 + KINDS.index(kind))
    model = Model.random(kind, rng, 3000, 128)
    src_proc, h = dev.plant(model, rings_of([b""] * 3000, CAP, rng))
    m = rng.integers(-1, 3000, 3000).astype(np.int64)
    want = model.remapped(m)
    a = carried(dev, h, src_proc, model, m, "remap")
    same_state(a, want)
    b = carried(dev, h, src_proc, model, m, "restore")
    same_state(b, want)
    assert a.snapshot() == b.snapshot()
    # the schedule, with a twentieth of the streams hearing something at each poll (the model is Python: 60 000 full stream-steps
    # would take this case out of the seconds the suite allows; every stream still takes part in every poll, most with an empty ring)
    run_polls(dev, a, want, rng, share=0.05)


def test_two_senders_with_different_store_histories_give_one_image(dev):
    wm = dev.wm
    rng = np.random.default_rng(0x517)
    S = 70
    files = [bytes(rng.integers(0, 256, LENGTHS[s % len(LENGTHS)], dtype=np.uint8)) if s % 5 else None for s in range(S)]
    has = np.array([f is not None for f in files])
    rings = rings_of([b""] * S, CAP, rng)
    a = wm.XModemSenderBatch(dev.bench(S).clone(rings), 128, MAX_RETRIES)
    b = wm.XModemSenderBatch(dev.bench(S).clone(rings), 128, MAX_RETRIES)
    dev.open += [a, b]
    a.send(files, mask=has)
    # b: other files first, replaced one half at a time in descending halves, so the store's order and dead bytes differ
    b.send([bytes(700) for _ in files], mask=has)
    idle = dict(state=np.zeros(S, np.uint32))
    for part in (has & (np.arange(S) >= S // 2), has & (np.arange(S) < S // 2)):
        b.set_state(**idle)
        b.send(files, mask=part)
    b.set_state(**a.state())
    assert a.snapshot() == b.snapshot()
    sel = rng.integers(0, S, 40)
    assert a.snapshot(sel) == b.snapshot(sel)
    # the image is the documented layout
    img = a.snapshot()
    head = struct.unpack("<8I2Q", img[:48])
    live = [f for f in files if f is not None]
    assert head[:8] == (0x584B5346, 1, 48, 2, S, 8, 128, MAX_RETRIES) and head[9] == sum(map(len, live))
    assert len(img) == 48 + 32 * S + (head[9] + 15) // 16 * 16
    assert img[48 + 32 * S:48 + 32 * S + head[9]] == b"".join(live) and not any(img[48 + 32 * S + head[9]:])
    blob = bytearray(img)
    blob[32:40] = bytes(8)
    assert head[8] == _checksum(blob)
    table = np.frombuffer(img[48:48 + 32 * S], "<u4").reshape(S, 8)
    assert table[:, 7].tolist() == has.astype(int).tolist() and table[:, 6].tolist() == [len(f) if f is not None else 0 for f in files]


def test_refusals_leave_the_destination_as_it_was(dev):
    wm, L = dev.wm, dev.wm._lib.lib()
    rng = np.random.default_rng(0x4EF)
    S = 70
    ident = np.arange(S, dtype=np.int64)
    empty = rings_of([b""] * S, CAP, rng)
    for kind in KINDS:
        model = Model.random(kind, rng, S, 128)
        if kind == "recv":   # one file of exactly file_capacity, stream 9's
            for s in range(S):
                model.files[s] = bytes(range(200)) * 3 if s == 9 else model.files[s][:599]
                model.words["file_len"][s] = len(model.files[s])
        src_proc, h = dev.plant(model, empty)
        fresh = model.fresh(S)
        make = {"rx": lambda p, **kw: wm.XModemReceiverBatch(p), "tx": lambda p, **kw: wm.XModemSenderBatch(p, kw.get("max_payload", 128), MAX_RETRIES),
                "recv": lambda p, **kw: wm.XModemFileReceiverBatch(p, kw.get("file_cap", FILE_CAP), MAX_RETRIES)}[kind]
        dst = make(dev.bench(S).clone(empty))
        dev.open.append(dst)
        fn = lambda what: getattr(L, "fskhip_xmodem_%s_%s" % (kind, what))   # noqa: E731

        def refused(rc, pattern, dst=dst):
            msg = L.fskhip_last_error().decode()
            assert rc == E_INVALID and pattern in msg, (kind, rc, msg)
            same_state(dst, fresh)
        refused(fn("remap")(dst._h, h._h, ident.ctypes.data, S - 1), "n_map 69 != the destination's 70 streams")
        bad = ident.copy()
        bad[13] = S
        refused(fn("remap")(dst._h, h._h, bad.ctypes.data, S), "map[13] = 70")
        bad[13] = -2
        refused(fn("remap")(dst._h, h._h, bad.ctypes.data, S), "map[13] = -2")
        refused(fn("remap")(dst._h, dst._h, ident.ctypes.data, S), "the same handle")
        snap = h.snapshot()
        flipped = bytearray(snap)
        flipped[32] ^= 1
        flipped = bytes(flipped)
        refused(fn("restore")(dst._h, flipped, len(flipped), ident.ctypes.data, S), "checksum")
        refused(fn("restore")(dst._h, snap, len(snap), ident.ctypes.data, S - 1), "n_map 69")
        if kind == "tx":
            other = make(dev.bench(S).clone(empty), max_payload=64)
            dev.open.append(other)
            refused(fn("remap")(other._h, h._h, ident.ctypes.data, S), "max_payload_size differs", dst=other)
            refused(fn("restore")(other._h, snap, len(snap), ident.ctypes.data, S), "max_payload_size differs", dst=other)
        if kind == "recv":
            small = make(dev.bench(S).clone(empty), file_cap=599)
            dev.open.append(small)
            m = np.roll(ident, 3)   # stream 12 of the destination would take stream 9's 600 bytes
            refused(fn("remap")(small._h, h._h, m.ctypes.data, S), "the file of stream 12 (source stream 9) has 600 bytes", dst=small)
            refused(fn("restore")(small._h, snap, len(snap), m.ctypes.data, S), "the file of stream 12 (record 9) has 600 bytes", dst=small)
            # without that stream the smaller capacity is fine
            m[12] = -1
            assert fn("remap")(small._h, h._h, m.ctypes.data, S) == 0
            small.file_capacity = 599
            want = model.remapped(m)
            same_state(small, want)
        # a short cap: the size comes back, nothing is written
        import ctypes as C
        w = C.c_size_t(0)
        buf = (C.c_char * len(snap))()
        assert fn("snapshot")(h._h, None, 0, buf, len(snap) - 1, C.byref(w)) == E_OVERFLOW and w.value == len(snap) and not any(buf.raw)
        assert fn("snapshot")(h._h, None, 0, None, 0, C.byref(w)) == E_OVERFLOW and w.value == len(snap) == fn("snapshot_bytes")(h._h, None, 0)
        # the destination is still fresh: a remap succeeds; after that it works, and once polled it is a used one
        assert fn("remap")(dst._h, h._h, ident.ctypes.data, S) == 0
        same_state(dst, model)
        dst.poll()
        assert fn("remap")(dst._h, h._h, ident.ctypes.data, S) == E_INVALID and "used already" in L.fskhip_last_error().decode()
        assert fn("restore")(dst._h, snap, len(snap), ident.ctypes.data, S) == E_INVALID and "used already" in L.fskhip_last_error().decode()


def _transfer(files, max_payload, perm=None, interrupt_at=None, Q=2048, limit=600):
    """an XModemSenderBatch on processor A and an XModemFileReceiverBatch on processor B, cross-wired by process() quanta -- A's
    output is B's input and B's output is A's input --, both polled every fourth quantum, until every stream of both has ended.
    interrupt_at: after that many quanta both engines, both processors and both handles are snapshotted and closed, then restored
    under `perm`, the samples in flight permuted with them, and the schedule goes on.  Returns (files received, sender words,
    receiver words, quanta)."""
    import webaudio_modem_amd as wm
    S = len(files)
    eng_a, eng_b = (wm.FSKEngine(S, dict(baudRate=1200), precision=wm.PRECISION_F32) for _ in range(2))
    A, B = (wm.FSKProcessorBatch(e, rx_capacity=CAP, clear_rx_on_tx_complete=True) for e in (eng_a, eng_b))
    tx, rx = wm.XModemSenderBatch(A, max_payload), wm.XModemFileReceiverBatch(B, FILE_CAP)
    tx.send(files)
    rx.start()
    a_out = b_out = np.zeros((S, Q), np.float32)
    tx_end, rx_end = {}, {}
    for quantum in range(limit):
        if quantum == interrupt_at:
            snaps = A.snapshot(), B.snapshot(), tx.snapshot(), rx.snapshot()
            for x in (tx, rx, A, B, eng_a, eng_b):
                x.close()
            A, B = (wm.FSKProcessorBatch.from_snapshot(s, stream_map=perm) for s in snaps[:2])
            eng_a, eng_b = A.engine, B.engine
            tx, rx = wm.XModemSenderBatch.from_snapshot(A, snaps[2], perm), wm.XModemFileReceiverBatch.from_snapshot(B, snaps[3], perm)
            a_out, b_out = a_out[perm], b_out[perm]
            tx_end, rx_end = ({i: e[int(p)] for i, p in enumerate(perm) if int(p) in e} for e in (tx_end, rx_end))
        a_out, b_out = A.process(b_out, Q), B.process(a_out, Q)
        if quantum % 4 == 3:
            for s, ev in tx.poll_active().items():
                if ev["status"] != tx_ref.PROGRESS:
                    tx_end[s] = ev["status"]
            for s, ev in rx.poll_active().items():
                if ev["status"] != recv_ref.PROGRESS:
                    rx_end[s] = ev["status"]
            if len(tx_end) == S and len(rx_end) == S:
                break
    assert tx_end == {s: tx_ref.DONE for s in range(S)} and rx_end == {s: recv_ref.DONE for s in range(S)}, (tx_end, rx_end, quantum)
    out = rx.files(), tx.state(), rx.state(), quantum
    for x in (tx, rx, A, B, eng_a, eng_b):
        x.close()
    return out


def test_a_transfer_interrupted_mid_way_and_restored_under_a_permutation_ends_as_the_uninterrupted_one():
    rng = np.random.default_rng(0xE2E5)
    S, max_payload = 70, 128
    sizes = [0, 1, 127, 128, 129, 600] + [int(n) for n in rng.integers(0, 601, S - 6)]
    files = [bytes(rng.integers(0, 256, n, dtype=np.uint8)) for n in sizes]
    perm = rng.permutation(S).astype(np.int64)
    got_files, tx_words, rx_words, quanta = _transfer(files, max_payload)
    assert got_files == files
    cut = 4 * (quanta // 8)   # mid-transfer, at a quantum boundary
    files2, tx2, rx2, quanta2 = _transfer(files, max_payload, perm=perm, interrupt_at=cut)
    assert quanta2 == quanta
    assert files2 == [files[p] for p in perm]
    for k in tx_words:
        assert np.array_equal(tx2[k], tx_words[k][perm]), k
    for k in rx_words:
        assert np.array_equal(rx2[k], rx_words[k][perm]), k
    n_frag = np.array([len(tx_ref.fragments(f, max_payload)) for f in files])
    assert np.array_equal(tx_words["packets_sent"], n_frag + 1) and np.array_equal(rx_words["packets_received"], n_frag)
