"""The resident XModem sender on the GPU (include/fskhip_next.h: fskhip_xmodem_tx_*; XModemSenderBatch).  Ring states are planted as
tests/test_gpu_xmodem_rx.py plants them -- the processor image of a fresh batch rewritten in numpy and restored --, sender words go
in through send() + set_state(), pending modulations through modulate(); one poll is then compared with step_ref
(tests/xmodem_tx_ref.py, pinned to the real XModemTransport by the golden set): the lists, the events, every sender word, and the
whole processor image -- every ring word, tx_pending / tx_len / tx_n_payload and the payload bytes -- against a twin processor
that was given step_ref's rings and step_ref's packets through fskhip_processor_modulate_host.  All comparisons are exact.  Shapes:
a lone lane, a partial wave, one lane into the next wave, one into the next workgroup, and 66 000 streams (258 workgroup pairs:
the totals kernel makes a second pass); capacities 16 and 1 024 take the 16-byte tile path (one tile and sixteen), 100 the byte
path; spans wrap the ring's end."""
import ctypes as C

import numpy as np
import pytest

import drain_ref
import xmodem_tx_ref as ref
from test_gpu_rx_drain_sparse import Bench, _hip_runtime

pytestmark = pytest.mark.gpu

E_INVALID, E_OVERFLOW, E_BUSY = -1, -7, -8


@pytest.fixture
def bench():
    made = []

    def make(n_streams, cap):
        made.append(Bench(n_streams, cap))
        return made[-1]
    yield make
    for b in made:
        b.close()


def premod_rows(rng_mask):
    """{stream: the payload of a modulation that is pending before the poll} for the streams of a bool array"""
    return {int(s): bytes([0x40 + s % 50]) * (1 + s % 7) for s in np.flatnonzero(rng_mask)}


def modulate_rows(proc, rows):
    if rows:
        proc.modulate([rows.get(s, b"") for s in range(proc.n_streams)], mask=[s in rows for s in range(proc.n_streams)])


def planted(b, rings, words, files, max_payload, max_retries, premod=None):
    """a clone of the batch with these rings (and the pending modulations premod: {stream: payload}) and a sender over it with these words"""
    proc = b.clone(rings)
    tx = b.wm.XModemSenderBatch(proc, max_payload, max_retries)
    has = np.array([f is not None for f in files])
    if has.any():
        tx.send(files, mask=has)
    tx.set_state(**words)
    modulate_rows(proc, premod)
    return proc, tx


def twin_image(b, rings_after, sent, premod=None):
    """the image of a processor that holds step_ref's rings and was given step_ref's packets through modulate()"""
    twin = b.clone(rings_after)
    modulate_rows(twin, premod)
    modulate_rows(twin, sent)
    return twin.snapshot().processor


def same_words(got, want):
    return all(np.array_equal(got[k], want[k]) for k in ref.WORDS)


def check_poll(b, proc, tx, rings, words, files, max_payload, max_retries, mask=None, abort=None, premod=None):
    pending = None if premod is None else np.array([s in premod for s in range(b.n_streams)])
    want = ref.step_ref(rings, words, files, max_payload, max_retries, mask=mask, abort=abort, pending=pending)
    streams, events = tx.poll(mask, abort)
    assert streams.dtype == np.uint32 and events.dtype == ref.EVENT_DTYPE
    assert np.array_equal(streams, want[0]) and events.tolist() == want[1].tolist()
    assert same_words(tx.state(), want[3])
    assert proc.snapshot().processor == twin_image(b, want[2], want[4], premod)
    return want


@pytest.mark.parametrize("n_streams", [1, 63, 65, 257])
def test_lists_events_rings_words_and_modulations_match_step_ref(bench, n_streams):
    rng = np.random.default_rng(0x7A0 + n_streams)
    seen = set()
    for cap, max_payload, max_retries in ((16, 5, 2), (100, 128, 0), (1024, 255, 10)):
        b = bench(n_streams, cap)
        rings, words, files = ref.random_case(rng, n_streams, cap, max_payload, max_retries)
        proc, tx = planted(b, rings, words, files, max_payload, max_retries)
        want = check_poll(b, proc, tx, rings, words, files, max_payload, max_retries)
        seen |= {(int(e["status"]), int(e["control"])) for e in want[1]}
        # a second poll: the streams that transmitted are mid-modulation now and keep every word, the others see an empty reply
        check_poll(b, proc, tx, want[2], want[3], files, max_payload, max_retries, premod=want[4])
        tx.close()
        b.close()
        b.made = []
    if n_streams >= 63:
        assert {st for st, _ in seen} == {ref.PROGRESS, ref.DONE, ref.MAX_RETRIES} and {c for _, c in seen} >= {ref.ACK, ref.NAK, ref.EOT}


@pytest.mark.parametrize("cap", [16, 100])
def test_66000_streams_take_a_second_totals_pass(bench, cap):
    n_streams, tile, max_payload, max_retries = 66000, 1100, 16, 3
    rng = np.random.default_rng(66 + cap)
    small, w, f = ref.random_case(rng, tile, cap, max_payload, max_retries, idle=0.6)
    k = n_streams // tile
    rings = drain_ref.Rings(np.tile(small.r, k), np.tile(small.n, k), np.tile(small.ring, (k, 1)))
    words, files = {key: np.tile(v, k) for key, v in w.items()}, f * k
    for s in (0, n_streams - 1):   # the first lane and the last one of the partial workgroup answer a NAK with a packet
        words["state"][s], words["fragment_index"][s], files[s] = ref.WAIT_NAK, 0, b"edge" * 5
        rings.n[s], rings.ring[s, rings.r[s]] = 1, ref.NAK
    b = bench(n_streams, cap)
    proc, tx = planted(b, rings, words, files, max_payload, max_retries)
    want = check_poll(b, proc, tx, rings, words, files, max_payload, max_retries)
    assert len(want[0]) > 5000 and want[0][0] == 0 and want[0][-1] == n_streams - 1 and len(want[4]) > 2000
    tx.close()


def test_mask_abort_and_pending_modulations(bench):
    """an unselected stream and a stream mid-modulation keep every word; an abort ends the transfer and leaves the ring and the
    modulation alone -- also where the stream is mid-modulation, and before the pending rule"""
    n_streams, cap, max_payload, max_retries = 300, 100, 16, 2
    rng = np.random.default_rng(41)
    b = bench(n_streams, cap)
    rings, words, files = ref.random_case(rng, n_streams, cap, max_payload, max_retries)
    mask, abort, premod = rng.random(n_streams) < 0.6, rng.random(n_streams) < 0.25, rng.random(n_streams) < 0.3
    rows = premod_rows(premod)
    proc, tx = planted(b, rings, words, files, max_payload, max_retries, rows)
    want = check_poll(b, proc, tx, rings, words, files, max_payload, max_retries, mask, abort, rows)
    live = words["state"] != ref.IDLE
    aborted = mask & abort & live
    kept = (~mask | (premod & ~abort)) & live
    assert aborted.sum() > 20 and kept.sum() > 50 and (aborted & premod).sum() > 3
    ev = {int(s): e for s, e in zip(want[0], want[1])}
    assert all(ev[s]["status"] == ref.ABORTED and ev[s]["state_after"] == ref.IDLE and ev[s]["sent_len"] == 0 for s in np.flatnonzero(aborted))
    assert np.array_equal(want[2].n[aborted | kept], rings.n[aborted | kept]) and not set(np.flatnonzero(kept)) & set(ev)
    assert all(np.array_equal(want[3][k][kept], words[k][kept]) for k in ref.WORDS)
    check_poll(b, proc, tx, want[2], want[3], files, max_payload, max_retries, premod={**rows, **want[4]})
    tx.close()


def test_overflow_is_atomic_and_the_count_is_reported(bench):
    n_streams, cap, max_payload, max_retries = 600, 100, 16, 2
    rng = np.random.default_rng(9)
    b = bench(n_streams, cap)
    rings, words, files = ref.random_case(rng, n_streams, cap, max_payload, max_retries)
    proc, tx = planted(b, rings, words, files, max_payload, max_retries)
    ws, we, after, wwords, sent = ref.step_ref(rings, words, files, max_payload, max_retries)
    assert len(ws) > 100 and len(sent) > 50 and after.n.sum() < rings.n.sum()
    before = proc.snapshot().processor
    L = tx._L
    streams, events = np.zeros(len(ws), np.uint32), np.zeros(len(ws), ref.EVENT_DTYPE)
    ne = C.c_uint32(0)

    def call(cap_streams, lists=True):
        ne.value = 0xFFFFFFFF
        p = (lambda a: a.ctypes.data) if lists else (lambda a: None)
        return L.fskhip_xmodem_tx_poll_host(tx._h, None, None, p(streams), p(events), cap_streams, C.byref(ne))
    for cap_streams, lists in ((len(ws) - 1, True), (1, True), (0, False)):
        assert call(cap_streams, lists) == E_OVERFLOW
        assert "nothing was polled" in L.fskhip_last_error().decode()
        assert ne.value == len(ws)
        assert proc.snapshot().processor == before and same_words(tx.state(), words)   # no ring word, no sender word, no modulation
    assert call(len(ws)) == 0 and ne.value == len(ws)
    assert np.array_equal(streams, ws) and events.tolist() == we.tolist()
    assert proc.snapshot().processor == twin_image(b, after, sent) and same_words(tx.state(), wwords)
    # send() on a stream that is still sending is the reference's ensureIdle; nothing starts
    busy = int(np.flatnonzero(wwords["state"] == ref.WAIT_ACK)[0])
    with pytest.raises(RuntimeError, match=r"^Transport busy: sendData cannot start while in SENDING_WAIT_ACK state \(stream %d\)$" % busy):
        tx.send([b"x"] * n_streams, mask=np.arange(n_streams) >= busy)
    assert same_words(tx.state(), wwords)
    # state_set validates as a whole and names the first bad stream
    bad = wwords["sequence"].copy()
    bad[[17, 40]] = [0, 256]
    assert L.fskhip_xmodem_tx_state_set(tx._h, None, bad.ctypes.data, None, None, None, None) == E_INVALID
    assert L.fskhip_last_error().decode() == "fskhip_xmodem_tx_state_set: sequence[17] = 0 is not a sequence number (1-255)"
    assert same_words(tx.state(), wwords)
    tx.reset(busy)   # reset(): IDLE, sequence 1, index 0, the counters too; then a new file may be sent
    st = tx.state()
    assert [int(st[k][busy]) for k in ref.WORDS] == [ref.IDLE, 1, 0, 0, 0, 0]
    others = np.arange(n_streams) != busy
    assert all(np.array_equal(st[k][others], wwords[k][others]) for k in ref.WORDS)
    tx.send([b"again"] * n_streams, mask=~others)
    assert tx.state()["state"][busy] == ref.WAIT_NAK
    tx.reset()
    assert same_words(tx.state(), ref.fresh_words(n_streams))
    tx.close()


def test_device_form(bench):
    n_streams, cap, max_payload, max_retries = 700, 1024, 128, 3
    rng = np.random.default_rng(11)
    b = bench(n_streams, cap)
    rings, words, files = ref.random_case(rng, n_streams, cap, max_payload, max_retries)
    mask, abort = (rng.random(n_streams) < 0.7).astype(np.uint8), (rng.random(n_streams) < 0.1).astype(np.uint8)
    ws, we, after, wwords, sent = ref.step_ref(rings, words, files, max_payload, max_retries, mask=mask, abort=abort)
    dev, tx = planted(b, rings, words, files, max_payload, max_retries)
    L, eh, lib = tx._L, dev.engine._h, b.wm._lib
    hip, stream = _hip_runtime(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0 and stream.value   # a stream of the caller's own, not the null stream
    sizes = {"mask": n_streams, "abort": n_streams, "streams": 4 * len(ws), "events": 32 * len(ws), "totals": 12}
    d = {}
    for k, nbytes in sizes.items():
        p = C.c_void_p()
        lib.check(L.fskhip_device_malloc(eh, nbytes, C.byref(p)))
        d[k] = p
    try:
        lib.check(L.fskhip_memcpy_h2d(eh, d["mask"], mask.ctypes.data, n_streams))
        lib.check(L.fskhip_memcpy_h2d(eh, d["abort"], abort.ctypes.data, n_streams))
        before = dev.snapshot().processor

        def run(cap_streams):
            lib.check(L.fskhip_xmodem_tx_poll_device(tx._h, d["mask"], d["abort"], d["streams"], d["events"], cap_streams, d["totals"], stream))
            assert hip.hipStreamSynchronize(stream) == 0
            totals = np.zeros(3, np.uint32)
            lib.check(L.fskhip_memcpy_d2h(eh, totals.ctypes.data, d["totals"], 12))
            return list(totals)
        assert run(len(ws) - 1) == [len(ws), 0, 0]
        assert dev.snapshot().processor == before and same_words(tx.state(), words)
        assert run(len(ws)) == [len(ws), 0, 1]
        gs, ge = np.zeros(len(ws), np.uint32), np.zeros(len(ws), ref.EVENT_DTYPE)
        for arr, k in ((gs, "streams"), (ge, "events")):
            lib.check(L.fskhip_memcpy_d2h(eh, arr.ctypes.data, d[k], arr.nbytes))
        assert np.array_equal(gs, ws) and ge.tolist() == we.tolist()
        assert dev.snapshot().processor == twin_image(b, after, sent) and same_words(tx.state(), wwords)
    finally:
        for p in d.values():
            L.fskhip_device_free(eh, p)
        hip.hipStreamDestroy(stream)
        tx.close()


def test_files_are_replaced_and_the_store_is_compacted(bench):
    """files sent in several calls, one replaced by longer ones until the packed store has to grow and move the files that stay, one
    dropped: every stream then answers a NAK with fragment 0 of ITS current file"""
    n_streams, cap, max_payload = 130, 16, 200
    rng = np.random.default_rng(77)
    b = bench(n_streams, cap)
    rings = drain_ref.Rings(np.zeros(n_streams, int), np.ones(n_streams, int), np.full((n_streams, cap), ref.NAK, np.uint8))
    proc = b.clone(rings)
    tx = b.wm.XModemSenderBatch(proc, max_payload, 10)
    files = [bytes(rng.integers(0, 256, int(rng.integers(0, 120)), dtype=np.uint8)) for _ in range(n_streams)]
    tx.send(files)
    only5 = np.arange(n_streams) == 5
    for grow in (3000, 40000):   # the second one does not fit behind what the store holds
        tx.reset(5)
        files[5] = bytes(rng.integers(0, 256, grow, dtype=np.uint8))
        tx.send([files[s] if s == 5 else None for s in range(n_streams)], mask=only5)
    tx.reset(7)
    files[7] = None
    words = ref.sent_words(ref.fresh_words(n_streams), mask=np.arange(n_streams) != 7)
    assert same_words(tx.state(), words)
    want = check_poll(b, proc, tx, rings, words, files, max_payload, 10)
    assert len(want[4]) == n_streams - 1 and want[4][5][4:-2] == files[5][:max_payload]
    tx.close()


def test_the_signal_is_that_of_the_same_bytes_through_modulate():
    """after a poll that transmits, process() output is bit for bit that of a twin processor given the same packet bytes through
    fskhip_processor_modulate_host: 65 streams, two quantum sizes"""
    import webaudio_modem_amd as wm
    S, max_payload = 65, 32
    rng = np.random.default_rng(65)
    files = [bytes(rng.integers(0, 256, (7 * s) % 90, dtype=np.uint8)) for s in range(S)]
    words = ref.sent_words(ref.fresh_words(S))
    last = np.arange(S) % 5 == 4      # a fifth of the streams are on their last fragment: the ACK brings the EOT out
    for s in np.flatnonzero(last):
        words["state"][s], words["fragment_index"][s], words["sequence"][s] = ref.WAIT_ACK, len(ref.fragments(files[s], max_payload)) - 1, 9
    reply = np.where(last, ref.ACK, ref.NAK)
    rings = drain_ref.Rings(np.full(S, 1020), np.full(S, 8), np.zeros((S, 1024), np.uint8))
    rings.ring[:, [1020, 1021, 1022, 1023, 0, 1, 2]] = 0x55
    rings.ring[:, 3] = reply          # the control byte behind noise, the span wrapping the ring's end
    want = ref.step_ref(rings, words, files, max_payload, 10)
    assert len(want[4]) == S and sum(len(p) == 1 for p in want[4].values()) == last.sum()
    out = {}
    for quantum in (128, 1000):
        got = []
        for use_sender in (True, False):
            eng = wm.FSKEngine(S, {}, precision=wm.PRECISION_F32)
            proc = wm.FSKProcessorBatch(eng, rx_capacity=1024)
            if use_sender:
                fresh = proc.snapshot()
                proc.close()
                proc = wm.FSKProcessorBatch.from_snapshot(wm.ProcessorBatchSnapshot(engine=fresh.engine, processor=rings.image(fresh=fresh.processor)))
                eng.close()
                eng = proc.engine
                tx = wm.XModemSenderBatch(proc, max_payload, 10)
                tx.send(files)
                tx.set_state(**words)
                streams, events = tx.poll()
                assert np.array_equal(streams, want[0]) and events.tolist() == want[1].tolist()
                tx.close()
            else:
                proc.modulate([want[4][s] for s in range(S)])
            n = max(len(p) for p in want[4].values()) * 11 * 40 + 48000 // 10   # past the end of the longest frame
            got.append(np.concatenate([proc.process(None, quantum) for _ in range((n + quantum - 1) // quantum)], axis=1))
            assert not proc.tx_state()["pendingModulation"].any()
            proc.close()
            eng.close()
        assert got[0].shape == got[1].shape and got[0].tobytes() == got[1].tobytes() and np.abs(got[0]).max() > 0.1
        out[quantum] = got[0]
    n = min(out[128].shape[1], out[1000].shape[1])
    assert out[128][:, :n].tobytes() == out[1000][:, :n].tobytes()


def test_closed_loop_with_the_resident_receiver():
    """the sender on processor A, XModemReceiverBatch on processor B, A's output samples into B and B's into A, quantum by quantum;
    the host sends the control byte each receiver record asks for.  Every file arrives byte-identical, every sender ends DONE, and
    the counters are those of step_ref fed one control byte per reply.  One stream has one packet's samples zeroed: its receiver
    hears nothing, the host's timer answers with a NAK, the sender retransmits."""
    import webaudio_modem_amd as wm
    from oracle import next_oracle as no
    S, max_payload, Q, lost = 65, 16, 512, 33
    cfg = dict(baudRate=4800, markFrequency=9600, spaceFrequency=14400)
    rng = np.random.default_rng(0xC105ED)
    files = [bytes(rng.integers(0, 256, (300 * s) // (S - 1), dtype=np.uint8)) for s in range(S)]
    assert len(files[0]) == 0 and len(files[-1]) == 300 and len(files[lost]) > 2 * max_payload
    eng_a, eng_b = (wm.FSKEngine(S, cfg, precision=wm.PRECISION_F32) for _ in range(2))
    A, B = (wm.FSKProcessorBatch(e, rx_capacity=1024, clear_rx_on_tx_complete=True) for e in (eng_a, eng_b))
    tx, rx = wm.XModemSenderBatch(A, max_payload), wm.XModemReceiverBatch(B)
    tx.send(files)
    B.modulate([bytes([ref.NAK])] * S)          # sendInitialNAK
    got, done, ended = [b""] * S, np.zeros(S, bool), {}
    owed = [[] for _ in range(S)]               # control bytes B's host still has to send, oldest first
    zeroing, zeroed, nak_due = False, False, False
    a_out, b_out = np.zeros((S, Q), np.float32), np.zeros((S, Q), np.float32)
    for quantum in range(4000):
        a_next, b_next = A.process(b_out, Q), B.process(a_out, Q)
        if zeroing:
            a_next[lost] = 0
            if not A.tx_state()["pendingModulation"][lost]:   # the packet has gone out unheard: the receiver's timer fires
                zeroing, nak_due = False, True
        a_out, b_out = a_next, b_next
        if quantum % 4 == 3:                    # (both hosts act every fourth quantum: frames keep their distance)
            for s, ev in tx.poll_active().items():
                if ev["status"] != ref.PROGRESS:
                    ended[s] = ev["status"]
                if s == lost and not zeroed and ev["sent_len"] > 1 and ev["fragment_index"] == 1:
                    zeroing = zeroed = True
            for s, (res, data) in rx.poll_active(mask=~done).items():
                got[s] += data
                owed[s] += [ref.ACK] * (res["packets"] + res["dropped"]) if res["status"] not in (no.XM_INVALID_SEQUENCE, no.XM_INVALID_CRC, no.XM_UNEXPECTED_SEQUENCE) \
                    else [ref.ACK] * max(res["packets"] + res["dropped"] - 1, 0) + [ref.NAK]
                if res["status"] == no.XM_EOT:
                    owed[s].append(ref.ACK)
                    done[s] = True
            if nak_due:
                owed[lost].append(ref.NAK)
                nak_due = False
            free = ~B.tx_state()["pendingModulation"]
            go = np.array([bool(owed[s]) and free[s] for s in range(S)])
            if go.any():
                B.modulate([bytes([owed[s].pop(0)]) if go[s] else b"" for s in range(S)], mask=go)
        if len(ended) == S:
            break
    assert len(ended) == S and set(ended.values()) == {ref.DONE}, (len(ended), quantum)
    assert got == files and zeroed
    # the counters: step_ref fed one control byte per reply -- NAK, an ACK per fragment (one more NAK for the lost packet), the final ACK
    st = tx.state()
    for s in range(S):
        n_frag = len(ref.fragments(files[s], max_payload))
        replies = [ref.NAK] + [ref.ACK] * n_frag + [ref.ACK]
        if s == lost:
            replies.insert(2, ref.NAK)
        words = ref.sent_words(ref.fresh_words(1))
        for c in replies:
            ring = drain_ref.Rings([0], [1], np.full((1, 16), c, np.uint8))
            words = ref.step_ref(ring, words, [files[s]], max_payload, 10)[3]
        assert all(int(st[k][s]) == int(words[k][0]) for k in ref.WORDS), s
        assert int(st["packets_sent"][s]) == n_frag + 1 + (s == lost) and int(st["retransmitted"][s]) == 2 * (s == lost)
    rs = rx.state()
    assert not rs["dropped"].any() and all(int(rs["packets"][s]) == len(ref.fragments(files[s], max_payload)) for s in range(S))
    tx.close()
    rx.close()
    for x in (A, B, eng_a, eng_b):
        x.close()
