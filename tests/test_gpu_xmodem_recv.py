"""The resident XModem file receiver on the GPU (include/fskhip_next.h: fskhip_xmodem_recv_*; XModemFileReceiverBatch).  Ring states
are planted as tests/test_gpu_xmodem_tx.py plants them -- the processor image of a fresh batch rewritten in numpy and restored --,
receiver words and files go in through set_files() + set_state(), pending modulations through modulate(); one poll is then compared
with step_ref (tests/xmodem_recv_ref.py, pinned to the real XModemTransport by the golden set): the lists, the events, every
receiver word, every file byte, and the whole processor image -- every ring word, tx_pending / tx_len / tx_n_payload and the payload
bytes -- against a twin processor that was given step_ref's rings and step_ref's control bytes through
fskhip_processor_modulate_host.  All comparisons are exact."""
import ctypes as C

import numpy as np
import pytest

import drain_ref
import xmodem_recv_ref as ref
import xmodem_tx_ref as tx_ref
from oracle import next_oracle as no
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


def close_clones(b):
    """closes the processors cloned from a Bench so far (and their engines); the Bench itself stays usable"""
    made, b.made = b.made, []
    for p in made:
        p.close()
        p.engine.close()


def premod_rows(rng_mask):
    """{stream: the payload of a modulation that is pending before the poll} for the streams of a bool array"""
    return {int(s): bytes([0x40 + s % 50]) * (1 + s % 7) for s in np.flatnonzero(rng_mask)}


def modulate_rows(proc, rows):
    if rows:
        proc.modulate([rows.get(s, b"") for s in range(proc.n_streams)], mask=[s in rows for s in range(proc.n_streams)])


def planted(b, rings, words, files, file_capacity, max_retries, premod=None):
    """a clone of the batch with these rings (and the pending modulations premod: {stream: payload}) and a receiver over it with
    these words and files"""
    proc = b.clone(rings)
    rx = b.wm.XModemFileReceiverBatch(proc, file_capacity, max_retries)
    rx.set_files(files)
    rx.set_state(**words)
    modulate_rows(proc, premod)
    return proc, rx


def twin_image(b, rings_after, sent, premod=None):
    """the image of a processor that holds step_ref's rings and was given step_ref's control bytes through modulate()"""
    twin = b.clone(rings_after)
    modulate_rows(twin, premod)
    modulate_rows(twin, sent)
    return twin.snapshot().processor


def same_words(got, want):
    return all(np.array_equal(got[k], want[k]) for k in ref.WORDS)


def check_poll(b, proc, rx, rings, words, files, file_capacity, max_retries, mask=None, timeout=None, abort=None, premod=None):
    pending = None if premod is None else np.array([s in premod for s in range(b.n_streams)])
    want = ref.step_ref(rings, words, files, file_capacity, max_retries, mask=mask, timeout=timeout, abort=abort, pending=pending)
    streams, events = rx.poll(mask, timeout, abort)
    assert streams.dtype == np.uint32 and events.dtype == ref.EVENT_DTYPE
    assert np.array_equal(streams, want[0]) and events.tolist() == want[1].tolist()
    assert same_words(rx.state(), want[3])
    assert rx.files() == want[4]
    assert proc.snapshot().processor == twin_image(b, want[2], want[5], premod)
    return want


@pytest.mark.parametrize("n_streams", [1, 63, 65, 257])
def test_lists_events_rings_words_files_and_modulations_match_step_ref(bench, n_streams):
    rng = np.random.default_rng(0x4EC0 + n_streams)
    seen = set()
    for cap, max_payload, max_retries, file_capacity in ((16, 5, 2, 12), (100, 40, 0, 100), (1024, 255, 10, 600)):
        b = bench(n_streams, cap)
        rings, words, files = ref.random_case(rng, n_streams, cap, max_payload, max_retries, file_capacity)
        timeout, abort = rng.random(n_streams) < 0.3, rng.random(n_streams) < 0.08
        proc, rx = planted(b, rings, words, files, file_capacity, max_retries)
        want = check_poll(b, proc, rx, rings, words, files, file_capacity, max_retries, timeout=timeout, abort=abort)
        seen |= {(int(e["status"]), int(e["step"])) for e in want[1]}
        # a second poll straight after: the streams that transmitted are mid-modulation now and keep every word
        again = check_poll(b, proc, rx, want[2], want[3], want[4], file_capacity, max_retries, premod=want[5])
        assert not set(again[0]) & set(want[5])
        rx.close()
        close_clones(b)
    if n_streams >= 63:
        assert {st for st, _ in seen} == {ref.PROGRESS, ref.DONE, ref.MAX_RETRIES, ref.ABORTED, ref.FILE_FULL}
        assert {k for _, k in seen} >= set(ref.ERRORS)


@pytest.mark.parametrize("cap", [16, 100])
def test_66000_streams_take_a_second_totals_pass(bench, cap):
    n_streams, tile, max_payload, max_retries, file_capacity = 66000, 1100, 5, 3, 24
    rng = np.random.default_rng(66 + cap)
    small, w, f = ref.random_case(rng, tile, cap, max_payload, max_retries, file_capacity, idle=0.6)
    k = n_streams // tile
    rings = drain_ref.Rings(np.tile(small.r, k), np.tile(small.n, k), np.tile(small.ring, (k, 1)))
    words, files = {key: np.tile(v, k) for key, v in w.items()}, f * k
    for s in (0, n_streams - 1):   # the first lane and the last one of the partial workgroup accept a packet
        words["state"][s], words["expected"][s], words["file_len"][s], files[s] = ref.WAIT_BLOCK, 7, 3, b"abc"
        p = ref.packet(7, b"edge!")
        rings.r[s], rings.n[s] = cap - 4, len(p)
        rings.ring[s, (cap - 4 + np.arange(len(p))) % cap] = np.frombuffer(p, np.uint8)
    b = bench(n_streams, cap)
    proc, rx = planted(b, rings, words, files, file_capacity, max_retries)
    want = check_poll(b, proc, rx, rings, words, files, file_capacity, max_retries)
    assert len(want[0]) > 5000 and want[0][0] == 0 and want[0][-1] == n_streams - 1
    assert want[4][0] == want[4][-1] == b"abcedge!" and want[1][0]["accepted_len"] == want[1][-1]["accepted_len"] == 5
    rx.close()


def test_mask_abort_timeout_and_pending_modulations(bench):
    """precedence is rules 1-3: abort before pending before the walk; a stream mid-modulation and an unselected stream keep every
    word, timeout flag or not; a timeout on a stream with a complete packet in its ring is ignored"""
    n_streams, cap, max_payload, max_retries, file_capacity = 300, 100, 16, 2, 64
    rng = np.random.default_rng(41)
    b = bench(n_streams, cap)
    rings, words, files = ref.random_case(rng, n_streams, cap, max_payload, max_retries, file_capacity)
    mask, abort, premod = rng.random(n_streams) < 0.6, rng.random(n_streams) < 0.25, rng.random(n_streams) < 0.3
    timeout = rng.random(n_streams) < 0.5
    for s in (3, 4):   # a complete packet, with and without the timeout flag: the same event
        words["state"][s], words["expected"][s], words["file_len"][s], words["retries"][s], files[s] = ref.WAIT_BLOCK, 9, 0, 1, b""
        p = ref.packet(9, b"whole")
        rings.r[s], rings.n[s] = 95, len(p)
        rings.ring[s, (95 + np.arange(len(p))) % cap] = np.frombuffer(p, np.uint8)
        mask[s], abort[s], premod[s], timeout[s] = True, False, False, s == 3
    rows = premod_rows(premod)
    proc, rx = planted(b, rings, words, files, file_capacity, max_retries, rows)
    want = check_poll(b, proc, rx, rings, words, files, file_capacity, max_retries, mask, timeout, abort, rows)
    live = words["state"] != ref.IDLE
    aborted = mask & abort & live
    kept = (~mask | (premod & ~abort)) & live
    assert aborted.sum() > 20 and kept.sum() > 50 and (aborted & premod).sum() > 3 and (kept & timeout).sum() > 10
    ev = {int(s): e for s, e in zip(want[0], want[1])}
    assert all(ev[s]["status"] == ref.ABORTED and ev[s]["state_after"] == ref.IDLE and ev[s]["control"] == -1 for s in np.flatnonzero(aborted))
    assert np.array_equal(want[2].n[aborted | kept], rings.n[aborted | kept]) and not set(np.flatnonzero(kept)) & set(ev)
    assert all(np.array_equal(want[3][k][kept], words[k][kept]) for k in ref.WORDS)
    assert ev[3].tolist() == ev[4].tolist() and ev[3]["control"] == ref.ACK and ev[3]["retries"] == 0 and want[4][3] == b"whole"
    timed = [s for s in ev if timeout[s] and ev[s]["step"] == no.XM_NEED_MORE and ev[s]["control"] == ref.NAK]
    assert len(timed) > 5 and all(want[2].n[s] == 0 for s in timed)
    check_poll(b, proc, rx, want[2], want[3], want[4], file_capacity, max_retries, premod={**rows, **want[5]})
    rx.close()


def test_overflow_is_atomic_and_the_count_is_reported(bench):
    n_streams, cap, max_payload, max_retries, file_capacity = 600, 100, 16, 2, 64
    rng = np.random.default_rng(9)
    b = bench(n_streams, cap)
    rings, words, files = ref.random_case(rng, n_streams, cap, max_payload, max_retries, file_capacity)
    proc, rx = planted(b, rings, words, files, file_capacity, max_retries)
    ws, we, after, wwords, wfiles, sent = ref.step_ref(rings, words, files, file_capacity, max_retries)
    assert len(ws) > 100 and len(sent) > 50 and after.n.sum() < rings.n.sum() and wfiles != files
    before = proc.snapshot().processor
    L = rx._L
    streams, events = np.zeros(len(ws), np.uint32), np.zeros(len(ws), ref.EVENT_DTYPE)
    ne = C.c_uint32(0)

    def call(cap_streams, lists=True):
        ne.value = 0xFFFFFFFF
        p = (lambda a: a.ctypes.data) if lists else (lambda a: None)
        return L.fskhip_xmodem_recv_poll_host(rx._h, None, None, None, p(streams), p(events), cap_streams, C.byref(ne))
    for cap_streams, lists in ((len(ws) - 1, True), (1, True), (0, False)):
        assert call(cap_streams, lists) == E_OVERFLOW
        assert "nothing was polled" in L.fskhip_last_error().decode()
        assert ne.value == len(ws)
        # no ring word, no receiver word, no file byte, no modulation
        assert proc.snapshot().processor == before and same_words(rx.state(), words) and rx.files() == files
    assert call(len(ws)) == 0 and ne.value == len(ws)
    assert np.array_equal(streams, ws) and events.tolist() == we.tolist()
    assert proc.snapshot().processor == twin_image(b, after, sent) and same_words(rx.state(), wwords) and rx.files() == wfiles
    # start() on a stream that is still receiving is the reference's ensureIdle; nothing starts
    busy = int(np.flatnonzero(wwords["state"] == ref.SEND_ACK)[0])
    with pytest.raises(RuntimeError, match=r"^Transport busy: receiveData cannot start while in RECEIVING_SEND_ACK state \(stream %d\)$" % busy):
        rx.start(mask=np.arange(n_streams) >= busy)
    assert same_words(rx.state(), wwords)
    # state_set validates as a whole and names the first bad stream
    bad = wwords["expected"].copy()
    bad[[17, 40]] = [0, 256]
    assert L.fskhip_xmodem_recv_state_set(rx._h, None, bad.ctypes.data, None, None, None, None, None) == E_INVALID
    assert L.fskhip_last_error().decode() == "fskhip_xmodem_recv_state_set: expected[17] = 0 is not a sequence number (1-255)"
    assert same_words(rx.state(), wwords)
    rx.reset(busy)   # reset(): IDLE, expected 1, an empty file, the counters too
    st = rx.state()
    assert [int(st[k][busy]) for k in ref.WORDS] == [ref.IDLE, 1, 0, 0, 0, 0, 0] and rx.files([busy]) == [b""]
    others = np.arange(n_streams) != busy
    assert all(np.array_equal(st[k][others], wwords[k][others]) for k in ref.WORDS)
    rx.reset()
    assert same_words(rx.state(), ref.fresh_words(n_streams))
    rx.close()


def test_start_sends_the_initial_nak_and_refuses_a_busy_modulator(bench):
    n_streams, cap = 70, 100
    b = bench(n_streams, cap)
    rings = drain_ref.random_rings(np.random.default_rng(5), n_streams, cap, "random30")
    proc = b.clone(rings)
    rx = b.wm.XModemFileReceiverBatch(proc, 32, 3)
    modulate_rows(proc, {68: b"busy"})
    before = proc.snapshot().processor
    with pytest.raises(RuntimeError, match=r"^Modulation already in progress \(stream 68\)$"):
        rx.start()
    assert same_words(rx.state(), ref.fresh_words(n_streams)) and proc.snapshot().processor == before
    mask = np.arange(n_streams) % 3 != 2
    mask[68] = False
    rx.start(mask)
    assert same_words(rx.state(), ref.started_words(ref.fresh_words(n_streams), mask))
    # the ring is NOT cleared; the NAK is the one modulate() would have started
    assert proc.snapshot().processor == twin_image(b, rings, {int(s): bytes([ref.NAK]) for s in np.flatnonzero(mask)}, {68: b"busy"})
    rx.close()


def test_files_round_trip_and_a_small_cap_copies_nothing(bench):
    n_streams, cap, file_capacity = 130, 16, 300
    rng = np.random.default_rng(77)
    b = bench(n_streams, cap)
    proc = b.clone(drain_ref.Rings(np.zeros(n_streams, int), np.zeros(n_streams, int), np.zeros((n_streams, cap), np.uint8)))
    rx = b.wm.XModemFileReceiverBatch(proc, file_capacity, 3)
    files = [bytes(rng.integers(0, 256, int(rng.choice([0, 1, 63, 64, 65, 300, int(rng.integers(0, 301))])), dtype=np.uint8)) for _ in range(n_streams)]
    rx.set_files(files)
    assert rx.files() == files and np.array_equal(rx.state()["file_len"], [len(f) for f in files])
    pick = [129, 0, 64, 5]
    assert rx.files(pick) == [files[s] for s in pick] and rx.files([]) == []
    only = np.arange(n_streams) % 7 == 1
    for s in np.flatnonzero(only):
        files[s] = bytes(rng.integers(0, 256, 17, dtype=np.uint8))
    rx.set_files([files[s] if only[s] else None for s in range(n_streams)], mask=only)
    assert rx.files() == files
    L, total = rx._L, sum(len(f) for f in files)
    sel, offsets, nb = np.arange(n_streams, dtype=np.uint32), np.zeros(n_streams + 1, np.uint64), C.c_uint64(0)
    data = np.full(total, 0xEE, np.uint8)
    assert L.fskhip_xmodem_recv_files_host(rx._h, sel.ctypes.data, n_streams, offsets.ctypes.data, data.ctypes.data, total - 1, C.byref(nb)) == E_OVERFLOW
    assert nb.value == total and (data == 0xEE).all()
    assert L.fskhip_xmodem_recv_files_host(rx._h, sel.ctypes.data, n_streams, offsets.ctypes.data, None, 0, C.byref(nb)) == E_OVERFLOW and nb.value == total
    too_long = np.array([0, file_capacity + 1], np.uint64)
    one = np.array([3], np.uint32)
    assert L.fskhip_xmodem_recv_files_set_host(rx._h, one.ctypes.data, 1, too_long.ctypes.data, data.ctypes.data) == E_INVALID
    assert rx.files() == files
    rx.close()


def test_device_form(bench):
    n_streams, cap, max_payload, max_retries, file_capacity = 700, 1024, 128, 3, 400
    rng = np.random.default_rng(11)
    b = bench(n_streams, cap)
    rings, words, files = ref.random_case(rng, n_streams, cap, max_payload, max_retries, file_capacity)
    mask, timeout, abort = ((rng.random(n_streams) < p).astype(np.uint8) for p in (0.7, 0.3, 0.1))
    ws, we, after, wwords, wfiles, sent = ref.step_ref(rings, words, files, file_capacity, max_retries, mask=mask, timeout=timeout, abort=abort)
    dev, rx = planted(b, rings, words, files, file_capacity, max_retries)
    L, eh, lib = rx._L, dev.engine._h, b.wm._lib
    hip, stream = _hip_runtime(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0 and stream.value   # a stream of the caller's own, not the null stream
    sizes = {"mask": n_streams, "timeout": n_streams, "abort": n_streams, "streams": 4 * len(ws), "events": 48 * len(ws), "totals": 12}
    d = {}
    for k, nbytes in sizes.items():
        p = C.c_void_p()
        lib.check(L.fskhip_device_malloc(eh, nbytes, C.byref(p)))
        d[k] = p
    try:
        for k, a in (("mask", mask), ("timeout", timeout), ("abort", abort)):
            lib.check(L.fskhip_memcpy_h2d(eh, d[k], a.ctypes.data, n_streams))
        before = dev.snapshot().processor

        def run(cap_streams):
            lib.check(L.fskhip_xmodem_recv_poll_device(rx._h, d["mask"], d["timeout"], d["abort"], d["streams"], d["events"], cap_streams, d["totals"], stream))
            assert hip.hipStreamSynchronize(stream) == 0
            totals = np.zeros(3, np.uint32)
            lib.check(L.fskhip_memcpy_d2h(eh, totals.ctypes.data, d["totals"], 12))
            return list(totals)
        assert run(len(ws) - 1) == [len(ws), 0, 0]
        assert dev.snapshot().processor == before and same_words(rx.state(), words) and rx.files() == files
        assert run(len(ws)) == [len(ws), 0, 1]
        gs, ge = np.zeros(len(ws), np.uint32), np.zeros(len(ws), ref.EVENT_DTYPE)
        for arr, k in ((gs, "streams"), (ge, "events")):
            lib.check(L.fskhip_memcpy_d2h(eh, arr.ctypes.data, d[k], arr.nbytes))
        assert np.array_equal(gs, ws) and ge.tolist() == we.tolist()
        assert dev.snapshot().processor == twin_image(b, after, sent) and same_words(rx.state(), wwords) and rx.files() == wfiles
    finally:
        for p in d.values():
            L.fskhip_device_free(eh, p)
        hip.hipStreamDestroy(stream)
        rx.close()


def finish_modulations(proc, quantum=512):
    """process() quanta until no one-byte modulation is pending"""
    for _ in range(64):
        if not proc.tx_state()["pendingModulation"].any():
            return
        proc.process(None, quantum)
    raise AssertionError("a one-byte modulation did not end")


def test_cut_invariance_without_errors():
    """one error-free byte stream per stream, duplicates and noise included, delivered in three different splittings; polls run to
    quiescence, the pending one-byte modulations finished by process() quanta: the transmission sequences, the files and the
    final words are identical"""
    import webaudio_modem_amd as wm
    S, cap, file_capacity = 65, 1024, 512
    rng = np.random.default_rng(0xC07)
    lines, files = [], []
    for s in range(S):
        line, data, seq = b"", b"", 1
        for k in range(int(rng.integers(0, 6)) if s else 0):
            p = bytes(rng.integers(0, 256, int(rng.integers(0, 40)), dtype=np.uint8))
            line += bytes(rng.choice(ref.NOISE_ARR, size=int(rng.integers(0, 3)))) + ref.packet(seq, p)
            if rng.random() < 0.3:
                line += ref.packet(seq, p)   # the sender did not hear the ACK
            data, seq = data + p, seq % 255 + 1
        lines.append(line + bytes([ref.EOT]) + b"\x99after")
        files.append(data)
    results = []
    for cuts in ("whole", "bytes37", "random"):
        eng = wm.FSKEngine(S, dict(baudRate=4800, markFrequency=9600, spaceFrequency=14400), precision=wm.PRECISION_F32)
        fresh_proc = wm.FSKProcessorBatch(eng, rx_capacity=cap)
        fresh = fresh_proc.snapshot()
        fresh_proc.close()
        eng.close()
        proc = wm.FSKProcessorBatch.from_snapshot(wm.ProcessorBatchSnapshot(engine=fresh.engine, processor=drain_ref.Rings(
            np.full(S, 1000), np.zeros(S, int), np.zeros((S, cap), np.uint8)).image(fresh=fresh.processor)), clear_rx_on_tx_complete=False)
        rx = wm.XModemFileReceiverBatch(proc, file_capacity, 10)
        rx.start()
        sent = [[ref.NAK] for _ in range(S)]
        finish_modulations(proc)
        at = np.zeros(S, int)
        crng = np.random.default_rng(3)
        while True:
            # deliver the next piece of every line: restore the processor with the bytes appended to its rings
            image = np.frombuffer(proc.snapshot().processor, np.uint8).copy()
            rec = int(image[12:16].view("<u4")[0])
            recs = image[drain_ref.HEADER_BYTES:].reshape(S, rec)
            w = recs[:, :16].copy().view("<u4")   # writeIndex, readIndex, _length
            more = False
            for s in range(S):
                left = len(lines[s]) - at[s]
                step = left if cuts == "whole" else min(left, 37) if cuts == "bytes37" else min(left, int(crng.integers(0, 60)))
                piece = np.frombuffer(lines[s][at[s]:at[s] + step], np.uint8)
                assert w[s, 2] + step <= cap
                recs[s, drain_ref.REC_FIXED + (int(w[s, 0]) + np.arange(step)) % cap] = piece
                w[s, 0], w[s, 2] = (w[s, 0] + step) % cap, w[s, 2] + step
                at[s] += step
                more |= at[s] < len(lines[s])
            recs[:, :16] = w.view(np.uint8)
            state = rx.state()
            held = rx.files()
            rx.close()
            engine = proc.engine
            proc.close()
            engine.close()
            proc = wm.FSKProcessorBatch.from_snapshot(wm.ProcessorBatchSnapshot(engine=fresh.engine, processor=drain_ref.seal(image).tobytes()),
                                                     clear_rx_on_tx_complete=False)
            rx = wm.XModemFileReceiverBatch(proc, file_capacity, 10)
            rx.set_files(held)
            rx.set_state(**state)
            while True:   # to quiescence
                evs = rx.poll_active()
                for s, e in evs.items():
                    assert e["control"] in (ref.ACK, -1) and e["status"] in (ref.PROGRESS, ref.DONE)
                    if e["control"] != -1:
                        sent[s].append(e["control"])
                if not evs:
                    break
                finish_modulations(proc)
            if not more:
                break
        results.append((sent, rx.files(), {k: v.tolist() for k, v in rx.state().items()}, proc.demodulate()))
        rx.close()
        engine = proc.engine
        proc.close()
        engine.close()
    assert results[0][1] == files and all(r[:3] == results[0][:3] for r in results[1:])
    assert all(x == ref.IDLE for x in results[0][2]["state"]) and results[0][2]["dropped"] != [0] * S
    assert results[0][3] == results[1][3] == results[2][3] == [b"\x99after"] * S   # what lies behind the EOT stays, in every splitting


@pytest.mark.parametrize("cap,r0", [(272, 259), (300, 0)])
def test_golden_replay_on_the_device(bench, cap, r0):
    """every recorded run of the real receiveData() through the device, each on one stream of its own: capacity 272 with readIndex
    259 takes the tile path with a wrap, capacity 300 the byte path.  The runs that share a maxRetries advance side by side, one
    reply each per round: the reply is planted behind what the stream's ring holds (a recorded timeout is the poll's timeout flag,
    the recorded external abort its abort flag), then polls run until nothing is listed, the one-byte modulations finished by
    process() quanta in between."""
    g = ref.golden_recv()
    for max_retries in sorted({c["maxRetries"] for c in g.cases}):
        cases = [c for c in g.cases if c["maxRetries"] == max_retries]
        S = len(cases)
        b = bench(S, cap)
        rings = drain_ref.Rings(np.full(S, r0), np.zeros(S, int), np.zeros((S, cap), np.uint8))
        words, files = ref.started_words(ref.fresh_words(S)), [b""] * S
        sent, status, taken, aborted = [[(0, bytes([ref.NAK]))] for _ in range(S)], [ref.PROGRESS] * S, [0] * S, [False] * S
        while True:
            timeout, abort, active = np.zeros(S, bool), np.zeros(S, bool), False
            for s, c in enumerate(cases):
                if status[s] != ref.PROGRESS:
                    continue
                if taken[s] < len(c["replies"]):
                    reply = c["replies"][taken[s]]
                    taken[s] += 1
                    active = True
                    if reply is None:
                        timeout[s] = True
                        continue
                    assert rings.n[s] + len(reply) <= cap
                    rings.ring[s, (rings.r[s] + rings.n[s] + np.arange(len(reply))) % cap] = np.frombuffer(reply, np.uint8)
                    rings.n[s] += len(reply)
                elif c["abort"] and not aborted[s]:
                    abort[s] = aborted[s] = active = True
            if not active:
                break
            proc = b.clone(rings, clear_rx_on_tx_complete=False)
            rx = b.wm.XModemFileReceiverBatch(proc, 4096, max_retries)
            rx.set_files(files)
            rx.set_state(**words)
            first = True
            while True:
                streams, events = rx.poll(None, timeout if first else None, abort if first else None)
                first = False
                for s, e in zip(streams, events):
                    status[s] = int(e["status"])
                    if e["control"] != -1:
                        sent[s].append((taken[s], bytes([int(e["control"])])))
                if not len(streams):
                    break
                finish_modulations(proc, 2048)
            words, files = rx.state(), rx.files()
            w = np.frombuffer(proc.snapshot().processor, np.uint8)[drain_ref.HEADER_BYTES:].reshape(S, -1)[:, :16].copy().view("<u4")
            rings = drain_ref.Rings(w[:, 1], w[:, 2], rings.ring)
            rx.close()
            close_clones(b)
        for s, c in enumerate(cases):
            st = {k: int(v[s]) for k, v in words.items()}
            assert sent[s] == c["sent"], c["name"]
            assert st["packets_received"] == c["statistics"]["packetsReceived"] and st["dropped"] == c["statistics"]["packetsDropped"], c["name"]
            assert st["packets_sent"] == len(c["sent"]) and st["expected"] == c["expectedSequence"] and st["state"] == ref.IDLE, c["name"]
            if c["result"] is not None:
                assert status[s] == ref.DONE and files[s] == c["result"], c["name"]
            else:
                assert status[s] == (ref.ABORTED if c["abort"] else ref.MAX_RETRIES), c["name"]


def test_end_to_end_with_no_host_bytes():
    """an XModemSenderBatch on processor A and an XModemFileReceiverBatch on processor B, cross-wired by process() quanta on device
    buffers -- A's output is B's input and B's output is A's input --, both polled every fourth quantum.  Files of 0, 1, 16, 17 and
    40 bytes at 1 200 baud with max_payload_size 16: every file arrives byte for byte, every sender and every receiver ends DONE,
    and the packet and control counters are those of the reference's protocol for 1, 1, 1, 2 and 3 fragments."""
    import webaudio_modem_amd as wm
    sizes, max_payload, Q = [0, 1, 16, 17, 40], 16, 2048
    S = len(sizes)
    rng = np.random.default_rng(0xE2E)
    files = [bytes(rng.integers(0, 256, n, dtype=np.uint8)) for n in sizes]
    eng_a, eng_b = (wm.FSKEngine(S, dict(baudRate=1200), precision=wm.PRECISION_F32) for _ in range(2))
    A, B = (wm.FSKProcessorBatch(e, rx_capacity=1024, clear_rx_on_tx_complete=True) for e in (eng_a, eng_b))
    tx, rx = wm.XModemSenderBatch(A, max_payload), wm.XModemFileReceiverBatch(B, 64)
    tx.send(files)
    rx.start()
    L, lib, zeros = wm._lib.lib(), wm._lib, np.zeros((S, Q), np.float32)
    bufs = []
    for _ in range(4):   # the sample buffers stay on the device: each side's output of one quantum is the other's input of the next
        p = C.c_void_p()
        lib.check(L.fskhip_device_malloc(eng_a._h, zeros.nbytes, C.byref(p)))
        lib.check(L.fskhip_memcpy_h2d(eng_a._h, p, zeros.ctypes.data, zeros.nbytes))
        bufs.append(p)
    a_out, a_next, b_out, b_next = bufs
    tx_end, rx_end = {}, {}
    for quantum in range(1200):
        A.process_device(b_out, Q, Q, a_next, Q, Q)
        B.process_device(a_out, Q, Q, b_next, Q, Q)
        a_out, a_next, b_out, b_next = a_next, a_out, b_next, b_out
        if quantum % 4 == 3:
            for s, ev in tx.poll_active().items():
                if ev["status"] != tx_ref.PROGRESS:
                    tx_end[s] = ev["status"]
            for s, ev in rx.poll_active().items():
                if ev["status"] != ref.PROGRESS:
                    rx_end[s] = ev["status"]
            if len(tx_end) == S and len(rx_end) == S:
                break
    assert tx_end == {s: tx_ref.DONE for s in range(S)} and rx_end == {s: ref.DONE for s in range(S)}, (tx_end, rx_end, quantum)
    assert rx.files() == files
    ts, rs = tx.state(), rx.state()
    n_frag = [len(tx_ref.fragments(f, max_payload)) for f in files]
    assert ts["packets_sent"].tolist() == [n + 1 for n in n_frag] and not ts["retransmitted"].any()        # the fragments and the EOT
    assert rs["packets_received"].tolist() == n_frag and not rs["dropped"].any() and not rs["retries"].any()
    assert rs["packets_sent"].tolist() == [n + 2 for n in n_frag]                                          # NAK, an ACK per fragment, the EOT's ACK
    assert rs["expected"].tolist() == [n % 255 + 1 for n in n_frag] and rs["file_len"].tolist() == sizes
    tx.close()
    rx.close()
    for p in bufs:
        L.fskhip_device_free(eng_a._h, p)
    for x in (A, B, eng_a, eng_b):
        x.close()
