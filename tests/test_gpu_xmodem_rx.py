"""The resident XModem receiver on the GPU (include/fskhip_next.h: fskhip_xmodem_rx_*; XModemReceiverBatch).  Ring states are set
directly, as tests/test_gpu_rx_drain_sparse.py sets them -- the processor image of a fresh batch rewritten in numpy and restored --
with traffic from tests/xmodem_rx_ref.py, and every list, payload byte, ring word and state word is compared with poll_ref, which
sits on the oracle's scan_burst and never calls the code under test.  All comparisons are exact.  The shapes are those where the
launches can go wrong: a partial wave, exactly one, one lane into the next, the same around a 256-stream workgroup, several
workgroups, and 66 000 streams (258 workgroup pairs: the totals kernel makes a second pass; a partial last workgroup); capacity 16
and 1 024 take the 16-byte tile path (one tile and sixteen), 100 and 1 the byte path."""
import ctypes as C

import numpy as np
import pytest

import drain_ref
import xmodem_rx_ref as ref
from oracle import next_oracle as no
from test_gpu_rx_drain_sparse import Bench, _hip_runtime

pytestmark = pytest.mark.gpu

E_INVALID, E_OVERFLOW = -1, -7


@pytest.fixture
def bench():
    made = []

    def make(n_streams, cap):
        made.append(Bench(n_streams, cap))
        return made[-1]
    yield make
    for b in made:
        b.close()


def receiver(b, rings, state=None):
    """a clone of the batch with these rings and a receiver over it in this state"""
    proc = b.clone(rings)
    rx = b.wm.XModemReceiverBatch(proc)
    if state is not None:
        rx.set_state(**state)
    return proc, rx


def same_state(got, want):
    return all(np.array_equal(got[k], want[k]) for k in ("expected", "packets", "dropped"))


def check_poll(b, proc, rx, rings, state, mask=None):
    want = ref.poll_ref(rings, state["expected"], mask, state["packets"], state["dropped"])
    streams, results, offsets, data = rx.poll(mask)
    assert streams.dtype == np.uint32 and offsets.dtype == np.uint32 and data.dtype == np.uint8 and results.dtype == ref.RESULT_DTYPE
    assert np.array_equal(streams, want[0]) and np.array_equal(offsets, want[2]) and np.array_equal(data, want[3])
    assert results.tolist() == want[1].tolist()
    assert proc.snapshot().processor == want[4].image(fresh=b.fresh.processor)   # every ring word (and live byte) of every stream
    assert same_state(rx.state(), want[5])
    return want


def zero_state(n_streams, expected):
    return {"expected": np.asarray(expected, np.uint32), "packets": np.zeros(n_streams, np.uint32), "dropped": np.zeros(n_streams, np.uint32)}


@pytest.mark.parametrize("n_streams", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_lists_payloads_rings_and_state_match_poll_ref(bench, n_streams):
    rng = np.random.default_rng(0xC0DE + n_streams)
    seen = set()
    for cap in (16, 100, 1024, 1):
        b = bench(n_streams, cap)
        state = zero_state(n_streams, ref.start_sequences(rng, n_streams))
        rings, _ = ref.traffic_rings(rng, n_streams, cap, state["expected"])
        proc, rx = receiver(b, rings, state)
        want = check_poll(b, proc, rx, rings, state)
        seen |= set(want[1]["status"].tolist())
        check_poll(b, proc, rx, want[4], want[5])   # what waited still waits; bytes behind an EOT are scanned now
        rx.close()
        b.close()
        b.made = []
    if n_streams >= 255:
        assert seen == {no.XM_NEED_MORE, no.XM_EOT, no.XM_INVALID_SEQUENCE, no.XM_INVALID_CRC, no.XM_UNEXPECTED_SEQUENCE}


def test_66000_streams_take_a_second_totals_pass(bench):
    n_streams, cap = 66000, 64
    rng = np.random.default_rng(66)
    b = bench(n_streams, cap)
    state = zero_state(n_streams, ref.start_sequences(rng, n_streams))
    rings, _ = ref.traffic_rings(rng, n_streams, cap, state["expected"], idle=0.97)
    rings.n[-1], rings.n[0] = max(rings.n[-1], 1), max(rings.n[0], 1)   # the first lane and the last one of the partial workgroup hold bytes
    proc, rx = receiver(b, rings, state)
    want = check_poll(b, proc, rx, rings, state)
    assert len(want[0]) > 500 and want[0][-1] > 65536
    rx.close()


def rings_of_image(image, n_streams, cap):
    """(r, n, ring bytes) out of a processor image"""
    img = np.frombuffer(bytes(image), np.uint8)
    rec = int(img[12:16].view("<u4")[0])
    recs = img[drain_ref.HEADER_BYTES:].reshape(n_streams, rec)
    words = recs[:, :16].copy().view("<u4").reshape(n_streams, 4)
    return words[:, 1].astype(np.int64), words[:, 2].astype(np.int64), recs[:, drain_ref.REC_FIXED:drain_ref.REC_FIXED + cap].copy()


def test_cut_invariance(bench):
    """a byte string fed in 3-6 pieces, polled after each, gives what one scan of the whole string up to its last complete step
    gives -- for every string without an error step.  The receiver and the rings are carried from piece to piece through state() /
    set_state and the snapshot, into a clone each time; a stream that reported EOT is masked out from then on, as a host that has
    seen the end of a transfer stops polling it (one scan ends there too)."""
    n_streams, cap = 300, 1024
    rng = np.random.default_rng(0x1A7)
    b = bench(n_streams, cap)
    e0 = ref.start_sequences(rng, n_streams)
    strings = [ref.traffic(rng, cap, int(e0[s]), p_error=0.25) for s in range(n_streams)]
    whole = [ref.poll_one(st, int(e0[s]))[0] for s, st in enumerate(strings)]
    qualify = [s for s, w in enumerate(whole) if w["status"] not in ref.ERRORS]
    assert len(qualify) >= 200
    cuts = [np.sort(rng.integers(0, len(st) + 1, int(rng.integers(2, 6)))) for st in strings]   # 2-5 cuts: 3-6 pieces
    pieces = [[st[a:z] for a, z in zip(np.concatenate([[0], c]), np.concatenate([c, [len(st)]]))] for st, c in zip(strings, cuts)]
    state = zero_state(n_streams, e0)
    r, n, ring = np.zeros(n_streams, np.int64), np.zeros(n_streams, np.int64), np.zeros((n_streams, cap), np.uint8)
    payload = [b""] * n_streams
    done = np.zeros(n_streams, bool)
    for k in range(6):
        for s in range(n_streams):
            if k < len(pieces[s]) and len(pieces[s][k]):
                piece = np.frombuffer(pieces[s][k], np.uint8)
                ring[s, (r[s] + n[s] + np.arange(len(piece))) % cap] = piece
                n[s] += len(piece)
        proc, rx = receiver(b, drain_ref.Rings(r, n, ring), state)
        for s, (res, data) in rx.poll_active(mask=~done).items():
            payload[s] += data
            done[s] |= res["status"] == no.XM_EOT
        state = rx.state()
        r, n, ring = rings_of_image(proc.snapshot().processor, n_streams, cap)
        rx.close()
        b.close()
        b.made = []
    for s in qualify:
        w = whole[s]
        assert payload[s] == w["data"], s
        assert (state["expected"][s], state["packets"][s], state["dropped"][s]) == (w["expected_after"], w["packets"], w["dropped"]), s


def test_a_masked_out_stream_is_untouched_and_polled_correctly_afterwards(bench):
    n_streams, cap = 300, 100
    rng = np.random.default_rng(31)
    b = bench(n_streams, cap)
    state = zero_state(n_streams, ref.start_sequences(rng, n_streams))
    state["packets"][:] = rng.integers(0, 1000, n_streams)
    rings, _ = ref.traffic_rings(rng, n_streams, cap, state["expected"])
    mask = rng.random(n_streams) < 0.5
    proc, rx = receiver(b, rings, state)
    want = check_poll(b, proc, rx, rings, state, mask=mask)   # (the image and state() comparisons cover every word of the others)
    out = ~mask & (rings.n > 0)
    assert out.sum() > 50 and np.array_equal(want[4].n[out], rings.n[out]) and np.array_equal(want[5]["expected"][out], state["expected"][out])
    check_poll(b, proc, rx, want[4], want[5])
    rx.close()


def test_overflow_is_atomic_and_sizes_are_reported(bench):
    n_streams, cap = 600, 100
    rng = np.random.default_rng(9)
    b = bench(n_streams, cap)
    state = zero_state(n_streams, ref.start_sequences(rng, n_streams))
    rings, _ = ref.traffic_rings(rng, n_streams, cap, state["expected"])
    proc, rx = receiver(b, rings, state)
    ws, wr, wo, wd, after, wstate = ref.poll_ref(rings, state["expected"])
    assert len(ws) > 100 and len(wd) > 100
    before = proc.snapshot().processor
    L = rx._L
    streams, offsets, data = np.zeros(len(ws), np.uint32), np.zeros(len(ws) + 1, np.uint32), np.zeros(len(wd), np.uint8)
    results = np.zeros(len(ws), ref.RESULT_DTYPE)
    ne, nb = C.c_uint32(0), C.c_uint32(0)

    def call(cap_streams, cap_bytes, lists=True):
        ne.value = nb.value = 0xFFFFFFFF
        p = (lambda a: a.ctypes.data) if lists else (lambda a: None)
        return L.fskhip_xmodem_rx_poll_host(rx._h, None, p(streams), p(results), p(offsets), cap_streams, p(data), cap_bytes, C.byref(ne), C.byref(nb))
    for cap_streams, cap_bytes, lists in ((len(ws) - 1, len(wd), True), (len(ws), len(wd) - 1, True), (0, 0, False)):
        assert call(cap_streams, cap_bytes, lists) == E_OVERFLOW
        assert "nothing was polled" in L.fskhip_last_error().decode()
        assert (ne.value, nb.value) == (len(ws), len(wd))
        assert proc.snapshot().processor == before and same_state(rx.state(), state)   # swallowed noise included
    assert call(len(ws), len(wd)) == 0 and (ne.value, nb.value) == (len(ws), len(wd))
    assert np.array_equal(streams, ws) and np.array_equal(offsets, wo) and np.array_equal(data, wd) and results.tolist() == wr.tolist()
    assert proc.snapshot().processor == after.image(fresh=b.fresh.processor) and same_state(rx.state(), wstate)
    # the size query of a batch with nothing to report is an ordinary poll that lists nothing
    ws2 = ref.poll_ref(after, wstate["expected"])[0]
    assert (call(0, 0, False) == 0 and (ne.value, nb.value) == (0, 0)) if len(ws2) == 0 else (call(0, 0, False) == E_OVERFLOW and ne.value == len(ws2))
    # state_set names the first bad stream and sets nothing
    bad = wstate["expected"].copy()
    bad[[17, 40]] = [0, 256]
    assert L.fskhip_xmodem_rx_state_set(rx._h, bad.ctypes.data, None, None) == E_INVALID
    assert L.fskhip_last_error().decode() == "fskhip_xmodem_rx_state_set: expected[17] = 0 is not a sequence number (1-255)"
    rx.reset(3)   # initializeReceive() for one stream, then for all: expected = 1, the counters stay
    want = wstate["expected"].copy()
    want[3] = 1
    st = rx.state()
    assert np.array_equal(st["expected"], want) and np.array_equal(st["packets"], wstate["packets"]) and np.array_equal(st["dropped"], wstate["dropped"])
    rx.reset()
    st = rx.state()
    assert (st["expected"] == 1).all() and np.array_equal(st["packets"], wstate["packets"]) and st["packets"].sum() > 0
    rx.close()


def test_device_form(bench):
    n_streams, cap = 700, 1024
    rng = np.random.default_rng(11)
    b = bench(n_streams, cap)
    state = zero_state(n_streams, ref.start_sequences(rng, n_streams))
    rings, _ = ref.traffic_rings(rng, n_streams, cap, state["expected"])
    mask = (rng.random(n_streams) < 0.7).astype(np.uint8)
    ws, wr, wo, wd, after, wstate = ref.poll_ref(rings, state["expected"], mask)
    dev, rx = receiver(b, rings, state)
    L, eh, lib = rx._L, dev.engine._h, b.wm._lib
    hip, stream = _hip_runtime(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0 and stream.value   # a stream of the caller's own, not the null stream
    sizes = {"mask": n_streams, "streams": 4 * len(ws), "results": 40 * len(ws), "offsets": 4 * (len(ws) + 1), "data": len(wd), "totals": 12}
    d = {}
    for k, nbytes in sizes.items():
        p = C.c_void_p()
        lib.check(L.fskhip_device_malloc(eh, nbytes, C.byref(p)))
        d[k] = p
    try:
        lib.check(L.fskhip_memcpy_h2d(eh, d["mask"], mask.ctypes.data, n_streams))
        before = dev.snapshot().processor

        def run(cap_streams, cap_bytes):
            lib.check(L.fskhip_xmodem_rx_poll_device(rx._h, d["mask"], d["streams"], d["results"], d["offsets"], cap_streams, d["data"], cap_bytes, d["totals"], stream))
            assert hip.hipStreamSynchronize(stream) == 0
            totals = np.zeros(3, np.uint32)
            lib.check(L.fskhip_memcpy_d2h(eh, totals.ctypes.data, d["totals"], 12))
            return list(totals)
        assert run(len(ws) - 1, len(wd)) == [len(ws), len(wd), 0]
        assert run(len(ws), len(wd) - 1) == [len(ws), len(wd), 0]
        assert dev.snapshot().processor == before and same_state(rx.state(), state)
        assert run(len(ws), len(wd)) == [len(ws), len(wd), 1]
        gs, go, gd = np.zeros(len(ws), np.uint32), np.zeros(len(ws) + 1, np.uint32), np.zeros(len(wd), np.uint8)
        gr = np.zeros(len(ws), ref.RESULT_DTYPE)
        for arr, k in ((gs, "streams"), (gr, "results"), (go, "offsets"), (gd, "data")):
            lib.check(L.fskhip_memcpy_d2h(eh, arr.ctypes.data, d[k], arr.nbytes))
        assert np.array_equal(gs, ws) and np.array_equal(go, wo) and np.array_equal(gd, wd) and gr.tolist() == wr.tolist()
        assert dev.snapshot().processor == after.image(fresh=b.fresh.processor) and same_state(rx.state(), wstate)
    finally:
        for p in d.values():
            L.fskhip_device_free(eh, p)
        hip.hipStreamDestroy(stream)
        rx.close()


def test_end_to_end_from_samples_to_payloads():
    """two serialised packets per stream, modulated, demodulated quantum by quantum into the RX rings, polled once mid-signal and
    once at the end: the union of the polls is what was sent, every stream expects 3, nothing is left in any ring"""
    import webaudio_modem_amd as wm
    S = 70
    rng = np.random.default_rng(70)
    sent = [[bytes(rng.integers(0, 256, (s + 11 * k) % 25, dtype=np.uint8)) for k in range(2)] for s in range(S)]
    wires = [b"".join(wm.serialize_batch([1, 2], sent[s])) for s in range(S)]
    tx = wm.FSKEngine(S, {}, precision=wm.PRECISION_F32)
    signals = tx.modulate_data(wires)
    tx.close()
    chunk = 2048
    n = (max(len(x) for x in signals) + 4 * chunk + chunk - 1) // chunk * chunk   # (silence behind the signal flushes the last byte)
    buf = np.zeros((S, n), np.float32)
    for s, x in enumerate(signals):
        buf[s, :len(x)] = x
    eng = wm.FSKEngine(S, {}, precision=wm.PRECISION_F32)
    proc = wm.FSKProcessorBatch(eng, rx_capacity=1024)
    rx = wm.XModemReceiverBatch(proc)
    got = [b""] * S
    polls = []
    for q in range(n // chunk):
        proc.process(buf[:, q * chunk:(q + 1) * chunk], 0)
        if q == n // chunk // 2 or q == n // chunk - 1:
            active = rx.poll_active()
            polls.append(len(active))
            for s, (res, data) in active.items():
                assert res["status"] == no.XM_NEED_MORE and res["dropped"] == 0
                got[s] += data
    assert got == [a + b for a, b in sent]
    st = rx.state()
    assert (st["expected"] == 3).all() and (st["packets"] == 2).all() and not st["dropped"].any()
    assert not proc.rx_lengths().any() and polls[0] > 0
    rx.close()
    proc.close()
    eng.close()
