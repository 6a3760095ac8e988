"""fskhip_processor_process_rate_* on the GPU (include/fskhip_next.h; FSKProcessorBatch.process_samples_at): one FSKProcessor quantum
with both sides at a trunk's low rate.  Every comparison is bit for bit against the chain of the existing calls on a twin processor
with twin handles -- Upsampler.process -> process() -> Downsampler.process -- never against the code under test: the elements
written, tx_state(), the drained rings, the handles' histories and the snapshot images of processor and engine, after every quantum."""
import ctypes as C

import numpy as np
import pytest

import processor_rate_ref as model
import samples_ref as sr

pytestmark = pytest.mark.gpu

CFG = {}                                   # the reference's defaults: 48 kHz, 1200 baud, 40 samples per bit
QUANTA = (160, 37, 3, 1)                   # a 20 ms packet at 8 kHz, odd, shorter than the generator's step, a single sample
SHAPES = [(fmt, layout) for fmt in ("f32", "s16", "mulaw", "alaw") for layout in ("stream", "sample")]
# the decimators: the default design of factor 6 (97 taps); 6 taps at factor 2, whose history of 5 is no multiple of the factor; one
# tap at factor 1, which has no history
DESIGNS = {"L6-default": (6, None), "L2-6taps": (2, [0.11, -0.23, 0.52, 0.47, -0.19, 0.07]), "L1-1tap": (1, [0.75])}


@pytest.fixture(scope="module")
def wm():
    import __graft_entry__ as ge
    ge.build()
    import webaudio_modem_amd as wm
    return wm


def twins(wm, S, precision, clear=True):
    engs = [wm.FSKEngine(S, CFG, precision=precision) for _ in range(2)]
    return engs, [wm.FSKProcessorBatch(e, rx_capacity=1024, clear_rx_on_tx_complete=clear) for e in engs]


def close(*things):
    for x in things:
        x.close()


def same_state(procs):
    a, b = (p.snapshot() for p in procs)
    return a.processor == b.processor and a.engine == b.engine


def same_tx(ref, dut):
    a, b = ref.tx_state(), dut.tx_state()
    return all(np.array_equal(a[k], b[k]) for k in a)


def payloads(S, seed):
    """ragged payloads of 0..3 bytes; every fifth stream idle"""
    rng = np.random.default_rng(seed)
    return [b"" if s % 5 == 4 else bytes(rng.integers(0, 256, 1 + (s + seed) % 3, dtype=np.uint8)) for s in range(S)]


def tx_equal_after_every_quantum(wm, S, eprec, dprec, factor, taps, quanta=QUANTA, min_quanta=0):
    """the run of the issue: start; a second modulation started (behind a reset) while the first still rings; completion inside a
    quantum; a third modulation started in the quantum after that completion, as an XModem reply is; its completion; the tail into
    silence.  Formats and layouts take turns so that each meets every quantum length.  (A frame ends in bitsPerByte * samplesPerBit =
    400 zeros of its own, so a decimator of up to 401 taps has just rung out when its stream completes: the third modulation meets a
    history that still rings only in the 1 025-tap case, which asserts it.)"""
    engs, (ref, dut) = twins(wm, S, getattr(wm, "PRECISION_" + eprec))
    dns = [wm.Downsampler(factor, S, taps=taps, precision=getattr(wm, "PRECISION_" + dprec)) for _ in range(2)]
    for p in (ref, dut):
        p.modulate(payloads(S, 1))
    k, stage, quiet = 0, 0, 0
    while True:
        n = quanta[k % len(quanta)]
        fmt, layout = SHAPES[(k + k // len(quanta)) % len(SHAPES)]
        want = dns[0].process(ref.process(None, n * factor), fmt, layout)
        got = dut.process_samples_at(None, n_out=n, out_fmt=fmt, out_layout=layout, downsampler=dns[1])
        where = (k, n, fmt, layout, stage)
        assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), (where, np.argwhere(got != want)[:4])
        assert same_tx(ref, dut), where
        assert dns[0].state().tobytes() == dns[1].state().tobytes(), where
        assert same_state((ref, dut)), where
        assert ref.demodulate() == dut.demodulate(), where
        k += 1
        if stage == 0 and k == 4:                       # mid-tone: cancel, and start the next while the filter still rings
            for p in (ref, dut):
                p.reset()
                p.modulate(payloads(S, 2))
            assert factor == 1 or np.abs(dns[0].state()).max() > 0.1
            stage = 1
        elif stage == 1 and not ref.tx_state()["isModulating"].any():
            # completed inside that quantum: the reply starts in the next one (the idle streams' empty modulators stay pending)
            free = ~ref.tx_state()["pendingModulation"]
            assert free.any() and (len(dns[0].taps) <= 401 or np.abs(dns[0].state()).max() > 0)
            for p in (ref, dut):
                p.modulate(payloads(S, 3), mask=free)
            stage = 2
        elif stage == 2 and not ref.tx_state()["isModulating"].any():
            stage = 3                                   # completed again: now the tail into silence
        elif stage == 3:
            quiet += 1
            if quiet >= 2 * len(quanta) and k >= min_quanta:
                break
    assert ref.tx_state()["completed"].max() == 2 and not dns[1].state().any()      # rung out
    assert got.tobytes() == np.full(got.shape, sr.silence(fmt), got.dtype).tobytes()
    close(*dns, ref, dut, *engs)
    return k


TX_CASES = [(S, e, d, design) for design in DESIGNS
            for S, e, d in ((65, "F32", "F32"), (65, "F64", "F64"), (65, "F32", "F64"), (65, "F64", "F32"), (130, "F32", "F32"), (1, "F64", "F32"))]


@pytest.mark.parametrize("S,eprec,dprec,design", TX_CASES, ids=["%d-%s-%s-%s" % c for c in TX_CASES])
def test_tx_is_the_decimated_encoded_output_of_process(wm, S, eprec, dprec, design):
    factor, taps = DESIGNS[design]
    k = tx_equal_after_every_quantum(wm, S, eprec, dprec, factor, taps, min_quanta=4 * len(SHAPES))
    assert k >= 4 * len(SHAPES)          # every format and layout met every quantum length


def test_tx_fallback_through_the_float_tile(wm):
    """1 025 taps at factor 6 are beyond the fused kernel's delay line: the two launches, with the same equalities"""
    taps = wm.FilterDesign.sincLowpass(3600.0, 48000.0, 1025)
    assert len(taps) == 1025
    tx_equal_after_every_quantum(wm, 3, "F32", "F32", 6, taps)


@pytest.mark.parametrize("precision", ("F32", "F64"))
def test_device_form_stream_major_rows_on_and_off_the_16_byte_grid(wm, precision):
    """Stream-major output straight into a caller's device buffer: rows whose pitch is no multiple of 16 bytes, rows at such a pitch
    behind a base one element off, and rows on the grid (the vector path with its partial last vector).  70 streams are a whole and
    a partial 64-stream block.  Every element equals the twin chain's, every other element of the buffer keeps its sentinel."""
    from hip_caller import Caller
    S, factor = 70, 6
    engs, (ref, dut) = twins(wm, S, getattr(wm, "PRECISION_" + precision))
    dns = [wm.Downsampler(factor, S) for _ in range(2)]
    for p in (ref, dut):
        p.modulate([bytes([s, 255 - s])[:1 + s % 2] for s in range(S)])
    longest = int(max(ref.tx_state()["totalSamples"]))
    c = Caller(engs[1])
    cap = S * 176 + 16
    d_buf = c.malloc(cap * 4)
    shapes = [(fmt, how) for fmt in ("f32", "s16", "mulaw", "alaw") for how in ("odd pitch", "offset base", "on the grid")]
    done, k = 0, 0
    while done < longest + 97 + 160 * factor or k < len(shapes):
        n = (50, 37, 160, 3, 45)[k % 5]
        fmt, how = shapes[k % len(shapes)]
        dtype, esz = sr.DTYPES[fmt], np.dtype(sr.DTYPES[fmt]).itemsize
        pitch = (n + 3 + ((n + 3) % 8 == 0)) if how == "odd pitch" else (n + 15) & ~15      # (odd: no multiple of 8 elements)
        first = 1 if how == "offset base" else 0
        assert how == "on the grid" or (pitch * esz) % 16 or first
        sentinel = np.array([0x5A5A5A5A], np.uint32).view(dtype)[0]
        h = np.full(cap, sentinel, dtype)
        c.upload(d_buf, h)
        want = dns[0].process(ref.process(None, n * factor), fmt, "stream")
        dut.process_samples_at_device(None, "mulaw", "sample", 0, 0, None, d_buf + first * esz, fmt, "stream", n, pitch, dns[1], stream=c.stream)
        c.sync()
        c.download(d_buf, h)
        rows = h[first:first + S * pitch].reshape(S, pitch)
        assert rows[:, :n].tobytes() == want.tobytes(), (k, fmt, how, n, np.argwhere(rows[:, :n] != want)[:4])
        poison = np.full(1, sentinel, dtype).tobytes()
        for rest in (rows[:, n:], h[:first], h[first + S * pitch:]):
            assert rest.tobytes() == poison * rest.size, (k, fmt, how, n)
        assert same_state((ref, dut)) and dns[0].state().tobytes() == dns[1].state().tobytes(), (k, fmt, how, n)
        done, k = done + n * factor, k + 1
    assert k >= len(shapes) and not dut.tx_state()["isModulating"].any()
    c.close()
    close(*dns, ref, dut, *engs)


@pytest.fixture(scope="module")
def trunk_frames(wm):
    """three payloads as 8 kHz float frames [n, 3] from modulate_samples_at, made once and left unchanged"""
    eng = wm.FSKEngine(3, CFG, precision=wm.PRECISION_F64)
    dn = wm.Downsampler(6, 3)
    pay = [b"rx0", b"\x00\xff\x55", b"Hi"]
    x, lens = eng.modulate_samples_at(pay, "f32", "stream", dn)
    close(dn, eng)
    x.setflags(write=False)
    return pay, x


def capture(trunk_frames, S, fmt):
    """[S, n] low rate samples of `fmt`: stream s one of the frames at 0.9 of full scale behind its own lead, and silence behind"""
    _, sig = trunk_frames
    x = np.zeros((S, sig.shape[1] + 7 + 200), np.float32)
    for s in range(S):
        x[s, s % 7:s % 7 + sig.shape[1]] = np.float32(0.9) * sig[s % 3]
    return sr.quantise(x, fmt)


@pytest.mark.parametrize("layout", ("stream", "sample"))
@pytest.mark.parametrize("fmt", ("mulaw", "s16"))
def test_rx_state_is_that_of_the_interpolated_process(wm, trunk_frames, fmt, layout):
    S = 65
    pay, _ = trunk_frames
    engs, (ref, dut) = twins(wm, S, wm.PRECISION_F32)
    ups = [wm.Upsampler(6, S) for _ in range(2)]
    xq = capture(trunk_frames, S, fmt)
    pos, k, got = 0, 0, [b""] * S
    while pos < xq.shape[1]:
        n = min((160, 37)[k % 2], xq.shape[1] - pos)
        part = xq[:, pos:pos + n] if layout == "stream" else np.ascontiguousarray(xq[:, pos:pos + n].T)
        ref.process(ups[0].process(part, fmt, layout), 0)
        assert dut.process_samples_at(part, fmt, layout, ups[1]) is None
        assert ups[0].state().tobytes() == ups[1].state().tobytes(), (k, n)
        assert np.array_equal(ref.rx_lengths(), dut.rx_lengths()) and same_state((ref, dut)), (k, n)      # ring contents and counts, engine state
        assert ref.status(S - 1) == dut.status(S - 1), (k, n)
        # 'eod': the engine keeps every stream's count (eodCount), in its image and, read here for every stream, in its status
        assert [ref.engine.get_status(s)["eodCount"] for s in range(S)] == [dut.engine.get_status(s)["eodCount"] for s in range(S)], (k, n)
        pos, k = pos + n, k + 1
        if k % 8 == 0:
            a, b = ref.demodulate(), dut.demodulate()
            assert a == b, k
            got = [g + x for g, x in zip(got, b)]
    a, b = ref.demodulate(), dut.demodulate()
    assert a == b and ref.processDemodulationCallCount == dut.processDemodulationCallCount == k
    assert [g + x for g, x in zip(got, b)] == [pay[s % 3] for s in range(S)]
    close(*ups, ref, dut, *engs)


@pytest.mark.parametrize("S,precision", ((65, "F32"), (3, "F64")))
def test_both_sides_in_one_call_with_different_formats(wm, trunk_frames, S, precision):
    """one call of 4 q against four rounds of the chain at q, s16 rows in and A-law frames out: the same elements and the same state"""
    q = 40
    # (without the RX clear on completion: that clears what the completing call has put, which is more in a call of 4 q)
    engs, (ref, dut) = twins(wm, S, getattr(wm, "PRECISION_" + precision), clear=False)
    ups, dns = [wm.Upsampler(6, S) for _ in range(2)], [wm.Downsampler(6, S) for _ in range(2)]
    for p in (ref, dut):
        p.modulate(payloads(S, 3))
    xq = capture(trunk_frames, S, "s16")
    for pos in range(0, xq.shape[1] - 4 * q, 4 * q):
        four = [dns[0].process(ref.process(ups[0].process(xq[:, pos + i * q:pos + (i + 1) * q], "s16", "stream"), 6 * q), "alaw", "sample") for i in range(4)]
        one = dut.process_samples_at(xq[:, pos:pos + 4 * q], "s16", "stream", ups[1], 4 * q, "alaw", "sample", dns[1])
        assert one.tobytes() == np.concatenate(four).tobytes(), pos
        # (four demodulate calls against one: the engine's call counter, and with it its image, is the one word that differs)
        assert ref.snapshot().processor == dut.snapshot().processor and same_tx(ref, dut), pos
        for s in (0, S // 2, S - 1):
            a, b = ref.status(s), dut.status(s)
            for counter in ("demodulationCalls", "processDemodulationCallCount"):
                assert a.pop(counter) == 4 * b.pop(counter) == 4 * (pos // (4 * q) + 1), (pos, s, counter)
            assert a == b, (pos, s, a, b)
        assert ups[0].state().tobytes() == ups[1].state().tobytes() and dns[0].state().tobytes() == dns[1].state().tobytes(), pos
    assert ref.demodulate() == dut.demodulate()
    assert ref.tx_state()["completed"].max() == 1
    close(*ups, *dns, ref, dut, *engs)


def test_refusals_on_live_handles_in_order(wm):
    from webaudio_modem_amd import _lib
    L = _lib.lib()
    S = 5
    engs, (a, b) = twins(wm, S, wm.PRECISION_F32)
    up, dn, up4, dn4 = wm.Upsampler(6, S), wm.Downsampler(6, S), wm.Upsampler(6, 4), wm.Downsampler(6, 4)
    a.modulate([b"x"] * S)
    a.process_samples_at(np.full((8, S), 0x31, np.uint8), upsampler=up, n_out=8, downsampler=dn)       # histories that are not zero
    before, hist = a.snapshot(), (up.state().tobytes(), dn.state().tobytes())
    buf = np.zeros(256, np.uint8)
    B = buf.ctypes.data
    name = "fskhip_processor_process_rate_host"
    U, D, U4, D4 = up._h, dn._h, up4._h, dn4._h
    for (hu, hd), args, text in (
            ((U, D), (B + 1, 4, 2, 8, 0, B + 1, -1, 7, 8, 0), name + ": unknown sample format 4"),
            # 3. the handles of the sides that have a buffer, input first: null, direction, streams
            ((None, None), (B + 1, 1, 0, 8, 7, B + 1, 1, 0, 8, 7), name + ": null up handle"),
            ((D, None), (B + 1, 1, 0, 8, 7, B + 1, 1, 0, 8, 7), name + ": the up handle resamples down"),
            ((U4, None), (B + 1, 1, 0, 8, 7, B + 1, 1, 0, 8, 7), name + ": the up handle has 4 streams, the processor 5"),
            ((U, None), (B + 1, 1, 0, 8, 7, B + 1, 1, 0, 8, 7), name + ": null down handle"),
            ((None, U), (None, 1, 0, 8, 7, B + 1, 1, 0, 8, 7), name + ": the down handle resamples up"),
            ((U, D4), (B + 1, 1, 0, 8, 7, B + 1, 1, 0, 8, 7), name + ": the down handle has 4 streams, the processor 5"),
            # 4. pitches, in before out
            ((U, D), (B + 1, 1, 0, 8, 7, B + 1, 1, 0, 8, 7), "in_pitch 7 < n_in 8"),
            ((U, D), (B + 1, 2, 1, 8, S - 1, B + 1, 1, 0, 8, 7), "in frame pitch 4 < n_streams 5"),
            ((None, D), (None, 1, 0, 8, 7, B + 1, 1, 0, 8, 7), "out_pitch 7 < n_out 8"),
            ((U, D), (B + 2, 1, 1, 8, S, B + 1, 3, 1, 8, S - 1), "out frame pitch 4 < n_streams 5"),
            # 5. alignment, in before out
            ((U, D), (B + 1, 1, 0, 8, 8, B + 1, 1, 0, 8, 8), "in is not aligned to its element size"),
            ((U, D), (B + 2, 1, 1, 8, S, B + 2, 0, 1, 8, S), "out is not aligned to its element size")):
        assert (L.fskhip_processor_process_rate_host(a._h, hu, hd, *args, 0), L.fskhip_last_error().decode()) == (-1, text)
    assert a.snapshot() == before and (up.state().tobytes(), dn.state().tobytes()) == hist
    # zero lengths and NULL sides are legal, and a side without samples needs no handle
    assert a.process_samples_at(None) is None
    assert a.process_samples_at(np.zeros((0, S), np.uint8), upsampler=up) is None
    assert (up.state().tobytes(), dn.state().tobytes()) == hist
    close(up, dn, up4, dn4, a, b, *engs)


def test_loopback_at_8_khz_equals_the_model(wm):
    """two processors, mu-law frames at 8 kHz in quanta of 160: A's output is B's input, and B's demodulate() gives the model's bytes
    (tests/processor_rate_ref.py, held to the payload by test_processor_rate_cpu.py) after the model's number of quanta"""
    S = 65
    wire, got = model.link()
    engs = [wm.FSKEngine(S, CFG, precision=wm.PRECISION_F64) for _ in range(2)]
    A, B = (wm.FSKProcessorBatch(e, rx_capacity=1024, clear_rx_on_tx_complete=True) for e in engs)
    dn, up = wm.Downsampler(model.FACTOR, S, precision=wm.PRECISION_F64), wm.Upsampler(model.FACTOR, S, precision=wm.PRECISION_F64)
    A.modulate([model.PAYLOAD] * S)
    assert model.signal_quanta(int(A.tx_state()["totalSamples"][0])) + model.TRAILING_QUANTA == wire.shape[0]
    for q in range(wire.shape[0]):
        frames = A.process_samples_at(None, n_out=model.QUANTUM, downsampler=dn)
        assert frames.shape == (model.QUANTUM, S) and frames.dtype == np.uint8
        assert B.process_samples_at(frames, upsampler=up) is None
    assert B.demodulate() == [b"".join(got)] * S == [model.PAYLOAD] * S
    assert not A.tx_state()["pendingModulation"].any()
    close(dn, up, A, B, *engs)


def test_xmodem_file_crosses_the_8_khz_link(wm):
    """an XModemSenderBatch on A and an XModemFileReceiverBatch on B, every sample between them a mu-law frame at 8 kHz that one
    process_samples_at produced and the other consumes, in quanta of 160; the one-packet files arrive intact"""
    import xmodem_recv_ref as ref
    import xmodem_tx_ref as tx_ref
    S, Q = 3, model.QUANTUM
    rng = np.random.default_rng(0x8000)
    files = [bytes(rng.integers(0, 256, n, dtype=np.uint8)) for n in (1, 9, 16)]
    engs = [wm.FSKEngine(S, CFG, precision=wm.PRECISION_F32) for _ in range(2)]
    A, B = (wm.FSKProcessorBatch(e, rx_capacity=1024, clear_rx_on_tx_complete=True) for e in engs)
    hs = [wm.Upsampler(6, S), wm.Downsampler(6, S), wm.Upsampler(6, S), wm.Downsampler(6, S)]
    a_up, a_dn, b_up, b_dn = hs
    tx, rx = wm.XModemSenderBatch(A, 16), wm.XModemFileReceiverBatch(B, 64)
    tx.send(files)
    rx.start()
    a_out = b_out = np.full((Q, S), sr.silence("mulaw"), np.uint8)
    tx_end, rx_end = {}, {}
    for quantum in range(400):
        a_next = A.process_samples_at(b_out, upsampler=a_up, n_out=Q, downsampler=a_dn)
        b_next = B.process_samples_at(a_out, upsampler=b_up, n_out=Q, downsampler=b_dn)
        a_out, b_out = a_next, b_next
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
    assert not tx.state()["retransmitted"].any() and not rx.state()["retries"].any()
    close(tx, rx, *hs, A, B, *engs)
