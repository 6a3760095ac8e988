"""FSKProcessorBatch.process_samples / fskhip_processor_process_fmt_* on the GPU: the streaming quantum with either side in a capture
format and layout, held against the float process() on a twin processor over a twin engine, bit for bit.
  RX  the twin takes process(samples_ref.decode(x)), the processor under test process_samples(x); after every quantum the
      processor's canonical image, the engine's snapshot and, at the end of a run, the demodulate() bytes are identical.
  TX  process_samples(n_out=...) equals samples_ref.encode(process(n_out=...)) element for element, across the quantum in which the
      modulation completes (the zero fill behind it is the format's silence), and the images stay identical.
One pair of twins serves all formats, layouts and quantum lengths of a case one after the other: they stay twins only while every
step before was exact."""
import numpy as np
import pytest

import samples_ref as sr

pytestmark = pytest.mark.gpu

CFG = {}                                                                 # the reference's defaults: 1200 baud, 40 samples per bit
XCFG = dict(baudRate=4800, markFrequency=9600, spaceFrequency=14400)     # 10 samples per bit (the XModem exchange)
FORMATS, LAYOUTS = ("f32", "s16", "mulaw", "alaw"), ("stream", "sample")
QUANTA = (128, 160, 37, 3)          # the real-time quantum, a 20 ms RTP frame at 8 kHz, odd, shorter than a quad
N_OUT = QUANTA + (50,)              # ... and one that ends inside the io kernel's 32-sample tile
STREAMS = (1, 63, 65, 130)          # a partial wave, more than one 64-stream workgroup


@pytest.fixture(scope="module")
def wm():
    import __graft_entry__ as ge
    ge.build()
    import webaudio_modem_amd as wm
    return wm


@pytest.fixture(scope="module")
def frames(wm):
    """three modulated frames of 3 payload bytes, made once and left unchanged"""
    eng = wm.FSKEngine(3, CFG, precision=wm.PRECISION_F64)
    rng = np.random.default_rng(0xF0A7)
    payloads = [bytes(rng.integers(0, 256, 3, dtype=np.uint8)) for _ in range(3)]
    sigs = [np.asarray(s, np.float32) for s in eng.modulate_data(payloads)]
    eng.close()
    return payloads, sigs


def twins(wm, S, precision, rx_capacity=1024, use_graph=(False, False), clear=True):
    engs = [wm.FSKEngine(S, CFG, precision=precision) for _ in range(2)]
    procs = [wm.FSKProcessorBatch(e, rx_capacity=rx_capacity, clear_rx_on_tx_complete=clear, use_graph=g) for e, g in zip(engs, use_graph)]
    return engs, procs


def close(engs, procs):
    for x in list(procs) + list(engs):
        x.close()


def capture(frames, S, fmt, seed):
    """[S, n] samples of format `fmt`: each stream one of the frames at 0.9 of full scale behind its own lead, in a little noise, and
    600 samples between it and the next capture's"""
    _, sigs = frames
    n = max(s.size for s in sigs) + 600
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((S, n)) * 0.004).astype(np.float32)
    for s in range(S):
        sig = sigs[s % 3]
        x[s, s % 7:s % 7 + sig.size] += np.float32(0.9) * sig
    return sr.quantise(x, fmt)


def schedule(total, q):
    """quantum lengths covering `total` samples: q throughout from 128 on; a shorter q between quanta of 128 -- two of them, then seven
    (q = 3) or nine (q = 37) of q, an odd number of samples that leaves the /2 decimator mid-pair, then 128 from that odd position on"""
    if q >= 128:
        lens = [q] * (total // q)
    else:
        k = 7 if q == 3 else 9
        lens = [128, 128] + [q] * k + [128] * ((total - 256 - k * q) // 128)
    return lens + ([total - sum(lens)] if total > sum(lens) else [])


def tx_schedule(longest, q):
    """quantum lengths that carry a modulation of `longest` samples to its end and one quantum beyond: q throughout from 128 on; a
    shorter q for the last ten or so quanta, behind quanta of 128"""
    if q >= 128:
        return schedule(longest + q, q)
    big = max(longest - 10 * q, 0) // 128
    return [128] * big + [q] * ((longest - 128 * big) // q + 2)


def in_layout_view(xq, layout, wide, rng):
    """the samples as process_samples takes them; wide: the frames (or rows) are a block of a wider array full of other values"""
    a = xq if layout == "stream" else np.ascontiguousarray(xq.T)
    if not wide:
        return a
    big = rng.integers(1, 127, (a.shape[0], a.shape[1] + 3)).astype(a.dtype)
    big[:, :a.shape[1]] = a
    return big[:, :a.shape[1]]


def same_state(procs):
    a, b = (p.snapshot() for p in procs)
    return a.processor == b.processor and a.engine == b.engine


CASES = [(S, precision) for S in STREAMS for precision in ("F32", "F64")]


@pytest.mark.parametrize("case", range(len(CASES)), ids=["%d-%s" % c for c in CASES])
def test_rx_state_is_that_of_process_on_the_decoded_floats(wm, frames, case):
    """every format x layout in every case, each with one of the four quantum lengths; over the eight cases every length meets every
    format and layout.  Nothing is drained before the end: eight frames of 3 bytes overrun a ring of 16."""
    S, precision = CASES[case]
    cap = 16 if S in (63, 130) else 1024
    engs, (ref, dut) = twins(wm, S, getattr(wm, "PRECISION_" + precision), rx_capacity=cap)
    rng = np.random.default_rng(S)
    run = 0
    for fmt in FORMATS:
        for layout in LAYOUTS:
            q = QUANTA[(run + run // 4 + case) % 4]
            xq = capture(frames, S, fmt, 1000 * S + run)
            xf = sr.decode(xq, fmt)
            t = 0
            lens = schedule(xq.shape[1], q)
            assert len(lens) >= 3
            for n in lens:
                ref.process(xf[:, t:t + n])
                dut.process_samples(in_layout_view(xq[:, t:t + n], layout, run % 2 == 1, rng), fmt, layout)
                assert same_state((ref, dut)), (q, fmt, layout, t)
                t += n
            run += 1
    assert ref.processDemodulationCallCount == dut.processDemodulationCallCount
    got, want = dut.demodulate(), ref.demodulate()
    assert got == want
    # (the stimulus: most frames were heard, and the ring of 16 ran over)
    assert sum(len(b) for b in want) >= S * min(12, cap) and (cap > 16 or max(len(b) for b in want) == 16), [len(b) for b in want][:8]
    close(engs, (ref, dut))


@pytest.mark.parametrize("q", (37, 3))
def test_short_quanta_meet_every_format_and_layout_at_a_partial_wave(wm, frames, q):
    """the floor under the rotation of the two tests around this one: at 63 streams every format and layout, in and out, meets the odd
    quantum and the one shorter than a quad"""
    S = 63
    engs, (ref, dut) = twins(wm, S, wm.PRECISION_F32, rx_capacity=16)
    run = 0
    for fmt in FORMATS:
        for layout in LAYOUTS:
            xq = capture(frames, S, fmt, 77 + run)
            xf = sr.decode(xq, fmt)
            for p in (ref, dut):
                p.modulate([bytes([s, run])[:1 + s % 2] for s in range(S)])
            longest = int(max(ref.tx_state()["totalSamples"]))
            assert longest + q <= xq.shape[1]
            t = 0
            for n in tx_schedule(longest, q):
                want = sr.encode(ref.process(xf[:, t:t + n], n), fmt)
                got = dut.process_samples(xq[:, t:t + n] if layout == "stream" else np.ascontiguousarray(xq[:, t:t + n].T), fmt, layout, n, fmt, layout)
                assert got.tobytes() == (want.T if layout == "sample" else want).tobytes(), (fmt, layout, t)
                assert same_state((ref, dut)), (fmt, layout, t)
                t += n
            assert not dut.tx_state()["pendingModulation"].any()
            run += 1
    assert dut.demodulate() == ref.demodulate()
    close(engs, (ref, dut))


def fmt_host_wide(wm, proc, n_out, fmt, layout, extra=3):
    """fskhip_processor_process_fmt_host into a block of a wider array: (the block, the whole array, the sentinel)"""
    from webaudio_modem_amd import _lib
    S = proc.n_streams
    rows, cols = (S, n_out) if layout == "stream" else (n_out, S)
    sentinel = sr.DTYPES[fmt](77)
    big = np.full((rows, cols + extra), sentinel, sr.DTYPES[fmt])
    _lib.check(_lib.lib().fskhip_processor_process_fmt_host(proc._h, None, 0, 0, 0, 0, big.ctypes.data, sr.FORMATS[fmt], sr.LAYOUTS[layout], n_out, cols + extra,
                                                             proc.flags))
    return big[:, :cols], big, sentinel


@pytest.mark.parametrize("case", range(len(CASES)), ids=["%d-%s" % c for c in CASES])
def test_tx_is_the_encoded_output_of_process(wm, frames, case):
    """every format x layout in every case, each with one of the five output lengths, rotating over the cases as in the RX test"""
    S, precision = CASES[case]
    engs, (ref, dut) = twins(wm, S, getattr(wm, "PRECISION_" + precision))
    payloads, sigs = frames
    rng = np.random.default_rng(7 * S)
    heard = np.zeros((S, 2 * (sigs[0].size + 608)), np.float32)      # the same frame twice
    heard[:, 8:8 + sigs[0].size] = sigs[0]
    heard[:, 616 + sigs[0].size:616 + 2 * sigs[0].size] = sigs[0]
    run, kept = 0, 0
    for fmt in FORMATS:
        for layout in LAYOUTS:
            q = N_OUT[(run + run // 5 + case) % 5]
            for p in (ref, dut):              # every ring holds a frame's bytes for the completion to clear
                p.reset()
                p.process(heard)
            # ragged payloads: stream 0 an empty one (pending for good, never a sample), stream 1 (or the last) a single byte
            rows = [bytes(rng.integers(0, 256, 1 + s % 2, dtype=np.uint8)) for s in range(S)]
            rows[0] = b""
            rows[min(1, S - 1)] = rows[min(1, S - 1)][:1] if S > 1 else b""
            if S == 1 and run % 2:
                rows[0] = b"\xa5"             # (one stream: alternately the empty and the one-byte payload)
            for p in (ref, dut):
                p.modulate(rows)
            longest = max(ref.tx_state()["totalSamples"])
            lens = tx_schedule(int(longest), q)
            wide = run % 2 == 1
            for n in lens:
                want = sr.encode(ref.process(None, n), fmt)
                if layout == "sample":
                    want = want.T
                if wide:
                    got, big, sentinel = fmt_host_wide(wm, dut, n, fmt, layout)
                    assert (big[:, got.shape[1]:] == sentinel).all(), (q, fmt, layout)       # the other columns are untouched
                else:
                    got = dut.process_samples(None, n_out=n, out_fmt=fmt, out_layout=layout)
                assert got.dtype == sr.DTYPES[fmt] and got.shape == want.shape
                assert got.tobytes() == want.tobytes(), (q, fmt, layout, n, np.argwhere(got != want)[:4])
                assert same_state((ref, dut)), (q, fmt, layout, n)
            st = dut.tx_state()
            assert not st["isModulating"].any() and list(st["pendingModulation"]) == [not r for r in rows]
            assert (got == sr.silence(fmt)).all()                                             # the last quantum: silence everywhere
            left = dut.rx_lengths()
            assert all(left[s] == 0 for s in range(S) if rows[s])                             # clear_rx_on_tx_complete ...
            kept = max([kept] + [int(left[s]) for s in range(S) if not rows[s]])
            run += 1
    assert kept > 0                                                                       # ... and only there: a pending stream kept its bytes
    close(engs, (ref, dut))


@pytest.mark.parametrize("S,precision", ((65, "F32"), (130, "F64"), (1, "F32")))
def test_both_sides_in_one_call_with_different_formats(wm, frames, S, precision):
    engs, (ref, dut) = twins(wm, S, getattr(wm, "PRECISION_" + precision), rx_capacity=16)
    rng = np.random.default_rng(S)
    pairs = ((("mulaw", "sample"), ("s16", "stream")), (("s16", "stream"), ("alaw", "sample")), (("f32", "stream"), ("mulaw", "stream")),
             (("alaw", "stream"), ("f32", "stream")), (("f32", "sample"), ("f32", "sample")))
    for i, ((ifmt, ilay), (ofmt, olay)) in enumerate(pairs):
        xq = capture(frames, S, ifmt, 31 * S + i)
        xf = sr.decode(xq, ifmt)
        for p in (ref, dut):
            p.reset()
            p.modulate([bytes([s & 0xFF, i]) for s in range(S)])
        t = 0
        for n in schedule(xq.shape[1], (160, 37, 128, 3, 160)[i]):
            want = sr.encode(ref.process(xf[:, t:t + n], n), ofmt)
            got = dut.process_samples(in_layout_view(xq[:, t:t + n], ilay, i % 2 == 0, rng), ifmt, ilay, n, ofmt, olay)
            assert got.tobytes() == (want.T if olay == "sample" else want).tobytes(), (i, t)
            assert same_state((ref, dut)), (i, t)
            t += n
        assert dut.demodulate() == ref.demodulate()
    close(engs, (ref, dut))


def test_graph_replays_equal_the_plain_launches(wm, frames):
    """use_graph=True: four quanta of one shape replay one capture; another n_in, then another format, capture afresh"""
    S = 65
    engs, (ref, dut) = twins(wm, S, wm.PRECISION_F32, use_graph=(False, True))
    for p in (ref, dut):
        p.modulate([bytes([s, 1, 2]) for s in range(S)])
    steps = [("mulaw", "sample", 128)] * 4 + [("mulaw", "sample", 160)] * 2 + [("s16", "sample", 160)] * 2 + [("s16", "stream", 37)] * 3 + [("mulaw", "sample", 128)] * 2
    xs = {f: capture(frames, S, f, 5) for f in ("mulaw", "s16")}
    t = 0
    for fmt, layout, n in steps:
        x = xs[fmt][:, t:t + n]
        x = x if layout == "stream" else np.ascontiguousarray(x.T)
        want = ref.process_samples(x, fmt, layout, n, fmt, layout)
        got = dut.process_samples(x, fmt, layout, n, fmt, layout)
        assert got.tobytes() == want.tobytes(), (fmt, layout, n, t)
        assert same_state((ref, dut)), (fmt, layout, n, t)
        t += n
    assert dut.demodulate() == ref.demodulate()
    close(engs, (ref, dut))


def test_device_form_on_caller_buffers_and_stream(wm, frames):
    """fskhip_processor_process_fmt_device on device buffers of the caller's and a HIP stream of the caller's, frames wider than the
    batch on both sides: the output and the state are the host form's on the twin, the other columns untouched"""
    from hip_caller import Caller
    S, n = 130, 160
    engs, (ref, dut) = twins(wm, S, wm.PRECISION_F32)
    for p in (ref, dut):
        p.modulate([bytes([s & 0xFF]) * 2 for s in range(S)])
    xq = capture(frames, S, "alaw", 9)
    c = Caller(engs[1])
    pitch = S + 6
    d_in, d_out = c.malloc(n * pitch), c.malloc(n * pitch * 2)
    for k in range(4):
        x = np.ascontiguousarray(xq[:, k * n:(k + 1) * n].T)
        want = ref.process_samples(x, "alaw", "sample", n, "s16", "sample")
        h_in = np.full((n, pitch), 0x2A, np.uint8)
        h_in[:, :S] = x
        h_out = np.full((n, pitch), 1234, np.int16)
        c.upload(d_in, h_in)
        c.upload(d_out, h_out)
        dut.process_samples_device(d_in, "alaw", "sample", n, pitch, d_out, "s16", "sample", n, pitch, stream=c.stream)
        c.sync()
        c.download(d_out, h_out)
        assert h_out[:, :S].tobytes() == want.tobytes(), k
        assert (h_out[:, S:] == 1234).all()
        assert same_state((ref, dut)), k
    c.close()
    close(engs, (ref, dut))


@pytest.mark.parametrize("precision", ("F32", "F64"))
def test_device_form_stream_major_rows_on_and_off_the_16_byte_grid(wm, precision):
    """Stream-major output straight into a caller's device buffer, where the io kernel's store path is the caller's choice: rows whose
    pitch is no multiple of 16 bytes, rows at such a pitch behind a base one element off, and rows on the grid (the vector path with
    its partial last vector).  70 streams are a whole and a partial 64-stream block; the lengths end inside a 32-sample tile.  Every
    element equals the twin's encoded process(), every other element of the buffer keeps its sentinel."""
    from hip_caller import Caller
    S = 70
    engs, (ref, dut) = twins(wm, S, getattr(wm, "PRECISION_" + precision))
    for p in (ref, dut):
        p.modulate([bytes([s, 255 - s])[:1 + s % 2] for s in range(S)])
    longest = int(max(ref.tx_state()["totalSamples"]))
    c = Caller(engs[1])
    cap = S * 160 + 16
    d_buf = c.malloc(cap * 2)
    shapes = [(fmt, how) for fmt in ("s16", "mulaw", "alaw") for how in ("odd pitch", "offset base", "on the grid")]
    done, k = 0, 0
    while done < longest + 128:
        n = (50, 37, 128, 3, 45)[k % 5]
        fmt, how = shapes[k % len(shapes)]
        dtype, esz = sr.DTYPES[fmt], np.dtype(sr.DTYPES[fmt]).itemsize
        pitch = (n + 3 + ((n + 3) % 8 == 0)) if how == "odd pitch" else (n + 15) & ~15      # (odd: no multiple of 8 elements)
        first = 1 if how == "offset base" else 0
        assert how == "on the grid" or (pitch * esz) % 16 or first
        sentinel = dtype(0x5A)
        h = np.full(cap, sentinel, dtype)
        c.upload(d_buf, h)
        want = sr.encode(ref.process(None, n), fmt)
        dut.process_samples_device(None, "f32", "stream", 0, 0, d_buf + first * esz, fmt, "stream", n, pitch, stream=c.stream)
        c.sync()
        c.download(d_buf, h)
        rows = h[first:first + S * pitch].reshape(S, pitch)
        assert rows[:, :n].tobytes() == want.tobytes(), (k, fmt, how, n, np.argwhere(rows[:, :n] != want)[:4])
        assert (rows[:, n:] == sentinel).all() and (h[:first] == sentinel).all() and (h[first + S * pitch:] == sentinel).all(), (k, fmt, how, n)
        assert same_state((ref, dut)), (k, fmt, how, n)
        done, k = done + n, k + 1
    assert k >= 2 * len(shapes) and not dut.tx_state()["isModulating"].any()
    c.close()
    close(engs, (ref, dut))


def test_refusals_on_a_live_processor_in_order(wm):
    from webaudio_modem_amd import _lib
    L = _lib.lib()
    S = 5
    engs, (a, b) = twins(wm, S, wm.PRECISION_F32)
    buf = np.zeros(256, np.uint8)
    B = buf.ctypes.data
    before = a.snapshot()
    name = "fskhip_processor_process_fmt_host"
    for args, text in (((B + 1, 4, 2, 8, 0, B + 1, -1, 7, 8, 0), name + ": unknown sample format 4"),
                       ((B + 1, 1, 1, 8, 0, B + 1, 3, -1, 8, 0), name + ": unknown layout -1"),
                       ((B + 1, 1, 0, 8, 7, B + 1, 1, 0, 8, 7), "in_pitch 7 < n_in 8"),
                       ((B + 1, 2, 1, 8, S - 1, B + 1, 1, 0, 8, 7), "in frame pitch 4 < n_streams 5"),
                       ((B + 2, 1, 1, 8, S, B + 1, 3, 1, 8, S - 1), "out frame pitch 4 < n_streams 5"),
                       ((B + 1, 1, 0, 8, 8, B + 1, 1, 0, 8, 8), "in is not aligned to its element size"),
                       ((B + 2, 1, 1, 8, S, B + 2, 0, 1, 8, S), "out is not aligned to its element size")):
        assert (L.fskhip_processor_process_fmt_host(a._h, *args, 0), L.fskhip_last_error().decode()) == (-1, text)
    assert a.snapshot() == before
    # zero lengths and NULL sides are legal
    assert a.process_samples(None) is None
    assert a.process_samples(np.zeros((0, S), np.uint8), "mulaw", "sample") is None
    assert a.process_samples(np.zeros((S, 0), np.int16), "s16", "stream", 0, "alaw", "sample") is None
    close(engs, (a, b))


def test_xmodem_file_crosses_as_mulaw_frames(wm):
    """an XModemSenderBatch and an XModemReceiverBatch on two processors, every sample between them a mu-law interleaved frame that
    one process_samples produced and the other consumes; the file of three fragments arrives intact"""
    import xmodem_tx_ref as ref
    from oracle import next_oracle as no
    S, max_payload, Q = 2, 16, 1024
    rng = np.random.default_rng(0x3F11E)
    files = [bytes(rng.integers(0, 256, 40, dtype=np.uint8)) for _ in range(S)]
    assert len(ref.fragments(files[0], max_payload)) == 3
    engs = [wm.FSKEngine(S, XCFG, precision=wm.PRECISION_F32) for _ in range(2)]
    A, B = (wm.FSKProcessorBatch(e, rx_capacity=1024, clear_rx_on_tx_complete=True) for e in engs)
    tx, rx = wm.XModemSenderBatch(A, max_payload), wm.XModemReceiverBatch(B)
    tx.send(files)
    B.modulate([bytes([ref.NAK])] * S)
    got, done, ended = [b""] * S, np.zeros(S, bool), {}
    owed = [[] for _ in range(S)]
    a_out = b_out = np.full((Q, S), sr.silence("mulaw"), np.uint8)
    for quantum in range(400):
        a_next = A.process_samples(b_out, "mulaw", "sample", Q, "mulaw", "sample")
        b_next = B.process_samples(a_out, "mulaw", "sample", Q, "mulaw", "sample")
        assert a_next.dtype == np.uint8 and a_next.shape == (Q, S)
        a_out, b_out = a_next, b_next
        if quantum % 2 == 1:
            for s, ev in tx.poll_active().items():
                if ev["status"] != ref.PROGRESS:
                    ended[s] = ev["status"]
            for s, (res, data) in rx.poll_active(mask=~done).items():
                got[s] += data
                assert res["status"] not in (no.XM_INVALID_SEQUENCE, no.XM_INVALID_CRC, no.XM_UNEXPECTED_SEQUENCE), (s, res)
                owed[s] += [ref.ACK] * (res["packets"] + res["dropped"])
                if res["status"] == no.XM_EOT:
                    owed[s].append(ref.ACK)
                    done[s] = True
            free = ~B.tx_state()["pendingModulation"]
            go = np.array([bool(owed[s]) and free[s] for s in range(S)])
            if go.any():
                B.modulate([bytes([owed[s].pop(0)]) if go[s] else b"" for s in range(S)], mask=go)
        if len(ended) == S:
            break
    assert len(ended) == S and set(ended.values()) == {ref.DONE}, (ended, quantum)
    assert got == files
    tx.close()
    rx.close()
    close(engs, (A, B))
