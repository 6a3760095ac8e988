"""fskhip_processor_process_ratecvt_* on the GPU (include/fskhip_next.h; FSKProcessorBatch.process_samples_at with a CaptureConverter
and a PlaybackConverter): one FSKProcessor quantum with both sides at the converters' outer rate.  Every comparison is bit for bit,
with no tolerance anywhere, against the chain of the existing calls on a twin processor with twin handles --
CaptureConverter.process -> process() -> PlaybackConverter.process -- never against the code under test: the elements returned,
tx_state(), the ring lengths and the drained rings, both handles' histories and the snapshot images of processor and engine,
after every quantum.  70 streams are one whole wave of the fused TX kernel and a tail of 6 lanes.

The shapes are small on purpose: ratios 3 / 2 and 2 / 3 with 7 and 8 taps have several outputs per engine sample, histories of 2
to 4 samples and periods of fewer engine samples than the history; 147 / 160 with the default 2 561 taps is what the call is for."""
import numpy as np
import pytest

import samples_ref as sr

pytestmark = pytest.mark.gpu

CFG = {}                                   # the reference's defaults: 48 kHz, 1200 baud, 40 samples per bit
# what a quantum's output is asked in, by turns: all four formats stream-major (the fused kernel), two as frames (the pair)
SHAPES = [("f32", "stream"), ("s16", "sample"), ("mulaw", "stream"), ("s16", "stream"), ("mulaw", "sample"), ("alaw", "stream")]
TAPS = {7: [0.09, -0.21, 0.48, 0.55, 0.31, -0.17, 0.05], 8: [0.07, -0.19, 0.41, 0.52, 0.36, 0.13, -0.15, 0.04]}
# the playback side's up / down; the capture side is its inverse, so both sides of the engine run at one outer rate
RATIOS = {"3/2": (3, 2), "2/3": (2, 3), "147/160": (147, 160), "160/147": (160, 147)}


@pytest.fixture(scope="module")
def wm():
    import __graft_entry__ as ge
    ge.build()
    import webaudio_modem_amd as wm
    return wm


def twins(wm, S, precision, clear=True, n=2):
    engs = [wm.FSKEngine(S, CFG, precision=getattr(wm, "PRECISION_" + precision)) for _ in range(n)]
    return engs, [wm.FSKProcessorBatch(e, rx_capacity=1024, clear_rx_on_tx_complete=clear) for e in engs]


def converters(wm, S, ratio, n_taps, precision, n=2):
    """n capture and n playback converters of one design: playback by up / down = RATIOS[ratio], capture by down / up; n_taps None:
    the default designs"""
    up, down = RATIOS[ratio]
    prec = getattr(wm, "PRECISION_" + precision)
    taps = None if n_taps is None else TAPS[n_taps]
    cap_taps = None if taps is None else [float(down) * t for t in reversed(taps)]
    caps = [wm.CaptureConverter(up, down, S, taps=cap_taps, precision=prec) for _ in range(n)]
    plays = [wm.PlaybackConverter(down, up, S, taps=taps, precision=prec) for _ in range(n)]
    assert (caps[0].up, caps[0].down, plays[0].up, plays[0].down) == (down, up, up, down)
    return caps, plays


def close(*things):
    for x in things:
        x.close()


def payloads(S, seed):
    """ragged payloads of 1..3 bytes; every fifth stream idle"""
    rng = np.random.default_rng(seed)
    return [b"" if s % 5 == 4 else bytes(rng.integers(0, 256, 1 + (s + seed) % 3, dtype=np.uint8)) for s in range(S)]


def chain(ref, cap, play, inputs, in_fmt, in_layout, n_out, out_fmt, out_layout):
    """one quantum through the three existing calls"""
    x = None if inputs is None else cap.process(inputs, in_fmt, in_layout)
    y = ref.process(x, n_out // play.up * play.down if n_out else 0)
    return play.process(y, out_fmt, out_layout) if n_out else None


def assert_same(ref, dut, caps, plays, where, engine=True):
    a, b = ref.tx_state(), dut.tx_state()
    assert all(np.array_equal(a[k], b[k]) for k in a), where
    assert np.array_equal(ref.rx_lengths(), dut.rx_lengths()), where
    assert caps[0].state().tobytes() == caps[1].state().tobytes(), where
    assert plays[0].state().tobytes() == plays[1].state().tobytes(), where
    sa, sb = ref.snapshot(), dut.snapshot()
    assert sa.processor == sb.processor, where
    if engine:
        assert sa.engine == sb.engine, where


def equal_after_every_quantum(wm, S, eprec, cprec, ratio, n_taps, periods, clear):
    """Both sides in every call, the output of one quantum the input of the next: a modulation starts; a second is started behind a
    reset while the first still sounds; it ends inside a quantum; a third starts in the quantum after that; it ends; then an RX-only,
    a TX-only and an empty quantum, and silence.  Formats and layouts take turns."""
    engs, (ref, dut) = twins(wm, S, eprec, clear)
    caps, plays = converters(wm, S, ratio, n_taps, cprec)
    up, down = RATIOS[ratio]
    assert caps[0].history == -(-(len(caps[0].taps) - 1) // down) and plays[0].history == -(-(len(plays[0].taps) - 1) // up)
    for p in (ref, dut):
        p.modulate(payloads(S, 1))
    k, stage, tail, wire, wire_shape, seen = 0, 0, 0, None, None, set()
    while True:
        assert k < 400
        n = periods[k % len(periods)]
        fmt, layout = SHAPES[k % len(SHAPES)]
        inputs, n_out = wire, n * up
        if stage == 3:                                  # one side only, then neither
            inputs, n_out = ((wire, 0), (None, n * up), (np.zeros((0, S), np.uint8), 0))[min(tail, 3) - 1] if 1 <= tail <= 3 else (wire, n * up)
        in_fmt, in_layout = wire_shape if inputs is wire and wire is not None else ("mulaw", "sample")
        want = chain(ref, caps[0], plays[0], inputs, in_fmt, in_layout, n_out, fmt, layout)
        got = dut.process_samples_at(inputs, in_fmt, in_layout, caps[1], n_out, fmt, layout, plays[1])
        where = (k, n, in_fmt, in_layout, fmt, layout, stage, tail)
        if n_out:
            assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), (where, np.argwhere(got != want)[:4])
            wire, wire_shape = want, (fmt, layout)
            if n * down < plays[0].history:
                seen.add("short")                       # fewer engine samples than the history: old history survives
        else:
            assert got is None and want is None, where
        assert_same(ref, dut, caps, plays, where)
        if k % 4 == 3:
            assert ref.demodulate() == dut.demodulate(), where
        k += 1
        if stage == 0 and k == 4:                       # mid-tone: cancel, and start the next while the filter still rings
            for p in (ref, dut):
                p.reset()
                p.modulate(payloads(S, 2))
            assert np.abs(plays[0].state()).max() > 0.01
            stage = 1
        elif stage == 1 and not ref.tx_state()["isModulating"].any():
            free = ~ref.tx_state()["pendingModulation"]
            assert free.any()
            for p in (ref, dut):
                p.modulate(payloads(S, 3), mask=free)
            stage = 2
        elif stage == 2 and not ref.tx_state()["isModulating"].any():
            stage = 3
        elif stage == 3:
            tail += 1
            if tail >= 4 + len(SHAPES):
                break
    assert ref.tx_state()["completed"].max() == 2
    assert ref.demodulate() == dut.demodulate()
    assert ref.processDemodulationCallCount == dut.processDemodulationCallCount
    close(*caps, *plays, ref, dut, *engs)
    return seen


SMALL = [(70, e, c, r, t) for r in ("3/2", "2/3") for t in (7, 8) for e, c in (("F32", "F32"), ("F64", "F64"))] + [(1, "F32", "F64", "3/2", 8), (1, "F64", "F32", "2/3", 7)]


@pytest.mark.parametrize("S,eprec,cprec,ratio,n_taps", SMALL, ids=["%d-%s-%s-%s-%dtaps" % c for c in SMALL])
def test_small_ratios_equal_the_chain_after_every_quantum(wm, S, eprec, cprec, ratio, n_taps):
    up, down = RATIOS[ratio]
    seen = equal_after_every_quantum(wm, S, eprec, cprec, ratio, n_taps, (1, 90, 3, 64, 1, 33, 120), clear=True)
    H = -(-(n_taps - 1) // up)
    assert ("short" in seen) == (down < H)
    if n_taps == 8:
        assert "short" in seen                          # 3 / 2: 2 engine samples against a history of 3; 2 / 3: 3 against 4


DEFAULT = [(70, "F32", "F32", "147/160", True), (70, "F64", "F64", "147/160", False), (70, "F32", "F32", "160/147", False), (1, "F64", "F32", "147/160", True)]


@pytest.mark.parametrize("S,eprec,cprec,ratio,clear", DEFAULT, ids=["%d-%s-%s-%s-clear%d" % c for c in DEFAULT])
def test_default_designs_equal_the_chain_after_every_quantum(wm, S, eprec, cprec, ratio, clear):
    """44.1 kHz either side of the engine (and the ratio the other way round), the default 2 561 taps, quanta of one and three
    periods, with and without the RX clear when a modulation completes"""
    equal_after_every_quantum(wm, S, eprec, cprec, ratio, None, (1, 3, 3, 1, 3), clear)


@pytest.fixture(scope="module")
def wire441(wm):
    """70 streams of 44.1 kHz mu-law, [70, 24 * 147], from the existing calls alone: stream s sends a payload of its own behind a lead
    of its own.  Made once and left unchanged."""
    S = 70
    eng = wm.FSKEngine(S, CFG, precision=wm.PRECISION_F32)
    proc = wm.FSKProcessorBatch(eng)
    play = wm.PlaybackConverter(48000, 44100, S)
    proc.modulate([bytes([0x41 + s % 26, s]) for s in range(S)])
    x = proc.process(None, 24 * 160)
    for s in range(S):
        x[s] = np.roll(x[s], 11 * (s % 7))              # (the frame is 2 400 samples: what rolls round is silence)
    out = play.process(x, "mulaw", "stream")
    close(play, proc, eng)
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("ratio,n_taps", (("147/160", None), ("3/2", 8)))
def test_any_cut_into_whole_periods_gives_the_same(wm, wire441, ratio, n_taps):
    """the same 12 periods as one quantum, as 12 quanta and as 5 + 7: the same samples, bytes and final state (without the RX clear on
    completion, which clears what the completing call has put: more in a longer call)"""
    S = 70
    up, down = RATIOS[ratio]
    unit = 1 if n_taps is None else 40      # (periods of 3 / 2 are 2 engine samples: 40 at a time, so that the cuts reach past the frame's leading zeros)
    cuts = {"one": [12 * unit], "twelve": [unit] * 12, "5+7": [5 * unit, 7 * unit]}
    engs, procs = twins(wm, S, "F32", clear=False, n=3)
    caps, plays = converters(wm, S, ratio, n_taps, "F32", n=3)
    x = np.ascontiguousarray(wire441[:, 4 * 147:4 * 147 + 12 * unit * up])      # (the capture side takes `up` samples per period)
    results = {}
    for (name, cut), p, cap, play in zip(cuts.items(), procs, caps, plays):
        p.modulate(payloads(S, 5))
        outs, pos = [], 0
        for n in cut:
            outs.append(p.process_samples_at(x[:, pos * up:(pos + n) * up], "mulaw", "stream", cap, n * up, "s16", "stream", play))
            pos += n
        tx = p.tx_state()
        status = [{k: v for k, v in p.status(s).items() if k not in ("demodulationCalls", "processDemodulationCallCount")} for s in (0, 33, S - 1)]
        results[name] = (np.concatenate(outs, axis=1).tobytes(), cap.state().tobytes(), play.state().tobytes(), p.snapshot().processor,
                         {k: tx[k].tobytes() for k in tx}, status, p.demodulate())
    assert results["twelve"] == results["one"] and results["5+7"] == results["one"]
    assert np.frombuffer(results["one"][0], np.int16).any()
    close(*caps, *plays, *procs, *engs)


def test_with_a_factor_of_one_it_is_the_resampler_call(wm, wire441):
    """down = 1 makes the capture side Upsampler(L), up = 1 the playback side Downsampler(M): process_samples_at through the
    converters equals process_samples_at through the resamplers, bit for bit, histories included"""
    S, F = 70, 6
    engs, (a, b) = twins(wm, S, "F32")
    up_r, down_r = wm.Upsampler(F, S), wm.Downsampler(F, S)
    cap, play = wm.CaptureConverter(1, F, S, taps=up_r.taps), wm.PlaybackConverter(F, 1, S, taps=down_r.taps)
    assert (cap.up, cap.down, play.up, play.down) == (F, 1, 1, F) and cap.history == up_r.history and play.history == down_r.history
    for p in (a, b):
        p.modulate(payloads(S, 7))
    pos = 0
    for k, n in enumerate((160, 37, 3, 1, 160, 80, 160, 41)):
        fmt, layout = SHAPES[k % len(SHAPES)]
        x = np.ascontiguousarray(wire441[:, pos:pos + n].T)
        want = a.process_samples_at(x, "mulaw", "sample", up_r, n, fmt, layout, down_r)
        got = b.process_samples_at(x, "mulaw", "sample", cap, n, fmt, layout, play)
        assert got.tobytes() == want.tobytes(), (k, n, fmt, layout)
        assert_same(a, b, (up_r, cap), (down_r, play), (k, n, fmt, layout))
        pos += n
    assert a.demodulate() == b.demodulate()
    close(up_r, down_r, cap, play, a, b, *engs)


def test_a_filter_beyond_the_delay_line_takes_the_two_launches(wm):
    """up = 1 with 4 096 taps is a history of 4 095 samples per stream, far beyond the fused kernel's delay line: the chain's result,
    stream-major too"""
    S = 3
    rng = np.random.default_rng(4096)
    taps = (rng.uniform(-1, 1, 4096) / 64).tolist()
    engs, (ref, dut) = twins(wm, S, "F32")
    caps = [wm.CaptureConverter(1, 2, S, taps=TAPS[7]) for _ in range(2)]
    plays = [wm.PlaybackConverter(2, 1, S, taps=taps) for _ in range(2)]
    assert plays[0].history == 4095
    for p in (ref, dut):
        p.modulate(payloads(S, 9))
    wire, wire_fmt = None, "s16"
    for k, n in enumerate((160, 1, 37, 480, 3, 800, 160)):
        fmt = ("s16", "mulaw", "f32", "alaw")[k % 4]
        want = chain(ref, caps[0], plays[0], wire, wire_fmt, "stream", n, fmt, "stream")
        got = dut.process_samples_at(wire, wire_fmt, "stream", caps[1], n, fmt, "stream", plays[1])
        assert got.tobytes() == want.tobytes(), (k, n, fmt)
        assert_same(ref, dut, caps, plays, (k, n, fmt))
        wire, wire_fmt = (None, fmt) if k % 2 else (want, fmt)
    assert np.abs(plays[0].state()).max() > 0
    close(*caps, *plays, ref, dut, *engs)


def live(wm, S=5):
    """a processor in the middle of a modulation with handles whose histories are not zero, and handles of 4 streams beside them"""
    engs, (a, b) = twins(wm, S, "F32")
    (cap,), (play,) = converters(wm, S, "3/2", 8, "F32", n=1)
    (cap4,), (play4,) = converters(wm, 4, "3/2", 8, "F32", n=1)
    a.modulate([b"x"] * S)
    a.process_samples_at(np.full((300, S), 0x31, np.uint8), upsampler=cap, n_out=300, downsampler=play)      # (200 engine samples: past the frame's leading zeros)
    return engs, a, b, cap, play, cap4, play4


def test_refusals_on_live_handles_in_order(wm):
    from webaudio_modem_amd import _lib
    L = _lib.lib()
    S = 5
    engs, a, b, cap, play, cap4, play4 = live(wm, S)
    before, hist = a.snapshot(), (cap.state().tobytes(), play.state().tobytes())
    assert any(hist[0]) and any(hist[1])
    buf = np.zeros(256, np.uint8)
    B = buf.ctypes.data
    U, D, U4, D4 = cap._h, play._h, cap4._h, play4._h          # capture: up 2, down 3; playback: up 3, down 2
    for name in ("fskhip_processor_process_ratecvt_host", "fskhip_processor_process_ratecvt_device"):
        fn, tail = getattr(L, name), ((None,) if name.endswith("device") else ())
        i, o = ("d_in", "d_out") if name.endswith("device") else ("in", "out")
        for (hu, hd), args, text in (
                ((U, D), (B + 1, 4, 2, 9, 0, B + 1, -1, 7, 9, 0), name + ": unknown sample format 4"),
                # the handles of the sides that have a buffer, input first: null, direction, streams
                ((None, None), (B + 1, 1, 0, 9, 7, B + 1, 1, 0, 9, 7), name + ": null capture handle"),
                ((D, None), (B + 1, 1, 0, 9, 7, B + 1, 1, 0, 9, 7), name + ": the capture handle converts for playback"),
                ((U4, None), (B + 1, 1, 0, 9, 7, B + 1, 1, 0, 9, 7), name + ": the capture handle has 4 streams, the processor 5"),
                ((U, None), (B + 1, 1, 0, 9, 7, B + 1, 1, 0, 9, 7), name + ": null playback handle"),
                ((None, U), (None, 1, 0, 9, 7, B + 1, 1, 0, 9, 7), name + ": the playback handle converts for capture"),
                ((U, D4), (B + 1, 1, 0, 9, 7, B + 1, 1, 0, 9, 7), name + ": the playback handle has 4 streams, the processor 5"),
                # pitches, in before out, before the multiples
                ((U, D), (B + 1, 1, 0, 8, 7, B + 1, 1, 0, 8, 7), "in_pitch 7 < n_in 8"),
                ((U, D), (B + 1, 2, 1, 8, S - 1, B + 1, 1, 0, 8, 7), "in frame pitch 4 < n_streams 5"),
                ((None, D), (None, 1, 0, 8, 7, B + 1, 1, 0, 8, 7), "out_pitch 7 < n_out 8"),
                ((U, D), (B + 2, 1, 1, 8, S, B + 1, 3, 1, 8, S - 1), "out frame pitch 4 < n_streams 5"),
                # alignment, in before out
                ((U, D), (B + 1, 1, 0, 8, 8, B + 1, 1, 0, 8, 8), i + " is not aligned to its element size"),
                ((U, D), (B + 2, 1, 1, 8, S, B + 2, 0, 1, 8, S), o + " is not aligned to its element size"),
                # whole periods, in before out
                ((U, D), (B + 2, 1, 1, 8, S, B + 4, 0, 1, 8, S), name + ": n_in 8 is not a multiple of the capture handle's down factor 3"),
                ((U, D), (B + 2, 1, 1, 9, S, B + 4, 0, 1, 8, S), name + ": n_out 8 is not a multiple of the playback handle's up factor 3"),
                ((None, D), (None, 1, 1, 8, S, B + 4, 0, 1, 8, S), name + ": n_out 8 is not a multiple of the playback handle's up factor 3")):
            assert (fn(a._h, hu, hd, *args, 0, *tail), L.fskhip_last_error().decode()) == (-1, text)
    assert a.snapshot() == before and (cap.state().tobytes(), play.state().tobytes()) == hist and not buf.any()
    # zero lengths and NULL sides are legal, and a side without samples needs no handle
    assert a.process_samples_at(None) is None
    assert a.process_samples_at(np.zeros((0, S), np.uint8), upsampler=cap) is None
    assert (cap.state().tobytes(), play.state().tobytes()) == hist
    close(cap, play, cap4, play4, a, b, *engs)


def test_a_handle_on_another_device_is_refused(wm):
    from webaudio_modem_amd import _lib
    L = _lib.lib()
    if L.fskhip_device_count() < 2:
        pytest.skip("needs a second GPU: a handle on another device than the processor's")
    S = 5
    engs, a, b, cap, play, cap4, play4 = live(wm, S)
    far_cap, far_play = wm.CaptureConverter(3, 2, S, taps=TAPS[8], device=1), wm.PlaybackConverter(2, 3, S, taps=TAPS[8], device=1)
    before = a.snapshot()
    buf = np.zeros(64, np.uint8)
    B = buf.ctypes.data
    name = "fskhip_processor_process_ratecvt_host"
    for (hu, hd), text in (((far_cap._h, play._h), ": the capture handle is on device 1, the processor on 0"),
                           ((cap._h, far_play._h), ": the playback handle is on device 1, the processor on 0")):
        rc = L.fskhip_processor_process_ratecvt_host(a._h, hu, hd, B, 1, 0, 2, 1, B, 1, 0, 2, 1, 0)      # (pitches too small as well: the device comes first)
        assert (rc, L.fskhip_last_error().decode()) == (-1, name + text)
    with pytest.raises(ValueError, match="upsampler is on device 1, the batch on 0"):
        a.process_samples_at(np.zeros((3, S), np.uint8), upsampler=far_cap)
    assert a.snapshot() == before
    close(far_cap, far_play, cap, play, cap4, play4, a, b, *engs)


def test_loopback_at_44100_delivers_the_payload(wm):
    """two processors at the default configuration joined by 44.1 kHz mu-law frames in quanta of 441: what A sends arrives on B byte for
    byte, and is what the chain of the existing calls delivers over twin processors and handles"""
    S, Q = 70, 441
    payload = bytes(range(0x30, 0x3C))
    engs, (A, B, A2, B2) = twins(wm, S, "F32", n=4)
    caps = [wm.CaptureConverter(44100, 48000, S) for _ in range(2)]
    plays = [wm.PlaybackConverter(48000, 44100, S) for _ in range(2)]
    assert (plays[0].up, plays[0].down, len(plays[0].taps), plays[0].history) == (147, 160, 2561, 18)
    for p in (A, A2):
        p.modulate([payload] * S)
    total = int(A.tx_state()["totalSamples"][0])
    n_quanta = -(-(total + 2 * 2561 // 147 + 480) // 480)
    for q in range(n_quanta):
        frames = A.process_samples_at(None, n_out=Q, downsampler=plays[0])
        assert frames.shape == (Q, S) and frames.dtype == np.uint8
        assert B.process_samples_at(frames, upsampler=caps[0]) is None
        want = chain(A2, None, plays[1], None, None, None, Q, "mulaw", "sample")
        assert frames.tobytes() == want.tobytes(), q
        chain(B2, caps[1], None, want, "mulaw", "sample", 0, None, None)
    assert not A.tx_state()["pendingModulation"].any()
    got = B.demodulate()
    assert got == [payload] * S and got == B2.demodulate()
    close(*caps, *plays, A, B, A2, B2, *engs)
