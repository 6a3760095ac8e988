"""fskhip_processor_process_ratecvt_any_* on the GPU (include/fskhip_next.h: "Rate conversion in calls of any length";
FSKProcessorBatch.process_samples_at_any): FSKProcessor quanta of 128 frames in and out at 44.1 kHz, lengths 1 and 129 mixed in, on
67 streams.  Every comparison is bit for bit against the chain of the separate calls on a twin processor with twin handles --
CaptureConverter.process_any -> process() with the engine counts the handles give, a side without engine samples left out ->
PlaybackConverter.process_any -- never against the code under test: the elements returned, tx_state(), the ring lengths, both
handles' histories and positions and the snapshot images of processor and engine, after every quantum.  The quanta's output is the
next quantum's input, so the link is a loopback, and the frame sent comes back byte for byte.  An n_out that a 3 / 2 playback
handle cannot write from its position is refused and changes nothing."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

S = 67
SHAPES = [("s16", "sample"), ("mulaw", "sample"), ("f32", "stream"), ("alaw", "stream"), ("s16", "stream")]
LENGTHS = (128, 128, 1, 129, 128, 128, 129, 1)


@pytest.fixture(scope="module")
def wm():
    import __graft_entry__ as ge
    ge.build()
    import webaudio_modem_amd as wm
    return wm


def chain(ref, cap, play, inputs, in_fmt, in_layout, n_out, out_fmt, out_layout):
    """one quantum through the three separate calls"""
    x = None
    if inputs is not None:
        x = cap.process_any(inputs, in_fmt, in_layout)
        if x.shape[1] == 0:
            x = None                                                      # no engine samples: the processor has no input side
    y = ref.process(x, play.in_count_any(n_out) if n_out else 0)
    return play.process_any(y, out_fmt, out_layout) if n_out else None


def assert_same(ref, dut, caps, plays, where):
    a, b = ref.tx_state(), dut.tx_state()
    assert all(np.array_equal(a[k], b[k]) for k in a), where
    assert np.array_equal(ref.rx_lengths(), dut.rx_lengths()), where
    assert caps[0].state().tobytes() == caps[1].state().tobytes() and caps[0].position == caps[1].position, where
    assert plays[0].state().tobytes() == plays[1].state().tobytes() and plays[0].position == plays[1].position, where
    sa, sb = ref.snapshot(), dut.snapshot()
    assert sa.processor == sb.processor and sa.engine == sb.engine, where


@pytest.mark.parametrize("precision", ["F32", "F64"])
def test_quanta_of_128_frames_equal_the_chain_and_loop_a_frame_back(wm, precision):
    prec = getattr(wm, "PRECISION_" + precision)
    engs = [wm.FSKEngine(S, {}, precision=prec) for _ in range(2)]
    ref, dut = (wm.FSKProcessorBatch(e, rx_capacity=1024, clear_rx_on_tx_complete=False) for e in engs)
    caps = [wm.CaptureConverter(44100, 48000, S, precision=prec) for _ in range(2)]
    plays = [wm.PlaybackConverter(48000, 44100, S, precision=prec) for _ in range(2)]
    try:
        rng = np.random.default_rng(128)
        payloads = [bytes(rng.integers(0, 256, 1 + s % 3, dtype=np.uint8)) for s in range(S)]
        for p in (ref, dut):
            p.modulate(payloads)
        wire, wire_shape, k, tail, positions = None, None, 0, 0, set()
        while tail < 40:
            assert k < 400
            n_out = LENGTHS[k % len(LENGTHS)]
            fmt, layout = SHAPES[k % len(SHAPES)]
            in_fmt, in_layout = wire_shape if wire is not None else ("s16", "sample")
            want = chain(ref, caps[0], plays[0], wire, in_fmt, in_layout, n_out, fmt, layout)
            got = dut.process_samples_at_any(wire, in_fmt, in_layout, caps[1], n_out, fmt, layout, plays[1])
            where = (k, n_out, in_fmt, in_layout, fmt, layout)
            assert got.dtype == want.dtype and got.shape == want.shape == ((S, n_out) if layout == "stream" else (n_out, S)), where
            assert got.tobytes() == want.tobytes(), (where, np.argwhere(got != want)[:4])
            assert_same(ref, dut, caps, plays, where)
            positions.add((caps[1].position, plays[1].position))
            wire, wire_shape = want, (fmt, layout)
            k += 1
            if not ref.tx_state()["isModulating"].any():
                tail += 1                                                 # the converters' delay and the demodulator's behind the last sample
        assert len(positions) > 20                                        # (the quanta began all over the periods, not at boundaries)
        # one side only, either way, and neither: the handle of an absent side stays where it is
        for inputs, n_out in ((wire, 0), (None, 128), (None, 0)):
            in_fmt, in_layout = wire_shape
            want = chain(ref, caps[0], plays[0], inputs, in_fmt, in_layout, n_out, "s16", "sample")
            got = dut.process_samples_at_any(inputs, in_fmt, in_layout, caps[1], n_out, "s16", "sample", plays[1])
            assert (got is None and want is None) if not n_out else got.tobytes() == want.tobytes()
            assert_same(ref, dut, caps, plays, (inputs is None, n_out))
        # the frame sent came back across 44.1 kHz in quanta of 128, byte for byte
        back = dut.demodulate()
        assert back == ref.demodulate()
        assert back == payloads
    finally:
        for x in (*caps, *plays, ref, dut, *engs):
            x.close()


def test_an_n_out_the_playback_handle_cannot_write_is_refused(wm):
    from webaudio_modem_amd import _lib
    eng = wm.FSKEngine(S, {})
    proc = wm.FSKProcessorBatch(eng)
    play = wm.PlaybackConverter(2, 3, S, taps=[0.09, -0.21, 0.48, 0.55, 0.31, -0.17, 0.05])
    try:
        assert (play.up, play.down, play.position) == (3, 2, 0)
        # from position 0 one engine sample gives 2 outputs, two give 3, three give 5: 1 and 4 cannot be written
        assert [play.out_count_any(n) for n in (1, 2, 3)] == [2, 3, 5]
        snap, st = proc.snapshot(), play.state()
        for n_out, text in ((1, "cannot write n_out 1: 0 engine samples give 0, 1 give 2"), (4, "cannot write n_out 4: 2 engine samples give 3, 3 give 5")):
            with pytest.raises(wm.FskHipError, match="fskhip_processor_process_ratecvt_any_host: the playback handle at position 0 " + text) as ei:
                proc.process_samples_at_any(None, n_out=n_out, out_fmt="s16", out_layout="stream", downsampler=play)
            assert ei.value.code == _lib.E_INVALID
        after = proc.snapshot()
        assert (after.processor, after.engine) == (snap.processor, snap.engine) and np.array_equal(play.state(), st) and play.position == 0
        assert proc.process_samples_at_any(None, n_out=2, out_fmt="s16", out_layout="stream", downsampler=play).shape == (S, 2) and play.position == 1
        # from position 1 the next sample gives one output
        assert proc.process_samples_at_any(None, n_out=1, out_fmt="s16", out_layout="stream", downsampler=play).shape == (S, 1) and play.position == 0
    finally:
        play.close()
        proc.close()
        eng.close()
