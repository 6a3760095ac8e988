"""The fused any-length TX quantum on the GPU (include/fskhip_next.h: fskhip_processor_process_ratecvt_any_*,
fskhip_processor_last_tx_kernel; csrc/fsk_mod.hip: processor_io_ratecvt_kernel, ANY): stream-major quanta of any n_out from any
position of the playback handle take one launch, and FSKProcessorBatch.last_tx_kernel says so.  The yardstick is a twin processor
with a twin handle whose quanta FSKHIP_PROC_RATECVT_PAIR sends through the two launches the kernel replaces -- processor_io_kernel
into a float tile, then the converter's own any-length kernel: the elements written, every processor and engine state word (the
snapshot images), the handle's history rows and its position are compared bit for bit after every quantum, and the two names.  fp64
handles are also held to the model (tests/ratecvt_any_ref.py) on the generator's floats.  Then FSKEngine.demodulate_samples_at /
modulate_samples_at with any_length=True against the chain of the device calls they stand for, and a frame looped back byte for
byte at 44.1 kHz in 128-frame quanta over the fused kernel."""
import numpy as np
import pytest

import ratecvt_any_ref as ra
import samples_ref as sr

pytestmark = pytest.mark.gpu

BELL = {}
FUSED_ANY, FUSED = "processor_io_ratecvt_kernel<any>", "processor_io_ratecvt_kernel"
PAIR_ANY, PAIR = "processor_io_kernel+ratecvt_playback_any_kernel", "processor_io_kernel+ratecvt_playback_kernel"
QUANTA = (128, 1, 129, 147, 2, 128)
FORMATS = ("f32", "s16", "mulaw", "alaw")
BITS = {"f32": np.uint32, "s16": np.uint16, "mulaw": np.uint8, "alaw": np.uint8}


@pytest.fixture(scope="module")
def wm():
    import __graft_entry__ as ge
    ge.build()
    import webaudio_modem_amd as wm
    return wm


class Twins:
    """a processor whose TX side takes the call's own choice, and one forced through the pair, each with its playback handle"""

    def __init__(self, wm, S, up_rate=48000, down_rate=44100, taps=None, precision=None, position=0, history_seed=None):
        from webaudio_modem_amd import _lib
        prec = wm.PRECISION_F32 if precision is None else precision
        self.S = S
        self.engs = [wm.FSKEngine(S, BELL) for _ in range(2)]
        self.dut, self.ref = (wm.FSKProcessorBatch(e, clear_rx_on_tx_complete=False) for e in self.engs)
        self.ref.flags |= _lib.PROC_RATECVT_PAIR
        self.plays = [wm.PlaybackConverter(up_rate, down_rate, S, taps=taps, precision=prec) for _ in range(2)]
        if history_seed is not None:
            st = np.random.default_rng(history_seed).uniform(-0.5, 0.5, (S, self.plays[0].history)).astype(np.float32)
            for p in self.plays:
                p.set_state(st)
        for p in self.plays:
            p.position = position

    def modulate(self, payloads):
        for p in (self.dut, self.ref):
            p.modulate(payloads)

    def quantum(self, n_out, fmt, layout="stream", where=None):
        got = self.dut.process_samples_at_any(None, n_out=n_out, out_fmt=fmt, out_layout=layout, downsampler=self.plays[0])
        want = self.ref.process_samples_at_any(None, n_out=n_out, out_fmt=fmt, out_layout=layout, downsampler=self.plays[1])
        assert got.dtype == want.dtype and got.shape == want.shape == ((self.S, n_out) if layout == "stream" else (n_out, self.S)), where
        assert got.tobytes() == want.tobytes(), (where, np.argwhere(got.view(BITS[fmt]) != want.view(BITS[fmt]))[:4])
        self.same_state(where)
        return got

    def same_state(self, where):
        a, b = self.dut.snapshot(), self.ref.snapshot()
        assert a.processor == b.processor and a.engine == b.engine, where
        ta, tb = self.dut.tx_state(), self.ref.tx_state()
        assert all(np.array_equal(ta[k], tb[k]) for k in ta), where
        assert self.plays[0].state().tobytes() == self.plays[1].state().tobytes(), where
        assert self.plays[0].position == self.plays[1].position, where

    def close(self):
        for x in (*self.plays, self.dut, self.ref, *self.engs):
            x.close()


def payloads_for(S, seed, longest=3):
    rng = np.random.default_rng(seed)
    return [bytes(rng.integers(0, 256, 1 + s % longest, dtype=np.uint8)) for s in range(S)]


def run_quanta(t, fmt, n_quanta, seed):
    """QUANTA over and over on a pending modulation that starts, completes and starts again within the run"""
    t.modulate(payloads_for(t.S, seed))
    restarted, positions = False, set()
    for k in range(n_quanta):
        n_out = QUANTA[k % len(QUANTA)]
        whole = t.plays[0].position == 0 and n_out % t.plays[0].up == 0 and t.plays[0].in_count_any(n_out) == n_out // t.plays[0].up * t.plays[0].down
        t.quantum(n_out, fmt, where=(fmt, k, n_out))
        assert t.dut.last_tx_kernel == (FUSED if whole else FUSED_ANY), (k, t.dut.last_tx_kernel)
        assert t.ref.last_tx_kernel == (PAIR if whole else PAIR_ANY), (k, t.ref.last_tx_kernel)
        positions.add(t.plays[0].position)
        if not restarted and not t.dut.tx_state()["pendingModulation"].any():
            t.modulate(payloads_for(t.S, seed + 1, longest=2))
            restarted = True
    done = t.dut.tx_state()["completed"]
    assert restarted and (done >= 1).all(), done
    return positions


@pytest.mark.parametrize("S", [70, 131])
@pytest.mark.parametrize("fmt", FORMATS)
def test_quanta_of_any_length_take_the_fused_kernel_and_equal_the_pair(wm, S, fmt):
    """70 streams: one wave and a 6-lane tail; 131: three workgroups.  Bell 202, the default 147 / 160 design."""
    t = Twins(wm, S)
    try:
        assert t.dut.last_tx_kernel == "" == t.ref.last_tx_kernel
        positions = run_quanta(t, fmt, 150, seed=S)
        assert len(positions) > 20
    finally:
        t.close()


@pytest.mark.parametrize("position", [1, 73, 159])
def test_quanta_from_a_handle_set_to_a_position_with_a_history(wm, position):
    for fmt in ("s16", "mulaw"):
        t = Twins(wm, 70, position=position, history_seed=position)
        try:
            assert t.plays[0].position == position and np.abs(t.plays[0].state()).max() > 0.1
            run_quanta(t, fmt, 150, seed=position)
        finally:
            t.close()


def test_quanta_shorter_than_the_history_keep_the_old_history(wm):
    """n_high < H: 40 quanta of one output take one or two engine samples each against a history of 18; the history row afterwards
    is the old one rolled by the generator's samples, which a third processor writes as floats"""
    S = 70
    t = Twins(wm, S, position=73, history_seed=7)
    gen_eng = wm.FSKEngine(S, BELL)
    gen = wm.FSKProcessorBatch(gen_eng, clear_rx_on_tx_complete=False)
    try:
        pay = payloads_for(S, 40)
        t.modulate(pay)
        gen.modulate(pay)
        H = t.plays[0].history
        assert H == 18
        line = t.plays[0].state().copy()
        took = 0
        for k in range(40):
            n_high = t.plays[0].in_count_any(1)
            assert 1 <= n_high < H
            t.quantum(1, "s16", where=k)
            assert t.dut.last_tx_kernel == FUSED_ANY
            line = np.concatenate([line, gen.process(None, n_high)], axis=1)
            took += n_high
            assert t.plays[0].state().tobytes() == line[:, -H:].tobytes(), k
        assert t.plays[0].position == (73 + took) % 160
    finally:
        gen.close()
        gen_eng.close()
        t.close()


CONVERTERS = [  # (engine rate, outer rate, taps): 3 / 2 with 7 and 31 taps, 1 / 6 with 97 taps, 6 / 1
    (2, 3, 7), (2, 3, 31), (6, 1, 97), (1, 6, 13)]


@pytest.mark.parametrize("rates", CONVERTERS)
def test_other_ratios_fp64_handles_and_the_model(wm, rates):
    """L > M, where one sample completes two outputs, L = 1 and M = 1, fp64 handles: the twin, and the model on the generator's
    floats; an n_out the handle cannot write from its position is refused in the existing words and changes nothing"""
    in_rate, out_rate, n_taps = rates
    S = 70
    taps = (np.hamming(n_taps) * np.sinc((np.arange(n_taps) - (n_taps - 1) / 2) / 3.0) * 0.4).tolist()
    t = Twins(wm, S, in_rate, out_rate, taps=taps, precision=wm.PRECISION_F64, history_seed=n_taps)
    gen_eng = wm.FSKEngine(S, BELL)
    gen = wm.FSKProcessorBatch(gen_eng, clear_rx_on_tx_complete=False)
    try:
        L, M = t.plays[0].up, t.plays[0].down
        assert (L, M) == wm.PlaybackConverter.ratio(in_rate, out_rate)
        pay = payloads_for(S, n_taps)
        t.modulate(pay)
        gen.modulate(pay)
        refused = ran = 0
        for k, n_out in enumerate((5, 1, 2, 3, 7, 4, 129, 6, 1, 12, 2, 33) * 3):
            fmt = FORMATS[k % 4]
            play = t.plays[0]
            pos, n_high = play.position, play.in_count_any(n_out)
            if play.out_count_any(n_high) != n_out:
                snap, st = t.dut.snapshot(), play.state()
                with pytest.raises(wm.FskHipError, match="the playback handle at position %d cannot write n_out %d: " % (pos, n_out)):
                    t.dut.process_samples_at_any(None, n_out=n_out, out_fmt=fmt, out_layout="stream", downsampler=play)
                after = t.dut.snapshot()
                assert (after.processor, after.engine) == (snap.processor, snap.engine) and play.state().tobytes() == st.tobytes() and play.position == pos
                refused += 1
                continue
            before = play.state()
            got = t.quantum(n_out, fmt, where=(rates, k, n_out))
            whole = pos == 0 and n_out % L == 0 and n_high == n_out // L * M
            assert t.dut.last_tx_kernel == (FUSED if whole else FUSED_ANY) and t.ref.last_tx_kernel == (PAIR if whole else PAIR_ANY), (k, n_out, pos)
            model, hist, nxt = ra.playback_any(gen.process(None, n_high), taps, L, M, fmt, pos=pos, hist=before)
            assert got.view(BITS[fmt]).tobytes() == np.asarray(model).view(BITS[fmt]).tobytes(), (rates, k, n_out, pos)
            assert play.state().tobytes() == hist.tobytes() and play.position == nxt
            ran += 1
        assert ran >= 6 and (refused > 0) == (L > M)
    finally:
        gen.close()
        gen_eng.close()
        t.close()


def test_frames_and_a_converter_beyond_the_delay_line_take_the_pair(wm):
    S = 70
    t = Twins(wm, S)
    try:
        t.modulate(payloads_for(S, 5))
        for k, n_out in enumerate((128, 1, 129, 147)):
            t.quantum(n_out, FORMATS[k], "sample", where=k)
            assert t.dut.last_tx_kernel == t.ref.last_tx_kernel == PAIR_ANY
        t.quantum(128, "s16", "stream")
        assert t.dut.last_tx_kernel == FUSED_ANY
        assert t.dut.process_samples_at_any(None, n_out=0, downsampler=t.plays[0]) is None and t.dut.last_tx_kernel == ""
    finally:
        t.close()
    long_taps = (np.hamming(4096) * 0.001).tolist()
    t = Twins(wm, S, 6, 1, taps=long_taps)       # up 1, down 6: a history of 4 095 samples per stream
    try:
        assert (t.plays[0].up, t.plays[0].down, t.plays[0].history) == (1, 6, 4095)
        t.modulate(payloads_for(S, 6))
        for k, n_out in enumerate((21, 1, 40)):
            t.quantum(n_out, "s16", "stream", where=k)
            assert t.dut.last_tx_kernel == t.ref.last_tx_kernel == PAIR_ANY
    finally:
        t.close()


def test_whole_periods_from_position_0(wm):
    """Whole periods of output that are whole periods of engine samples too (up > down: 3 / 2) run the whole-period form through
    the any-length call, with process_samples_at's results and state.  For 147 / 160 the fewest engine samples that write 147
    outputs are 159, not 160, so that quantum is the any-length form's; its elements are still process_samples_at's."""
    S = 70
    taps = [0.09, -0.21, 0.48, 0.55, 0.31, -0.17, 0.05]
    engs = [wm.FSKEngine(S, BELL) for _ in range(2)]
    procs = [wm.FSKProcessorBatch(e, clear_rx_on_tx_complete=False) for e in engs]
    plays = [wm.PlaybackConverter(2, 3, S, taps=taps) for _ in range(2)]
    try:
        for p in procs:
            p.modulate(payloads_for(S, 9))
        for k in range(6):
            a = procs[0].process_samples_at_any(None, n_out=48, out_fmt="s16", out_layout="stream", downsampler=plays[0])
            b = procs[1].process_samples_at(None, n_out=48, out_fmt="s16", out_layout="stream", downsampler=plays[1])
            assert procs[0].last_tx_kernel == FUSED == procs[1].last_tx_kernel
            assert a.tobytes() == b.tobytes() and procs[0].snapshot().processor == procs[1].snapshot().processor
            assert plays[0].state().tobytes() == plays[1].state().tobytes() and plays[0].position == plays[1].position == 0
    finally:
        for x in (*plays, *procs, *engs):
            x.close()
    engs = [wm.FSKEngine(S, BELL) for _ in range(2)]
    procs = [wm.FSKProcessorBatch(e, clear_rx_on_tx_complete=False) for e in engs]
    plays = [wm.PlaybackConverter(48000, 44100, S) for _ in range(2)]
    try:
        for p in procs:
            p.modulate(payloads_for(S, 10))
        a = procs[0].process_samples_at_any(None, n_out=294, out_fmt="mulaw", out_layout="stream", downsampler=plays[0])
        b = procs[1].process_samples_at(None, n_out=294, out_fmt="mulaw", out_layout="stream", downsampler=plays[1])
        assert a.tobytes() == b.tobytes()
        assert (procs[0].last_tx_kernel, plays[0].position) == (FUSED_ANY, 319 % 160) and (procs[1].last_tx_kernel, plays[1].position) == (FUSED, 0)
    finally:
        for x in (*plays, *procs, *engs):
            x.close()


@pytest.mark.parametrize("fmt,layout", [("s16", "stream"), ("mulaw", "stream"), ("s16", "sample"), ("mulaw", "sample")])
def test_engine_demodulates_a_capture_of_any_length(wm, fmt, layout):
    """44 100 + 5 samples per stream in calls of 128, 441, 1 and the rest equal one process_any_device + demodulate_device chain on a
    twin: bytes, 'eod' counts, status, history and position"""
    S, N = 67, 44105
    tx = wm.FSKEngine(S, BELL)
    play = wm.PlaybackConverter(48000, 44100, S)
    engs = [wm.FSKEngine(S, BELL) for _ in range(2)]
    caps = [wm.CaptureConverter(44100, 48000, S) for _ in range(2)]
    try:
        pay = payloads_for(S, 44, longest=40)
        sig, _lens = tx.modulate_samples_at(pay, fmt, "stream", play, n_per_stream=N, any_length=True)
        assert sig.shape == (S, N)
        x = sig if layout == "stream" else np.ascontiguousarray(sig.T)
        cut = (lambda a, b: x[:, a:b]) if layout == "stream" else (lambda a, b: x[a:b])
        got, eod, at = [b""] * S, np.zeros(S, np.uint32), 0
        for n in (128, 441, 1, N - 570):
            out, e = engs[0].demodulate_samples_at(np.ascontiguousarray(cut(at, at + n)), fmt, layout, caps[0], any_length=True)
            got = [g + o for g, o in zip(got, out)]
            eod += e
            at += n
        assert at == N
        # the twin: one conversion of the whole capture on the device, one demodulate call
        e1, c1 = engs[1], caps[1]
        n_eng = c1.out_count_any(N)
        tpitch, opitch = (n_eng + 3) & ~3, e1.max_bytes(n_eng)
        xs = np.ascontiguousarray(x)
        d_src, d_tile, d_out, d_counts, d_eod = (e1.device_malloc(b) for b in (xs.nbytes, 4 * S * tpitch, S * opitch, 4 * S, 4 * S))
        e1.h2d(d_src, xs)
        assert c1.process_any_device(d_src, fmt, layout, N, xs.shape[1], d_tile, tpitch) == n_eng
        e1.demodulate_device(d_tile, n_eng, tpitch, d_out, opitch, d_counts, d_eod)
        e1.synchronize()
        out, counts, eod1 = np.zeros((S, opitch), np.uint8), np.zeros(S, np.uint32), np.zeros(S, np.uint32)
        for a, d in ((out, d_out), (counts, d_counts), (eod1, d_eod)):
            e1.d2h(a, d)
        for d in (d_src, d_tile, d_out, d_counts, d_eod):
            e1.device_free(d)
        want = [out[s, :counts[s]].tobytes() for s in range(S)]
        assert got == want == pay
        assert np.array_equal(eod, eod1)
        for s in (0, 1, S - 1):
            a, b = engs[0].get_status(s), e1.get_status(s)
            assert all(a[k] == b[k] for k in ("frameStarted", "globalSampleCounter", "receivedBitsLength", "syncDetections")), (s, a, b)
        assert caps[0].state().tobytes() == c1.state().tobytes() and caps[0].position == c1.position == N % 147
        # without the flag the call still wants whole periods
        with pytest.raises(ValueError, match="not a multiple of the converter's down factor 147"):
            engs[0].demodulate_samples_at(np.ascontiguousarray(cut(0, 148)), fmt, layout, caps[0])
    finally:
        for h in (tx, play, *engs, *caps):
            h.close()


@pytest.mark.parametrize("position", [0, 73])
def test_engine_modulates_any_count_from_any_position(wm, position):
    """modulate_samples_at(n_per_stream=1000, any_length=True) equals modulate_device -> process_any on a twin, lengths included
    (4 800 baud: the frames of one and two bytes, 520 and 560 engine samples, fit the 1 089 that 1 000 outputs take)"""
    S, n = 67, 1000
    engs = [wm.FSKEngine(S, {"baudRate": 4800}) for _ in range(2)]
    plays = [wm.PlaybackConverter(48000, 44100, S) for _ in range(2)]
    try:
        pay = payloads_for(S, 1000 + position, longest=2)
        st = np.random.default_rng(position).uniform(-0.25, 0.25, (S, plays[0].history)).astype(np.float32)
        for p in plays:
            p.set_state(st)
            p.position = position
        for fmt, layout in (("s16", "stream"), ("mulaw", "sample")):
            pos = plays[1].position
            got, lens = engs[0].modulate_samples_at(pay, fmt, layout, plays[0], n_per_stream=n, any_length=True)
            sigs = engs[1].modulate_data(pay)
            n_in = plays[1].in_count_any(n)
            x = np.zeros((S, n_in), np.float32)
            for s, sig in enumerate(sigs):
                x[s, :sig.size] = sig
            want = plays[1].process_any(x, fmt, layout, lens=np.array([sg.size for sg in sigs], np.uint32))
            assert got.shape == want.shape == ((S, n) if layout == "stream" else (n, S)) and got.tobytes() == want.tobytes(), (fmt, layout)
            first = ra.first_output(147, 160, pos)
            assert lens.tolist() == [min(((pos + sg.size - 1) * 147 + 2560) // 160 + 1 - first, n) for sg in sigs]
            rows = got if layout == "stream" else got.T
            for s in range(S):
                assert (rows[s, lens[s]:].view(BITS[fmt]) == np.asarray(sr.silence(fmt)).view(BITS[fmt])).all()
            assert plays[0].state().tobytes() == plays[1].state().tobytes() and plays[0].position == plays[1].position == (pos + n_in) % 160
        # n_per_stream left out, from wherever the handle now is: the outputs that the longest signal and its ringing reach from there
        pos = plays[1].position
        assert pos != 0
        sigs = engs[1].modulate_data(pay)
        longest = max(sg.size for sg in sigs)
        first = ra.first_output(147, 160, pos)
        n_default = ((pos + longest - 1) * 147 + 2560) // 160 + 1 - first
        got, lens = engs[0].modulate_samples_at(pay, "s16", "stream", plays[0], any_length=True)
        n_in = plays[1].in_count_any(n_default)
        assert n_in >= longest                                            # (the whole signal is in the call)
        x = np.zeros((S, n_in), np.float32)
        for s, sig in enumerate(sigs):
            x[s, :sig.size] = sig
        want = plays[1].process_any(x, "s16", "stream", lens=np.array([sg.size for sg in sigs], np.uint32))
        assert got.shape == want.shape == (S, n_default) and got.tobytes() == want.tobytes()
        assert lens.tolist() == [min(((pos + sg.size - 1) * 147 + 2560) // 160 + 1 - first, n_default) for sg in sigs] and int(lens.max()) == n_default
        assert plays[0].state().tobytes() == plays[1].state().tobytes() and plays[0].position == plays[1].position
    finally:
        for h in (*engs, *plays):
            h.close()


def test_engine_call_that_completes_no_engine_sample(wm):
    """A down-converting capture (1 / 6: 288 kHz in front of the 48 kHz engine) on a fresh engine whose first call writes no
    engine sample: one input at position 1.  The returns are empty and nothing is demodulated, the handle has taken the sample
    (history and position as process_any leaves a twin), and the calls that follow continue bit for bit: the bytes, 'eod' counts
    and status are those of process_any -> demodulate_data on the twin, call by call."""
    S = 67
    tx = wm.FSKEngine(S, BELL)
    engs = [wm.FSKEngine(S, BELL) for _ in range(2)]
    caps = [wm.CaptureConverter(6, 1, S, taps=[1.0 / 6] * 6) for _ in range(2)]
    try:
        assert (caps[0].up, caps[0].down, caps[0].history) == (1, 6, 5)
        pay = payloads_for(S, 288)
        sigs = tx.modulate_data(pay)
        n48 = max(sg.size for sg in sigs) + 2000
        x48 = np.zeros((S, n48), np.float32)
        for s, sg in enumerate(sigs):
            x48[s, 300:300 + sg.size] = sg
        x = np.repeat(sr.encode(x48, "s16"), 6, axis=1)                   # each engine sample held for six capture samples
        st = np.random.default_rng(6).uniform(-0.01, 0.01, (S, 5)).astype(np.float32)
        for c in caps:
            c.set_state(st)
            c.position = 1
        got, want, eod, eod1, at = [b""] * S, [b""] * S, np.zeros(S, np.uint32), np.zeros(S, np.uint32), 0
        for k, n in enumerate((1, 1, 1, 1, 1, 1, 127, x.shape[1] - 133)):
            chunk = np.ascontiguousarray(x[:, at:at + n])
            n_eng = caps[0].out_count_any(n)
            assert (n_eng == 0) == (k < 5)                                # inputs 1 .. 5 of the period complete nothing, input 6 does
            out, e = engs[0].demodulate_samples_at(chunk, "s16", "stream", caps[0], any_length=True)
            if n_eng == 0:
                assert out == [b""] * S and not e.any() and e.shape == (S,)
            floats = caps[1].process_any(chunk, "s16", "stream")
            assert floats.shape == (S, n_eng)
            if n_eng:
                o1, e1 = engs[1].demodulate_data(floats)
                want = [w + o for w, o in zip(want, o1)]
                eod1 += e1
            got = [g + o for g, o in zip(got, out)]
            eod += e
            at += n
            assert caps[0].state().tobytes() == caps[1].state().tobytes() and caps[0].position == caps[1].position == (1 + at) % 6, k
            assert engs[0].snapshot().tobytes() == engs[1].snapshot().tobytes(), k
        assert got == want and np.array_equal(eod, eod1) and sum(len(g) for g in got) > 0
        assert got == pay
    finally:
        for h in (tx, *engs, *caps):
            h.close()


def test_a_frame_loops_back_at_44100_in_quanta_of_128_over_the_fused_kernel(wm):
    S = 67
    eng = wm.FSKEngine(S, BELL)
    proc = wm.FSKProcessorBatch(eng, rx_capacity=1024, clear_rx_on_tx_complete=False)
    cap, play = wm.CaptureConverter(44100, 48000, S), wm.PlaybackConverter(48000, 44100, S)
    try:
        pay = payloads_for(S, 128)
        proc.modulate(pay)
        wire, k, tail = None, 0, 0
        while tail < 40:
            assert k < 400
            wire = proc.process_samples_at_any(wire, "s16", "stream", cap, 128, "s16", "stream", play)
            assert proc.last_tx_kernel == FUSED_ANY
            k += 1
            if not proc.tx_state()["isModulating"].any():
                tail += 1
        assert proc.demodulate() == pay
    finally:
        for x in (cap, play, proc, eng):
            x.close()
