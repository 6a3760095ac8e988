"""FSKProcessorBatchSharded on the GPU against its twin: one FSKProcessorBatch of the same 131 streams fed the same calls.  The
shards are 66 + 65 on devices [0, 0] and 44 + 44 + 43 on [0, 0, 0]: none a multiple of 64, one boundary inside what is a wave of
the twin.  Everything is compared bit for bit -- no tolerance: the shards run the twin's kernels on the twin's data.

The line is a loopback: a quantum's input is the output of the quantum before it, moved on by one stream, so the frames that a
third of the streams send (ragged payloads) end in their neighbours' rings.  Quanta are 128 samples with 1 and 129 mixed in.
Outputs, ring lengths, TX words, status(i) and the engine's state words are compared for every stream after every quantum.  The
runs are as short as the line allows: a frame of one to three bytes is 1 600 to 2 400 samples long and has to arrive before the
end for the rings to hold bytes, and the second modulation has to be under way."""
import numpy as np
import pytest

from test_gpu_remap import _state, _same_state

pytestmark = pytest.mark.gpu

S = 131
LENS = [128] * 4 + [1] + [128] * 6 + [129] + [128] * 10        # 22 quanta, 2 690 samples: the frames below are 1 600 .. 2 400 long
SECOND_AT = 15                                                 # the quantum in front of which the second modulation starts
SILENCE = {"f32": 0, "s16": 0, "mulaw": 0xFF}


@pytest.fixture(scope="module")
def wm():
    import __graft_entry__ as ge
    ge.build()
    import webaudio_modem_amd as wm
    return wm


def _payloads(seed, keep):
    r = np.random.default_rng(seed)
    return [bytes(r.integers(0, 256, 1 + (s // 3 + seed) % 3, dtype=np.uint8)) if keep(s) else b"" for s in range(S)], [bool(keep(s)) for s in range(S)]


def _engine_of(b, s):
    """(engine, local stream) of global stream s of a sharded batch or a single one"""
    if hasattr(b, "locate"):
        i, local = b.locate(s)
        return b.engines[i], local
    return b.engine, s


def _assert_same(ref, dut, where):
    assert np.array_equal(ref.rx_lengths(), dut.rx_lengths()), where
    a, b = ref.tx_state(), dut.tx_state()
    assert set(a) == set(b) and all(np.array_equal(a[k], b[k]) and np.asarray(a[k]).dtype == np.asarray(b[k]).dtype for k in a), where
    for s in range(S):
        assert ref.status(s) == dut.status(s), (where, s)
        assert _same_state(_state(*_engine_of(ref, s)), _state(*_engine_of(dut, s))), (where, s)


def _quantum(wm, batches, fmt, layout, x, n_out, q):
    """one quantum on every batch -- batches[0] is the twin --, frames into one caller-owned `out` between two guard columns;
    everything compared to the twin.  Returns the twin's output."""
    outs = []
    for b in batches:
        if fmt == "f32" and layout == "stream" and q % 2 == 0:
            outs.append(b.process(x, n_out))                                  # (the float form on even quanta, the format form on odd ones)
        elif layout == "stream" or not hasattr(b, "locate"):
            outs.append(b.process_samples(x, fmt, layout, n_out, fmt, layout))
        else:
            guard = np.full((n_out, S + 2), 0x5A, wm.engine._FORMAT_DTYPE[wm.SAMPLE_FORMATS[fmt]])
            got = b.process_samples(x, fmt, layout, n_out, fmt, layout, out=guard[:, 1:S + 1])
            assert np.shares_memory(got, guard) and (guard[:, 0] == 0x5A).all() and (guard[:, S + 1] == 0x5A).all(), q
            outs.append(got)
    for k, o in enumerate(outs[1:]):
        assert o.dtype == outs[0].dtype and o.shape == outs[0].shape and np.array_equal(o.view(np.uint8) if fmt != "f32" else o.view(np.uint32),
                                                                                        outs[0].view(np.uint8) if fmt != "f32" else outs[0].view(np.uint32)), (q, k)
        _assert_same(batches[0], batches[k + 1], (q, k))
    return outs[0]


def _line(wm, fmt, layout, n):
    shape = (S, n) if layout == "stream" else (n, S)
    return np.full(shape, SILENCE[fmt], wm.engine._FORMAT_DTYPE[wm.SAMPLE_FORMATS[fmt]])


def _drive(wm, batches, fmt, layout, lens, x=None, q0=0, second_at=SECOND_AT):
    """quanta lens[...] on every batch from input x (None: silence); a second modulation starts at quantum `second_at`.  Returns the
    input of the quantum that would come next."""
    x = _line(wm, fmt, layout, lens[0]) if x is None else x
    for q, n in enumerate(lens, q0):
        if q == 0:
            pay, mask = _payloads(1, lambda s: s % 3 == 0)
            for b in batches:
                b.modulate(pay, mask)
        if q == second_at:
            pay, mask = _payloads(2, lambda s: s % 3 == 1)
            for b in batches:
                b.modulate(pay, mask)
        out = _quantum(wm, batches, fmt, layout, x, n, q)
        x = np.ascontiguousarray(np.roll(out, 1, axis=0 if layout == "stream" else 1))
    return x


def _pair(wm, prec, devices):
    twin = wm.FSKProcessorBatch(wm.FSKEngine(S, {}, device=0, precision=prec), clear_rx_on_tx_complete=False)
    sh = wm.FSKProcessorBatchSharded(S, {}, devices=devices, precision=prec, clear_rx_on_tx_complete=False)
    return twin, sh


def _close(*batches):
    for b in batches:
        eng = getattr(b, "engine", None)
        b.close()
        if eng is not None:
            eng.close()


def _mid_frame(wm, twin):
    """what the images and the rebalancing must carry: a half-sent modulation and bytes in the rings"""
    st = twin.tx_state()
    assert np.count_nonzero(st["pendingModulation"] & (st["samplePosition"] > 0) & (st["samplePosition"] < st["totalSamples"])) >= 20
    assert np.count_nonzero(twin.rx_lengths()) >= 20


def _parity(wm, prec, fmt, layout, devices):
    twin, sh = _pair(wm, prec, devices)
    try:
        assert [c for _, c, _ in sh.shards] == ([66, 65] if len(devices) == 2 else [44, 44, 43])
        _drive(wm, [twin, sh], fmt, layout, LENS)
        _mid_frame(wm, twin)
        assert sh.processDemodulationCallCount == twin.processDemodulationCallCount == len(LENS)
        assert len(sh.last_tx_kernel) == len(devices) and set(sh.last_tx_kernel) == {twin.last_tx_kernel}
        _assert_same(twin, sh, "end")
        mask = [s % 5 != 2 for s in range(S)]
        a, b = twin.demodulate_sparse(mask=mask, min_len=3), sh.demodulate_sparse(mask=mask, min_len=3)
        assert len(a[0]) >= 5 and all(np.array_equal(u, v) and u.dtype == v.dtype for u, v in zip(a, b))
        assert np.array_equal(twin.rx_lengths(), sh.rx_lengths())
        assert twin.demodulate_active(min_len=1) == sh.demodulate_active(min_len=1)
        got = twin.demodulate()
        assert got == sh.demodulate() and not any(got)          # (the sparse drains took everything)
    finally:
        _close(twin, sh)


@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]], ids=["two-shards", "three-shards"])
@pytest.mark.parametrize("fmt,layout", [("f32", "stream"), ("s16", "sample"), ("mulaw", "sample")])
@pytest.mark.parametrize("prec", ["F32", "F64"])
def test_every_quantum_equals_the_twins(wm, prec, fmt, layout, devices):
    _parity(wm, getattr(wm, "PRECISION_" + prec), fmt, layout, devices)


@pytest.mark.parametrize("fmt,layout", [("f32", "stream"), ("s16", "sample"), ("mulaw", "sample")])
@pytest.mark.parametrize("prec", ["F32", "F64"])
def test_every_quantum_equals_the_twins_on_two_devices(wm, prec, fmt, layout):
    from webaudio_modem_amd import _lib
    if _lib.lib().fskhip_device_count() < 2:
        pytest.skip("needs two HIP devices: this box has one (the same path runs on devices [0, 0] above)")
    _parity(wm, getattr(wm, "PRECISION_" + prec), fmt, layout, [0, 1])


def test_a_full_demodulate_equals_the_twins(wm):
    twin, sh = _pair(wm, wm.PRECISION_F32, [0, 0])
    try:
        _drive(wm, [twin, sh], "f32", "stream", LENS)
        got = twin.demodulate()
        assert got == sh.demodulate() and sum(1 for g in got if g) >= 20
    finally:
        _close(twin, sh)


@pytest.mark.parametrize("prec", ["F32", "F64"])
def test_images_equal_the_twins_and_restore_either_way(wm, prec):
    twin, sh = _pair(wm, getattr(wm, "PRECISION_" + prec), [0, 0])
    single = sharded = None
    try:
        x = _drive(wm, [twin, sh], "s16", "sample", LENS)
        _mid_frame(wm, twin)
        a, b = twin.snapshot(), sh.snapshot()
        assert isinstance(b.processor, bytes) and isinstance(b.engine, bytes)
        assert b.processor == a.processor                       # byte for byte, the shards' differing payload capacities included
        assert len({wm.processor_snapshot_info(p.snapshot().processor)["n_streams"] for p in sh.processors}) == 2
        assert wm.snapshot_info(b.engine)["n_streams"] == S
        single = wm.FSKProcessorBatch.from_snapshot(b, clear_rx_on_tx_complete=False)                       # the sharded pair into one batch
        sharded = wm.FSKProcessorBatchSharded.from_snapshot(a, devices=[0, 0, 0], clear_rx_on_tx_complete=False)   # the twin's pair into three shards
        assert single.processDemodulationCallCount == sharded.processDemodulationCallCount == 0
        assert [c for _, c, _ in sharded.shards] == [44, 44, 43] and sharded.rx_capacity == twin.rx_capacity and sharded.precision == sh.precision
        single.processDemodulationCallCount = len(LENS)         # (status() reports the host counter; it is not part of an image)
        sharded.processDemodulationCallCount = len(LENS)
        for dut in (single, sharded):
            _assert_same(twin, dut, "restored")
            assert dut.snapshot().processor == a.processor
        _drive(wm, [twin, sh, single, sharded], "s16", "sample", [128, 129, 128], x=x, q0=len(LENS))
        for dut in (sh, single, sharded):
            _assert_same(twin, dut, "three quanta on")
        assert twin.demodulate() == single.demodulate() == sharded.demodulate()
    finally:
        _close(twin, sh, *[b for b in (single, sharded) if b is not None])


def _rebalance_map():
    r = np.random.default_rng(0x5EED)
    src = r.permutation(S)[:S - 34]
    m = np.concatenate([src, r.choice(src, 25, replace=False), -np.ones(9)]).astype(np.int64)   # 25 entries name a source a second time
    r.shuffle(m)
    live = m[m >= 0]
    assert len(m) == S and np.count_nonzero(m < 0) == 9 and len(live) - len(set(live.tolist())) == 25
    return m


@pytest.mark.parametrize("prec", ["F32", "F64"])
def test_rebalancing_mid_frame_equals_the_twins_remap(wm, prec):
    twin, sh = _pair(wm, getattr(wm, "PRECISION_" + prec), [0, 0])
    made = []
    try:
        x = _drive(wm, [twin, sh], "f32", "stream", LENS)
        _mid_frame(wm, twin)
        m = _rebalance_map()
        made.append(twin.remapped(m))
        made.append(sh.remapped(m, devices=[0, 0, 0]))
        made.append(sh.remapped(m, devices=[0]))
        assert [c for _, c, _ in made[1].shards] == [44, 44, 43] and [c for _, c, _ in made[2].shards] == [S]
        assert [b.processDemodulationCallCount for b in made] == [len(LENS)] * 3
        _assert_same(twin, sh, "the source is left as it was")
        for dut in made[1:]:
            _assert_same(made[0], dut, "remapped")
        x2 = np.ascontiguousarray(np.where((m >= 0)[:, None], x[np.maximum(m, 0)], 0).astype(np.float32))
        _drive(wm, made, "f32", "stream", [128, 1, 129], x=x2, q0=len(LENS))
        for dut in made[1:]:
            _assert_same(made[0], dut, "three quanta on")
        assert made[0].demodulate() == made[1].demodulate() == made[2].demodulate()
    finally:
        _close(twin, sh, *made)


def test_any_length_quanta_at_44100_equal_the_twins(wm):
    """process_samples_at_any at 147 / 160, s16 frames, quanta of 128 from position 0"""
    twin, sh = _pair(wm, wm.PRECISION_F32, [0, 0])
    handles = []
    try:
        cap, play = wm.CaptureConverter(44100, 48000, S), wm.PlaybackConverter(48000, 44100, S)
        caps, plays = sh.make_rate_handles(wm.CaptureConverter, 44100, 48000), sh.make_rate_handles(wm.PlaybackConverter, 48000, 44100)
        handles = [cap, play] + caps + plays
        assert [h.n_streams for h in caps] == [h.n_streams for h in plays] == [66, 65] and (cap.up, cap.down, play.up, play.down) == (160, 147, 147, 160)
        pay, mask = _payloads(3, lambda s: s % 3 == 0)
        twin.modulate(pay, mask)
        sh.modulate(pay, mask)
        x = _line(wm, "s16", "sample", 128)

        def same(where):
            _assert_same(twin, sh, where)
            for one, parts in ((cap, caps), (play, plays)):
                assert [h.position for h in parts] == [one.position] * 2, where
                assert np.array_equal(np.concatenate([h.state() for h in parts]).view(np.uint32), one.state().view(np.uint32)), where
        for q in range(6):
            a = twin.process_samples_at_any(x, "s16", "sample", cap, 128, "s16", "sample", play)
            guard = np.full((128, S + 2), 0x5A5A, np.int16)
            b = sh.process_samples_at_any(x, "s16", "sample", caps, 128, "s16", "sample", plays, out=guard[:, 1:S + 1])
            assert np.array_equal(a, b) and (guard[:, 0] == 0x5A5A).all() and (guard[:, S + 1] == 0x5A5A).all(), q
            same(q)
            x = np.ascontiguousarray(np.roll(a, 1, axis=1))
        assert cap.position != 0 and np.count_nonzero(a) > 0 and sh.processDemodulationCallCount == 6
        assert set(sh.last_tx_kernel) == {twin.last_tx_kernel}
        # the refusals: before any shard is called, so no state word moves
        other = wm.CaptureConverter(44100, 48000, 65)                  # (at position 0, where the others have moved on)
        handles.append(other)
        for kw in (dict(upsampler=caps[:1], downsampler=plays), dict(upsampler=caps, downsampler=plays[::-1]), dict(upsampler=[caps[0], other], downsampler=plays),
                   dict(upsampler=caps, downsampler=None)):
            with pytest.raises(ValueError):
                sh.process_samples_at_any(x, "s16", "sample", n_out=128, out_fmt="s16", out_layout="sample", **kw)
        assert sh.processDemodulationCallCount == 6 and other.position == 0
        same("refused")
    finally:
        _close(twin, sh, *handles)
