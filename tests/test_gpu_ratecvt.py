"""The rational rate converter on the GPU (include/fskhip_next.h: fskhip_ratecvt_*; csrc/fsk_ratecvt.hip).

  * values: fp64 handles equal the CPU model (tests/ratecvt_ref.py) bit for bit; fp32 and fp64 handles equal FIRFilterBatch of the
    SAME precision, run on the GPU over the zero-stuffed input, columns ::M -- the same arithmetic in the same order, so no
    tolerance (np.array_equal on floats: zeros compare equal whatever their sign).  Ratios 3/2, 2/3, 7/5, 1/1, 160/147, 147/160 x
    taps 1, 5, L - 1 (fewer taps than phases), 13 and 16 max(L, M) + 1 x n_in of M, 3 M and one period past the plan's stream-major
    segment and past its sample-major tile x streams 1 / 63 / 65 / 130 x four formats x two layouts x two precisions x both
    directions, pitches wider than the rows, destinations off the 16-byte grid, and the whole destination compared, sentinels
    included: nothing else is written.  For the 160 / 147 pairs the stuffed reference is kept to 65 streams and 4 M inputs; the
    larger shapes of those pairs are held against the model (fp64);
  * with M = 1 a CaptureConverter is Upsampler(L), with L = 1 a PlaybackConverter is Downsampler(M), d_lens included;
  * d_lens: garbage behind a stream's length does not show, the tail ends in the format's silence, state() holds zeros there;
  * any cut into multiples of M gives the same samples and the same state(); the calls' refusals, in the header's order, leave
    state() as it was; reset(stream) zeroes that stream only; set_state(state()) on a twin under a permutation continues bit for bit;
  * end to end at 65 streams, Bell 202: modulate_samples_at(PlaybackConverter(48000, 44100)) -> demodulate_samples_at(
    CaptureConverter(44100, 48000)) returns every payload through s16, mu-law and A-law in both layouts, fp32 and fp64, and
    modulate_samples_at is the model's encoding of modulate_data's floats."""
import numpy as np
import pytest

import ratecvt_ref as rc
import samples_ref as sr

pytestmark = [pytest.mark.gpu]

PAIRS = ((3, 2), (2, 3), (7, 5), (1, 1), (160, 147), (147, 160))
STREAMS = (1, 63, 65, 130)
FORMATS = ("f32", "s16", "mulaw", "alaw")
LAYOUTS = ("stream", "sample")
BITS = {"f32": np.uint32, "s16": np.uint16, "mulaw": np.uint8, "alaw": np.uint8}
SENTINEL = {"f32": np.uint32(0x449A5000), "s16": np.uint16(0x5A5B), "mulaw": np.uint8(0xA5), "alaw": np.uint8(0xA5)}   # (f32: 1234.5)
SMAX, NMAX = max(STREAMS), 6400
MARGIN = 8
LDS = 65536
# shapes of _shapes() that have a reference: all 112 for fp64 (the model); for fp32 all but the 18 of the 160 / 147 pairs that are
# past the stuffed reference's bound (130 streams, or 25 periods)
COMPARED = {"f64": 112, "f32": 94}
BELL = dict(baudRate=1200, markFrequency=1200, spaceFrequency=2200)


def _wm():
    import webaudio_modem_amd as wm
    return wm


def _prec(name):
    wm = _wm()
    return wm.PRECISION_F64 if name == "f64" else wm.PRECISION_F32


def _taps(L, n_taps):
    return np.random.default_rng(1000 * L + n_taps).uniform(-1.0, 1.0, n_taps)


def _tap_counts(L, M):
    return sorted({1, 5, max(L - 1, 1), 13, 16 * max(L, M) + 1})


def _seg_periods(stream_major, playback, L, M, n_taps):
    """periods per workgroup, as csrc/fsk_ratecvt_plan.h cuts a launch (tests/cpp/ratecvt_plan_check.cpp holds that header)"""
    H = rc.history(L, n_taps)
    if stream_major:
        G = max(1024 // L, 1)
        while G > 1 and 4 * (H + 4 * G * M) > LDS * 3 // 4:
            G -= 1
        return 4 * G

    def lds(G, log2_ns):
        return 4 * ((((H + G * M) | 1) << log2_ns) + (G * L * ((1 << log2_ns) + 1) if playback else 0))
    G = max(64 // L, 1)
    while True:
        log2_ns = 0
        while log2_ns < 6 and lds(G, log2_ns + 1) <= LDS:
            log2_ns += 1
        if G == 1 or log2_ns >= 4:
            return G
        G = (G + 1) // 2


def _periods(L, M, n_taps, playback):
    """n_in / M of the shapes: one period, three, one past the sample-major tile, one past the stream-major segment"""
    return (1, 3, _seg_periods(False, playback, L, M, n_taps) + 1, _seg_periods(True, playback, L, M, n_taps) + 1)


@pytest.fixture(scope="module")
def eng():
    e = _wm().FSKEngine(1, {})
    yield e
    e.close()


_CACHE = {}


def _narrow(fmt):
    """[SMAX, NMAX] samples of the format, made once and never written to"""
    key = ("narrow", fmt)
    if key not in _CACHE:
        rng = np.random.default_rng(11)
        if fmt == "f32":
            a = rng.uniform(-1.2, 1.2, (SMAX, NMAX)).astype(np.float32)
            a[:, 5] = 0.0
        elif fmt == "s16":
            a = rng.integers(-32768, 32768, (SMAX, NMAX)).astype(np.int16)
        else:
            a = rng.integers(0, 256, (SMAX, NMAX)).astype(np.uint8)
        _CACHE[key] = a
    return _CACHE[key]


def _wide():
    """[SMAX, NMAX] floats in +-1.2: past the formats' range on both sides"""
    if "wide" not in _CACHE:
        _CACHE["wide"] = np.random.default_rng(12).uniform(-1.2, 1.2, (SMAX, NMAX)).astype(np.float32)
    return _CACHE["wide"]


@pytest.fixture(scope="module", autouse=True)
def _drop_cache():
    yield
    _CACHE.clear()


def _fir_ref(prec, x, taps, L, M):
    """FIRFilterBatch of the precision, on the GPU, over float32 [S, n] zero-stuffed by L, columns ::M"""
    z = np.zeros((x.shape[0], x.shape[1] * L), np.float32)
    z[:, ::L] = x
    f = _wm().FIRFilterBatch(taps, x.shape[0], precision=_prec(prec))
    try:
        return np.ascontiguousarray(f.processBuffer(z)[:, ::M])
    finally:
        f.close()


def _float_ref(prec, direction, fmt, L, M, n_taps, S, n_in):
    """{name: float32 [S, n_in / M * L]} of the references that hold for the shape: 'model' for fp64, 'fir' where the stuffed
    input is small (always for the small ratios; at most 65 streams and 4 M inputs for 160 / 147 and 147 / 160)"""
    key = ("ref", prec, direction, fmt if direction == "capture" else None, L, M, n_taps, n_in)
    if key not in _CACHE:
        x = sr.decode(_narrow(fmt)[:, :n_in], fmt) if direction == "capture" else _wide()[:, :n_in]
        refs = {}
        if prec == "f64":
            refs["model"] = (rc.convert(x, _taps(L, n_taps), L, M)[0], SMAX)
        if max(L, M) < 100 or n_in <= 4 * M:
            rows = SMAX if max(L, M) < 100 else 65
            refs["fir"] = (_fir_ref(prec, x[:rows], _taps(L, n_taps), L, M), rows)
        _CACHE[key] = refs
    return {k: v[:S] for k, (v, rows) in _CACHE[key].items() if S <= rows}


class _Buffers:
    """one narrow and one float buffer on the device, for many launches"""

    def __init__(self, eng, fmt):
        self.eng, self.fmt, self.bits = eng, fmt, BITS[fmt]
        self.esz = np.dtype(self.bits).itemsize
        self.n_narrow = 2 * MARGIN + 4 + max(SMAX * (NMAX + 8), NMAX * (SMAX + 8))
        self.n_wide = 2 * MARGIN + 4 + SMAX * (NMAX + 8)
        self.d_narrow = eng.device_malloc(self.n_narrow * self.esz)
        self.d_wide = eng.device_malloc(self.n_wide * 4)

    def close(self):
        for p in (self.d_narrow, self.d_wide):
            self.eng.device_free(p)

    def place(self, rows, pitch, off, total, fill, dtype):
        """a flat array of `fill` with `rows` at MARGIN + off, `pitch` elements apart"""
        used = MARGIN + off + (rows.shape[0] - 1) * pitch + rows.shape[1] + MARGIN
        assert used <= total and pitch >= rows.shape[1]                  # the launch stays inside the buffer: checked before it runs
        flat = np.full(used, fill, dtype)
        view = np.lib.stride_tricks.as_strided(flat[MARGIN + off:], shape=rows.shape, strides=(pitch * flat.itemsize, flat.itemsize))
        view[...] = rows
        return flat


def _variants(i):
    """(narrow pitch extra, float pitch extra, float offset in floats, narrow offset in elements), walking through the alignments"""
    return (0, 5)[i % 2], (0, 4, 3, 1)[(i // 2) % 4], (0, 1, 2, 3)[(i // 3) % 4], (0, 1, 3, 0)[(i // 5) % 4]


def _shapes(playback):
    """(L, M, n_taps, S, n_in): every ratio x tap count with every stream count and every length, four of the sixteen (S, n_in)
    each, a diagonal that moves on from one to the next"""
    i = 0
    for L, M in PAIRS:
        for n_taps in _tap_counts(L, M):
            periods = _periods(L, M, n_taps, playback)
            for j in range(4):
                S, per = STREAMS[(i + j) % 4], periods[(i // 4 + j + i) % 4]
                assert per * M <= NMAX and per * L <= NMAX
                yield L, M, n_taps, S, per * M
            i += 1


def test_the_shapes_cover_every_stream_count_and_length():
    for playback in (False, True):
        shapes = list(_shapes(playback))
        for L, M in PAIRS:
            for n_taps in _tap_counts(L, M):
                mine = [(S, n // M) for l, m, t, S, n in shapes if (l, m, t) == (L, M, n_taps)]
                assert sorted(S for S, _ in mine) == sorted(STREAMS) and sorted(per for _, per in mine) == sorted(_periods(L, M, n_taps, playback))
        assert len({(STREAMS.index(S), _periods(L, M, t, playback).index(n // M)) for L, M, t, S, n in shapes if (L, M) == (7, 5) or (L, M) == (3, 2)}) >= 8


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_capture_values(eng, prec, fmt, layout):
    wm = _wm()
    buf = _Buffers(eng, fmt)
    sent_f = np.array([SENTINEL["f32"]], np.uint32).view(np.float32)[0]
    compared = 0
    try:
        for i, (L, M, n_taps, S, n_in) in enumerate(_shapes(False)):
            refs = _float_ref(prec, "capture", fmt, L, M, n_taps, S, n_in)
            if not refs:
                continue                                                 # (fp32 at a 160 / 147 shape past the stuffed reference's bound)
            compared += 1
            n_out = n_in // M * L
            cv = wm.CaptureConverter(M, L, S, taps=_taps(L, n_taps), precision=_prec(prec))
            try:
                assert (cv.up, cv.down, cv.history, cv.out_count(n_in)) == (L, M, rc.history(L, n_taps), n_out)
                pe, we, woff, noff = _variants(i)
                src = _narrow(fmt)[:S, :n_in].view(BITS[fmt])
                rows = src if layout == "stream" else np.ascontiguousarray(src.T)
                npitch, wpitch = rows.shape[1] + pe, n_out + we
                eng.h2d(buf.d_narrow, buf.place(rows, npitch, noff, buf.n_narrow, SENTINEL[fmt], BITS[fmt]))
                n_dst = MARGIN + woff + (S - 1) * wpitch + n_out + MARGIN
                assert n_dst <= buf.n_wide                               # the launch stays inside the buffer: checked before it runs
                eng.h2d(buf.d_wide, np.full(n_dst, sent_f, np.float32))
                cv.process_device(buf.d_narrow + (MARGIN + noff) * buf.esz, fmt, layout, n_in, npitch, buf.d_wide + 4 * (MARGIN + woff), wpitch)
                eng.synchronize()
                for name, ref in refs.items():
                    want = buf.place(ref, wpitch, woff, buf.n_wide, sent_f, np.float32)
                    got = np.zeros(want.size, np.float32)
                    eng.d2h(got, buf.d_wide)
                    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32)) if name == "model" else np.flatnonzero(got != want)
                    assert bad.size == 0, "%s %s %s %s S=%d %d/%d taps=%d n_in=%d pitches %d / %d offsets %d / %d: %d floats differ, first at %d (got %r, want %r)" % (
                        name, prec, fmt, layout, S, L, M, n_taps, n_in, npitch, wpitch, noff, woff, bad.size, bad[0] - MARGIN - woff, got[bad[0]], want[bad[0]])
                assert np.array_equal(cv.state(), rc.capture(_narrow(fmt)[:S, :n_in], fmt, _taps(L, n_taps), L, M)[1])
            finally:
                cv.close()
    finally:
        buf.close()
    assert compared == COMPARED[prec]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_playback_values(eng, prec, fmt, layout):
    wm = _wm()
    buf = _Buffers(eng, fmt)
    sent_f = np.array([SENTINEL["f32"]], np.uint32).view(np.float32)[0]
    compared = 0
    try:
        for i, (L, M, n_taps, S, n_in) in enumerate(_shapes(True)):
            refs = _float_ref(prec, "playback", fmt, L, M, n_taps, S, n_in)
            if not refs:
                continue
            compared += 1
            n_out = n_in // M * L
            cv = wm.PlaybackConverter(M, L, S, taps=_taps(L, n_taps), precision=_prec(prec))
            try:
                assert (cv.up, cv.down, cv.history, cv.out_count(n_in)) == (L, M, rc.history(L, n_taps), n_out)
                pe, we, woff, noff = _variants(i)
                npitch, wpitch = (n_out if layout == "stream" else S) + pe, n_in + we
                shape = (S, n_out) if layout == "stream" else (n_out, S)
                eng.h2d(buf.d_wide, buf.place(_wide()[:S, :n_in], wpitch, woff, buf.n_wide, sent_f, np.float32))
                n_dst = MARGIN + noff + (shape[0] - 1) * npitch + shape[1] + MARGIN
                assert n_dst <= buf.n_narrow and npitch >= shape[1]      # the launch stays inside the buffer: checked before it runs
                eng.h2d(buf.d_narrow, np.full(n_dst, SENTINEL[fmt], BITS[fmt]))
                cv.process_device(buf.d_wide + 4 * (MARGIN + woff), n_in, wpitch, None, buf.d_narrow + (MARGIN + noff) * buf.esz, fmt, layout, npitch)
                eng.synchronize()
                for name, ref in refs.items():
                    enc = sr.encode(ref, fmt).view(BITS[fmt])
                    want = buf.place(enc if layout == "stream" else np.ascontiguousarray(enc.T), npitch, noff, buf.n_narrow, SENTINEL[fmt], BITS[fmt])
                    got = np.zeros(want.size, BITS[fmt])
                    eng.d2h(got, buf.d_narrow)
                    if fmt == "f32" and name == "fir":                   # (floats as bits: zeros compare equal whatever their sign)
                        bad = np.flatnonzero(got.view(np.float32) != want.view(np.float32))
                    else:
                        bad = np.flatnonzero(got != want)
                    assert bad.size == 0, "%s %s %s %s S=%d %d/%d taps=%d n_in=%d pitches %d / %d offsets %d / %d: %d elements differ, first at %d (got %#x, want %#x)" % (
                        name, prec, fmt, layout, S, L, M, n_taps, n_in, npitch, wpitch, noff, woff, bad.size, bad[0] - MARGIN - noff, got[bad[0]], want[bad[0]])
                assert np.array_equal(cv.state(), rc.convert(_wide()[:S, :n_in], _taps(L, n_taps), L, M)[1])
            finally:
                cv.close()
    finally:
        buf.close()
    assert compared == COMPARED[prec]


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_integer_ratios_are_the_resamplers(prec):
    wm = _wm()
    S = 65
    for factor, n_taps, n in ((6, 97, 1000), (3, 13, 37), (2, 1, 160), (1, 5, 64)):
        taps = _taps(factor, n_taps)
        lens = np.array([(0, 1, 7, n * factor // 2, n * factor - 1, n * factor, n * factor + 50, 33)[s % 8] for s in range(S)], np.uint32)
        for fmt, layout in (("mulaw", "stream"), ("s16", "sample"), ("f32", "stream"), ("alaw", "sample")):
            up, cap = wm.Upsampler(factor, S, taps=taps, precision=_prec(prec)), wm.CaptureConverter(1, factor, S, taps=taps, precision=_prec(prec))
            down, play = wm.Downsampler(factor, S, taps=taps, precision=_prec(prec)), wm.PlaybackConverter(factor, 1, S, taps=taps, precision=_prec(prec))
            try:
                assert (cap.up, cap.down, play.up, play.down) == (factor, 1, 1, factor) and cap.history == up.history and play.history == down.history
                x = _narrow(fmt)[:S, :n]
                x = x if layout == "stream" else np.ascontiguousarray(x.T)
                assert np.array_equal(cap.process(x, fmt, layout).view(np.uint32), up.process(x, fmt, layout).view(np.uint32)), (factor, n_taps, fmt, layout)
                assert np.array_equal(cap.state().view(np.uint32), up.state().view(np.uint32))
                w = _wide()[:S, :n * factor]
                for ln in (None, lens):
                    assert np.array_equal(play.process(w, fmt, layout, lens=ln).view(BITS[fmt]), down.process(w, fmt, layout, lens=ln).view(BITS[fmt])), (factor, n_taps, fmt, layout)
                    assert np.array_equal(play.state().view(np.uint32), down.state().view(np.uint32))
            finally:
                for h in (up, cap, down, play):
                    h.close()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_playback_lens_hide_what_lies_behind_a_stream(fmt, layout):
    wm = _wm()
    S, n_in = 65, 160 * 12
    x = _wide()[:S, :n_in].copy()
    lens = np.array([(0, 1, 7, 480, n_in - 1, n_in, n_in + 80, 333)[s % 8] for s in range(S)], np.uint32)
    clean = np.where(np.arange(n_in)[None, :] < lens[:, None].astype(np.int64), x, np.float32(0.0))
    for prec in (wm.PRECISION_F32, wm.PRECISION_F64):
        a, b = wm.PlaybackConverter(48000, 44100, S, precision=prec), wm.PlaybackConverter(48000, 44100, S, precision=prec)
        try:
            taps = a.taps
            assert len(taps) == 2561 and (a.up, a.down, a.history) == (147, 160, 18)
            got = a.process(x, fmt, layout, lens=lens)                   # garbage behind every length ...
            want = b.process(clean, fmt, layout)                         # ... against zeros there
            assert np.array_equal(got.view(BITS[fmt]), want.view(BITS[fmt]))
            state = a.state()
            assert np.array_equal(state, b.state())                      # the history holds what was read, not what was there
            rows = got if layout == "stream" else got.T
            for s in range(S):
                assert (rows[s, min(a.out_length(min(int(lens[s]), n_in)), rows.shape[1]):].view(BITS[fmt]) == np.asarray(sr.silence(fmt)).view(BITS[fmt])).all(), s
                assert not state[s, max(0, a.history - (n_in - min(int(lens[s]), n_in))):].any()
            if prec == wm.PRECISION_F64:
                model, hist = rc.playback(x, taps, 147, 160, fmt, lens=lens)
                assert np.array_equal(np.ascontiguousarray(rows).view(BITS[fmt]), model.view(BITS[fmt])) and np.array_equal(state, hist)
        finally:
            a.close()
            b.close()


def test_refused_calls_in_order_leave_the_history():
    wm = _wm()
    from webaudio_modem_amd import _lib
    S = 3
    p, c, c2 = wm.PlaybackConverter(3, 2, S, taps=_taps(2, 13)), wm.CaptureConverter(2, 3, S, taps=_taps(3, 13)), wm.CaptureConverter(3, 2, S, taps=_taps(2, 13))
    try:
        assert (p.up, p.down, c.up, c.down, c2.up, c2.down) == (2, 3, 3, 2, 2, 3)
        x = _wide()[:S, :60].copy()
        p.process(x, "s16")
        before = p.state()
        assert before.any()
        for n in (61, 5, 1):
            with pytest.raises(wm.FskHipError) as ei:
                p.process(_wide()[:S, :n], "s16")
            assert ei.value.code == _lib.E_INVALID and "fskhip_ratecvt_playback_host: n_in %d is not a multiple of the down factor 3" % n in str(ei.value)
        with pytest.raises(wm.FskHipError, match="fskhip_ratecvt_capture_host: n_in 7 is not a multiple of the down factor 2"):
            c.process(_narrow("s16")[:S, :7], "s16")
        out = np.zeros((S, 40), np.int16)
        L_, X, O = p._L, x.ctypes.data, out.ctypes.data
        # each call is wrong in everything behind what it is refused for as well
        for call, text in ((lambda: L_.fskhip_ratecvt_playback_host(p._h, None, 61, 0, None, None, 9, 5, 0), "fskhip_ratecvt_playback_host: unknown sample format 9"),
                           (lambda: L_.fskhip_ratecvt_playback_host(p._h, None, 61, 0, None, None, 1, 5, 0), "fskhip_ratecvt_playback_host: unknown layout 5"),
                           (lambda: L_.fskhip_ratecvt_playback_host(c2._h, None, 61, 0, None, O + 1, 1, 0, 0), "fskhip_ratecvt_playback_host: null buffer"),
                           (lambda: L_.fskhip_ratecvt_playback_host(c2._h, X, 61, 60, None, O + 1, 1, 0, 0), "fskhip_ratecvt_playback_host: float pitch 60 < 61 samples per stream"),
                           (lambda: L_.fskhip_ratecvt_playback_host(c2._h, X, 61, 61, None, O + 1, 1, 0, 39), "fskhip_ratecvt_playback_host: sample pitch 39 < 40 samples per stream"),
                           (lambda: L_.fskhip_ratecvt_playback_host(c2._h, X, 61, 61, None, O + 1, 1, 1, 2), "fskhip_ratecvt_playback_host: frame pitch 2 < n_streams 3"),
                           (lambda: L_.fskhip_ratecvt_playback_host(c2._h, X, 61, 61, None, O + 1, 1, 0, 40), "fskhip_ratecvt_playback_host: a buffer is not aligned to its element size"),
                           (lambda: L_.fskhip_ratecvt_playback_host(c2._h, X, 61, 61, None, O, 1, 0, 40), "fskhip_ratecvt_playback_host: the handle converts for capture"),
                           (lambda: L_.fskhip_ratecvt_capture_host(p._h, O, 1, 0, 7, 7, X, 60), "fskhip_ratecvt_capture_host: the handle converts for playback"),
                           (lambda: L_.fskhip_ratecvt_playback_host(p._h, X, 61, 61, None, O, 1, 0, 40), "fskhip_ratecvt_playback_host: n_in 61 is not a multiple of the down factor 3"),
                           (lambda: L_.fskhip_ratecvt_capture_host(c._h, O, 1, 0, 7, 7, X, 60), "fskhip_ratecvt_capture_host: n_in 7 is not a multiple of the down factor 2"),
                           (lambda: L_.fskhip_ratecvt_capture_host(c._h, O, 1, 0, 8, 8, X, 11), "fskhip_ratecvt_capture_host: float pitch 11 < 12 samples per stream"),
                           (lambda: L_.fskhip_ratecvt_capture_host(c._h, O, 1, 0, 8, 7, X, 12), "fskhip_ratecvt_capture_host: sample pitch 7 < 8 samples per stream")):
            assert call() == _lib.E_INVALID and L_.fskhip_last_error().decode() == text
        # the wrong call for the handle is refused whatever its length; the right one with no samples does nothing
        assert L_.fskhip_ratecvt_capture_host(p._h, None, 1, 0, 0, 0, None, 0) == _lib.E_INVALID
        assert L_.fskhip_last_error().decode() == "fskhip_ratecvt_capture_host: the handle converts for playback"
        assert L_.fskhip_ratecvt_playback_host(p._h, None, 0, 0, None, None, 1, 0, 0) == 0 and L_.fskhip_ratecvt_capture_host(c._h, None, 1, 0, 0, 0, None, 0) == 0
        assert np.array_equal(p.state(), before) and not c.state().any() and not c2.state().any()
        assert p.process(np.zeros((S, 0), np.float32), "s16").shape == (S, 0) and np.array_equal(p.state(), before)
    finally:
        for h in (p, c, c2):
            h.close()


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("direction", ["capture", "playback"])
def test_any_cut_into_multiples_of_down_is_one_call(direction, prec):
    wm = _wm()
    S = 65
    for (L, M), periods in (((160, 147), 30), ((147, 160), 30), ((3, 2), 1400)):   # (past one stream-major segment each)
        rates = (M * 300, L * 300)
        for fmt, layout in (("mulaw", "stream"), ("s16", "sample")):
            for taps in (None, _taps(L, 13)):
                cls = wm.CaptureConverter if direction == "capture" else wm.PlaybackConverter
                make = lambda: cls(rates[0], rates[1], S, taps=taps, precision=_prec(prec))   # noqa: E731
                x = _narrow(fmt)[:S, :periods * M] if direction == "capture" else _wide()[:S, :periods * M]

                def run(h, piece):
                    if direction == "capture":
                        return h.process(piece if layout == "stream" else np.ascontiguousarray(piece.T), fmt, layout)
                    o = h.process(piece, fmt, layout)
                    return o if layout == "stream" else o.T
                one = make()
                try:
                    assert (one.up, one.down) == (L, M)
                    whole = run(one, x)
                    state = one.state()
                    assert state.shape == (S, one.history) and state.any()
                    for schedule in ((1, 2, 7, periods - 10), (periods - 1, 1)):
                        h = make()
                        try:
                            parts, at = [], 0
                            for c in schedule:
                                parts.append(run(h, x[:, at:at + c * M]))
                                at += c * M
                            assert at == x.shape[1] and np.array_equal(np.concatenate(parts, axis=1).view(BITS[fmt] if direction == "playback" else np.uint32),
                                                                        np.ascontiguousarray(whole).view(BITS[fmt] if direction == "playback" else np.uint32)), (L, M, fmt, layout, schedule)
                            assert np.array_equal(h.state().view(np.uint32), state.view(np.uint32)), (L, M, fmt, layout, schedule)
                        finally:
                            h.close()
                finally:
                    one.close()


@pytest.mark.parametrize("direction", ["capture", "playback"])
def test_reset_and_state_carry(direction):
    wm = _wm()
    S, L, M, periods = 7, 7, 5, 16
    taps = _taps(L, 113)
    cls = wm.CaptureConverter if direction == "capture" else wm.PlaybackConverter
    make = lambda: cls(M, L, S, taps=taps)   # noqa: E731
    x = _narrow("s16")[:S, :2 * periods * M] if direction == "capture" else _wide()[:S, :2 * periods * M]
    half = periods * M

    def run(h, a):
        return h.process(a, "s16")

    a, twin, fresh = make(), make(), make()
    try:
        first = run(a, x[:, :half])
        st = a.state()
        assert st.shape == (S, 16) and st.any(axis=1).all()
        # reset(stream) zeroes that stream's history only
        a.reset(2)
        after = a.state()
        assert not after[2].any() and np.array_equal(np.delete(after, 2, 0), np.delete(st, 2, 0))
        cont = run(a, x[:, half:])
        whole = run(fresh, x)
        assert np.array_equal(np.delete(np.concatenate([first, cont], 1), 2, 0), np.delete(whole, 2, 0))
        fresh.reset()
        assert not fresh.state().any()
        assert np.array_equal(cont[2], run(fresh, x[:, half:])[2])        # stream 2 went on as a new one
        # set_state(state()) on a twin under a permutation continues bit for bit
        a.reset()
        run(a, x[:, :half])
        perm = np.array([3, 0, 6, 1, 5, 2, 4])
        twin.set_state(a.state()[perm])
        assert np.array_equal(run(twin, x[perm][:, half:]), run(a, x[:, half:])[perm])
        assert np.array_equal(twin.state(), a.state()[perm])
        with pytest.raises(ValueError):
            twin.set_state(np.zeros((S, twin.history + 1), np.float32))
    finally:
        for h in (a, twin, fresh):
            h.close()


# ---- end to end: a 48 kHz engine behind and in front of 44.1 kHz audio --------------------------------------------------------------
S_TRIP = 65


def _payloads():
    rng = np.random.default_rng(44100)
    return [bytes(rng.integers(0, 256, int(rng.integers(1, 41))).astype(np.uint8)) for _ in range(S_TRIP)]


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_round_trip_at_44100(prec):
    """Bell 202, 65 streams, random payloads of 1 .. 40 bytes, s16 and both G.711 laws, both layouts: every payload comes back"""
    wm = _wm()
    payloads = _payloads()
    tx, rx = wm.FSKEngine(S_TRIP, BELL, precision=_prec(prec)), wm.FSKEngine(S_TRIP, BELL, precision=_prec(prec))
    play, cap = wm.PlaybackConverter(48000, 44100, S_TRIP, precision=_prec(prec)), wm.CaptureConverter(44100, 48000, S_TRIP, precision=_prec(prec))
    try:
        assert len(play.taps) == len(cap.taps) == 2561 and (play.up, play.down, cap.up, cap.down) == (147, 160, 160, 147)
        n = (-(-play.out_length(tx.modulated_length(40)) // 147) + 2) * 147   # whole periods of the capture converter, and its delay
        for fmt in ("mulaw", "alaw", "s16"):
            for layout in LAYOUTS:
                for h in (play, cap):
                    h.reset()
                rx.reset()
                samples, lens = tx.modulate_samples_at(payloads, fmt, layout, play, n_per_stream=n)
                assert samples.dtype == sr.DTYPES[fmt] and samples.shape == ((S_TRIP, n) if layout == "stream" else (n, S_TRIP))
                assert lens.tolist() == [play.out_length(tx.modulated_length(len(p))) for p in payloads]
                got, _eod = rx.demodulate_samples_at(samples, fmt, layout, cap)
                assert got == payloads, (fmt, layout, [s for s in range(S_TRIP) if got[s] != payloads[s]])
        with pytest.raises(ValueError, match="not a multiple of the converter's down factor 147"):
            rx.demodulate_samples_at(np.zeros((S_TRIP, 148), np.int16), "s16", "stream", cap)
    finally:
        for h in (tx, rx, play, cap):
            h.close()


def test_modulate_samples_at_is_the_models_encoding_of_the_float_call():
    wm = _wm()
    payloads = _payloads()
    tx = wm.FSKEngine(S_TRIP, BELL, precision=wm.PRECISION_F64)
    play = wm.PlaybackConverter(48000, 44100, S_TRIP, precision=wm.PRECISION_F64)
    try:
        sigs = tx.modulate_data(payloads)
        n = play.out_length(max(s.size for s in sigs))
        assert n == rc.out_length(147, 160, 2561, max(s.size for s in sigs))
        x = np.zeros((S_TRIP, -(-n // 147) * 160), np.float32)
        for s, sig in enumerate(sigs):
            x[s, :sig.size] = sig
        y = rc.convert(x, play.taps, 147, 160)[0][:, :n]
        for fmt in ("mulaw", "alaw", "s16", "f32"):
            want = sr.encode(y, fmt).view(BITS[fmt])
            for layout in LAYOUTS:
                play.reset()
                got, lens = tx.modulate_samples_at(payloads, fmt, layout, play)
                rows = got if layout == "stream" else np.ascontiguousarray(got.T)
                assert rows.shape == (S_TRIP, n) and np.array_equal(rows.view(BITS[fmt]), want), (fmt, layout)
                assert lens.tolist() == [min(rc.out_length(147, 160, 2561, s.size), n) for s in sigs]
                for s in range(S_TRIP):
                    assert (rows[s, lens[s]:].view(BITS[fmt]) == np.asarray(sr.silence(fmt)).view(BITS[fmt])).all()
        # a slab too short for the longest signal is the modulator's refusal
        before = play.state()
        with pytest.raises(wm.FskHipError) as ei:
            tx.modulate_samples_at(payloads, "s16", "stream", play, n_per_stream=147)
        from webaudio_modem_amd import _lib
        assert ei.value.code == _lib.E_OVERFLOW and np.array_equal(play.state(), before)      # ... made before the converter runs
    finally:
        for h in (tx, play):
            h.close()
