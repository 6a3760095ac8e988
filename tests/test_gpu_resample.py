"""The resampler on the GPU (include/fskhip_next.h: fskhip_resampler_*; csrc/fsk_resample.hip).

  * up: the float tile equals FIRFilterBatch of the SAME precision, run on the GPU over the zero-stuffed decoded input -- the same
    arithmetic in the same order, so no tolerance (np.array_equal on floats: zeros compare equal whatever their sign); on fp64 it
    also equals the CPU model (tests/resample_ref.py).  down: bit for bit samples_ref.encode(FIRFilterBatch(x)[:, ::L]).
    Streams 1 / 63 / 65 / 130 x L 1 / 2 / 3 / 6 x 1 / 5 / 6 / 13 / 97 taps (fewer taps than phases, a ragged last phase) x 1 / 3 /
    37 / 160 / 1030 samples (1030 crosses the stream-major segment of 1024, 160 the sample-major tile of 64) x four formats x two
    layouts x two precisions, pitches wider than the rows, destinations off the 16-byte grid, and the whole destination compared,
    sentinels included: nothing else is written;
  * d_lens: garbage behind a stream's length does not show and the tail ends in the format's silence; n_in that is no multiple of
    L is refused and leaves the history as it was;
  * any cut of a stream into calls gives the same samples and the same state(); reset(stream) zeroes that stream only;
    set_state(state()) on a twin under a permutation continues bit for bit;
  * end to end at 65 streams, Bell 202: modulate_samples_at -> demodulate_samples_at returns every payload through mu-law, A-law and
    s16 in both layouts, fp32 and fp64; modulate_samples_at is the model's encoding of FIRFilterBatch(modulate_data(...))[:, ::6]."""
import numpy as np
import pytest

import resample_ref as rr
import samples_ref as sr

pytestmark = [pytest.mark.gpu]

STREAMS = (1, 63, 65, 130)
FACTORS = (1, 2, 3, 6)
TAPS = (1, 5, 6, 13, 97)
LENGTHS = (1, 3, 37, 160, 1030)
FORMATS = ("f32", "s16", "mulaw", "alaw")
LAYOUTS = ("stream", "sample")
BITS = {"f32": np.uint32, "s16": np.uint16, "mulaw": np.uint8, "alaw": np.uint8}
SENTINEL = {"f32": np.uint32(0x449A5000), "s16": np.uint16(0x5A5B), "mulaw": np.uint8(0xA5), "alaw": np.uint8(0xA5)}   # (f32: 1234.5)
SMAX, NMAX, LMAX = max(STREAMS), max(LENGTHS), max(FACTORS)
MARGIN = 8
BELL = dict(baudRate=1200, markFrequency=1200, spaceFrequency=2200)


def _wm():
    import webaudio_modem_amd as wm
    return wm


def _prec(name):
    wm = _wm()
    return wm.PRECISION_F64 if name == "f64" else wm.PRECISION_F32


@pytest.fixture(scope="module")
def eng():
    e = _wm().FSKEngine(1, {})
    yield e
    e.close()


def _taps(L, n_taps):
    return np.random.default_rng(1000 * L + n_taps).uniform(-1.0, 1.0, n_taps)


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
    """[SMAX, NMAX * LMAX] floats in +-1.2: past the formats' range on both sides"""
    if "wide" not in _CACHE:
        _CACHE["wide"] = np.random.default_rng(12).uniform(-1.2, 1.2, (SMAX, NMAX * LMAX)).astype(np.float32)
    return _CACHE["wide"]


def _fir(prec, L, n_taps, x):
    """FIRFilterBatch of the precision over float32 [SMAX, n], from a reset delay line (one filter per tap set, kept)"""
    key = ("fir", prec, L, n_taps)
    if key not in _CACHE:
        _CACHE[key] = _wm().FIRFilterBatch(_taps(L, n_taps), SMAX, precision=_prec(prec))
    f = _CACHE[key]
    f.reset()
    return f.processBuffer(x)


def _up_ref(prec, fmt, L, n_taps, n):
    key = ("up", prec, fmt, L, n_taps, n)
    if key not in _CACHE:
        _CACHE[key] = _fir(prec, L, n_taps, rr.stuff(_narrow(fmt)[:, :n], fmt, L))
    return _CACHE[key]


def _down_ref(prec, L, n_taps, n_out):
    key = ("down", prec, L, n_taps, n_out)
    if key not in _CACHE:
        _CACHE[key] = np.ascontiguousarray(_fir(prec, L, n_taps, _wide()[:, :n_out * L])[:, ::L])
    return _CACHE[key]


@pytest.fixture(scope="module", autouse=True)
def _drop_cache():
    yield
    for k, v in list(_CACHE.items()):
        if k[0] == "fir":
            v.close()
    _CACHE.clear()


class _Buffers:
    """one narrow and one float buffer on the device, for many launches"""

    def __init__(self, eng, fmt):
        self.eng, self.fmt, self.bits = eng, fmt, BITS[fmt]
        self.esz = np.dtype(self.bits).itemsize
        self.n_narrow = 2 * MARGIN + 4 + max(SMAX * (NMAX + 8), NMAX * (SMAX + 8))
        self.n_wide = 2 * MARGIN + 4 + SMAX * (NMAX * LMAX + 8)
        self.d_narrow = eng.device_malloc(self.n_narrow * self.esz)
        self.d_wide = eng.device_malloc(self.n_wide * 4)
        self.d_lens = eng.device_malloc(4 * SMAX)

    def close(self):
        for p in (self.d_narrow, self.d_wide, self.d_lens):
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


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_up_equals_fir_over_the_zero_stuffed_input(eng, prec, fmt, layout):
    wm = _wm()
    buf = _Buffers(eng, fmt)
    sent_f = np.array([SENTINEL["f32"]], np.uint32).view(np.float32)[0]
    i = 0
    try:
        for L in FACTORS:
            for n_taps in TAPS:
                for S in STREAMS:
                    up = wm.Upsampler(L, S, taps=_taps(L, n_taps), precision=_prec(prec))
                    try:
                        assert up.history == (n_taps - 1 + L - 1) // L
                        for n in LENGTHS:
                            pe, we, woff, noff = _variants(i)
                            i += 1
                            src = _narrow(fmt)[:S, :n].view(BITS[fmt])
                            rows = src if layout == "stream" else np.ascontiguousarray(src.T)
                            npitch, wpitch = rows.shape[1] + pe, n * L + we
                            host = buf.place(rows, npitch, noff, buf.n_narrow, SENTINEL[fmt], BITS[fmt])
                            want = buf.place(_up_ref(prec, fmt, L, n_taps, n)[:S], wpitch, woff, buf.n_wide, sent_f, np.float32)
                            eng.h2d(buf.d_narrow, host)
                            eng.h2d(buf.d_wide, np.full(want.size, sent_f, np.float32))
                            up.reset()
                            up.process_device(buf.d_narrow + (MARGIN + noff) * buf.esz, fmt, layout, n, npitch, buf.d_wide + 4 * (MARGIN + woff), wpitch)
                            eng.synchronize()
                            got = np.zeros(want.size, np.float32)
                            eng.d2h(got, buf.d_wide)
                            bad = np.flatnonzero(got != want)
                            assert bad.size == 0, "%s %s %s S=%d L=%d taps=%d n=%d pitches %d / %d offsets %d / %d: %d floats differ, first at %d (got %r, want %r)" % (
                                prec, fmt, layout, S, L, n_taps, n, npitch, wpitch, noff, woff, bad.size, bad[0] - MARGIN - woff, got[bad[0]], want[bad[0]])
                    finally:
                        up.close()
    finally:
        buf.close()
    assert i == len(FACTORS) * len(TAPS) * len(STREAMS) * len(LENGTHS)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_down_equals_the_encoded_fir_output(eng, prec, fmt, layout):
    wm = _wm()
    buf = _Buffers(eng, fmt)
    sent_f = np.array([SENTINEL["f32"]], np.uint32).view(np.float32)[0]
    i = 0
    try:
        for L in FACTORS:
            for n_taps in TAPS:
                for S in STREAMS:
                    down = wm.Downsampler(L, S, taps=_taps(L, n_taps), precision=_prec(prec))
                    try:
                        assert down.history == n_taps - 1
                        for n in LENGTHS:                                  # (samples per stream at the LOW rate)
                            pe, we, woff, noff = _variants(i)
                            i += 1
                            enc = sr.encode(_down_ref(prec, L, n_taps, n)[:S], fmt).view(BITS[fmt])
                            rows = enc if layout == "stream" else np.ascontiguousarray(enc.T)
                            npitch, wpitch = rows.shape[1] + pe, n * L + we
                            want = buf.place(rows, npitch, noff, buf.n_narrow, SENTINEL[fmt], BITS[fmt])
                            host = buf.place(_wide()[:S, :n * L], wpitch, woff, buf.n_wide, sent_f, np.float32)
                            eng.h2d(buf.d_wide, host)
                            eng.h2d(buf.d_narrow, np.full(want.size, SENTINEL[fmt], BITS[fmt]))
                            down.reset()
                            down.process_device(buf.d_wide + 4 * (MARGIN + woff), n * L, wpitch, None, buf.d_narrow + (MARGIN + noff) * buf.esz, fmt, layout, npitch)
                            eng.synchronize()
                            got = np.zeros(want.size, BITS[fmt])
                            eng.d2h(got, buf.d_narrow)
                            bad = np.flatnonzero(got != want)
                            assert bad.size == 0, "%s %s %s S=%d L=%d taps=%d n=%d pitches %d / %d offsets %d / %d: %d elements differ, first at %d (got %#x, want %#x)" % (
                                prec, fmt, layout, S, L, n_taps, n, npitch, wpitch, noff, woff, bad.size, bad[0] - MARGIN - noff, got[bad[0]], want[bad[0]])
                    finally:
                        down.close()
    finally:
        buf.close()
    assert i == len(FACTORS) * len(TAPS) * len(STREAMS) * len(LENGTHS)


def test_up_fp64_equals_the_cpu_model():
    wm = _wm()
    S, n = 5, 160
    for L in FACTORS:
        for n_taps in TAPS:
            for fmt in ("s16", "mulaw"):
                up = wm.Upsampler(L, S, taps=_taps(L, n_taps), precision=wm.PRECISION_F64)
                try:
                    x = _narrow(fmt)[:S, :n]
                    assert np.array_equal(up.process(x, fmt), rr.up(x, fmt, _taps(L, n_taps), L)), (L, n_taps, fmt)
                finally:
                    up.close()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_down_lens_hide_what_lies_behind_a_stream(fmt, layout):
    wm = _wm()
    S, L, n_out = 65, 6, 160
    x = _wide()[:S, :n_out * L].copy()
    lens = np.array([(0, 1, 7, 480, 959, 960, 2000, 333)[s % 8] for s in range(S)], np.uint32)
    clean = np.where(np.arange(x.shape[1])[None, :] < lens[:, None].astype(np.int64), x, np.float32(0.0))
    for prec in (wm.PRECISION_F32, wm.PRECISION_F64):
        a, b = wm.Downsampler(L, S, precision=prec), wm.Downsampler(L, S, precision=prec)
        try:
            taps = a.taps
            assert len(taps) == 97 and a.history == 96
            got = a.process(x, fmt, layout, lens=lens)                   # garbage behind every length ...
            want = b.process(clean, fmt, layout)                         # ... against zeros there
            assert np.array_equal(got.view(BITS[fmt]), want.view(BITS[fmt]))
            assert np.array_equal(a.state(), b.state())                  # the history holds what was read, not what was there
            rows = got if layout == "stream" else got.T
            for s in range(S):
                end = min((int(lens[s]) + len(taps) - 1 + L - 1) // L, n_out)
                assert (rows[s, end:].view(BITS[fmt]) == np.asarray(sr.silence(fmt)).view(BITS[fmt])).all(), s
            if prec == wm.PRECISION_F64:
                assert np.array_equal(np.ascontiguousarray(rows).view(BITS[fmt]), rr.down(x, taps, L, fmt, lens=lens).view(BITS[fmt]))
        finally:
            a.close()
            b.close()


def test_refused_calls_leave_the_history():
    wm = _wm()
    from webaudio_modem_amd import _lib
    S, L = 3, 6
    d, u = wm.Downsampler(L, S), wm.Upsampler(L, S)
    try:
        x = _wide()[:S, :60].copy()
        d.process(x, "s16")
        before = d.state()
        assert before.any()
        for n in (61, 5, 1):
            with pytest.raises(wm.FskHipError) as ei:
                d.process(_wide()[:S, :n], "s16")
            assert ei.value.code == _lib.E_INVALID and "fskhip_resampler_down_host: n_in %d is not a multiple of the factor 6" % n in str(ei.value)
        out = np.zeros((S, 10), np.int16)
        L_ = d._L
        for call, text in ((lambda: L_.fskhip_resampler_up_host(d._h, out.ctypes.data, 1, 0, 10, 10, x.ctypes.data, 60), "fskhip_resampler_up_host: the handle resamples down"),
                           (lambda: L_.fskhip_resampler_down_host(u._h, x.ctypes.data, 60, 60, None, out.ctypes.data, 1, 0, 10), "fskhip_resampler_down_host: the handle resamples up"),
                           (lambda: L_.fskhip_resampler_down_host(d._h, x.ctypes.data, 60, 60, None, out.ctypes.data, 9, 0, 10), "fskhip_resampler_down_host: unknown sample format 9"),
                           (lambda: L_.fskhip_resampler_down_host(d._h, x.ctypes.data, 60, 60, None, out.ctypes.data, 1, 5, 10), "fskhip_resampler_down_host: unknown layout 5"),
                           (lambda: L_.fskhip_resampler_down_host(d._h, None, 60, 60, None, out.ctypes.data, 1, 0, 10), "fskhip_resampler_down_host: null buffer"),
                           (lambda: L_.fskhip_resampler_down_host(d._h, x.ctypes.data, 60, 59, None, out.ctypes.data, 1, 0, 10), "fskhip_resampler_down_host: float pitch 59 < 60 samples per stream"),
                           (lambda: L_.fskhip_resampler_down_host(d._h, x.ctypes.data, 60, 60, None, out.ctypes.data, 1, 0, 9), "fskhip_resampler_down_host: sample pitch 9 < 10 samples per stream"),
                           (lambda: L_.fskhip_resampler_down_host(d._h, x.ctypes.data, 60, 60, None, out.ctypes.data, 1, 1, 2), "fskhip_resampler_down_host: frame pitch 2 < n_streams 3"),
                           (lambda: L_.fskhip_resampler_down_host(d._h, x.ctypes.data, 60, 60, None, out.ctypes.data + 1, 1, 0, 10), "fskhip_resampler_down_host: a buffer is not aligned to its element size")):
            assert call() == _lib.E_INVALID and L_.fskhip_last_error().decode() == text
        # the wrong call for the handle is refused whatever its length; the right one with no samples does nothing
        assert L_.fskhip_resampler_up_host(d._h, None, 1, 0, 0, 0, None, 0) == _lib.E_INVALID
        assert L_.fskhip_last_error().decode() == "fskhip_resampler_up_host: the handle resamples down"
        assert L_.fskhip_resampler_down_host(d._h, None, 0, 0, None, None, 1, 0, 0) == 0 and L_.fskhip_resampler_up_host(u._h, None, 1, 0, 0, 0, None, 0) == 0
        assert np.array_equal(d.state(), before) and not u.state().any()
        assert d.process(np.zeros((S, 0), np.float32), "s16").shape == (S, 0) and np.array_equal(d.state(), before)
    finally:
        d.close()
        u.close()


def _cuts(total, unit, schedule):
    """the schedule's pieces in samples (`unit` per entry), 'rest' taking what is left"""
    fixed = sum(c for c in schedule if c != "rest") * unit
    return [(total - fixed) if c == "rest" else c * unit for c in schedule]


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("direction", ["up", "down"])
def test_any_cut_into_calls_is_one_call(direction, prec):
    wm = _wm()
    S, L, n = 65, 6, 1100                                                 # (low-rate samples; past one stream-major segment)
    for fmt, layout in (("mulaw", "stream"), ("s16", "sample")):
        for taps in (None, _taps(L, 13)):
            make = (lambda: wm.Upsampler(L, S, taps=taps, precision=_prec(prec))) if direction == "up" else (lambda: wm.Downsampler(L, S, taps=taps, precision=_prec(prec)))
            x = _narrow(fmt)[:S, :n] if direction == "up" else _wide()[:S, :n * L]
            unit = 1 if direction == "up" else L
            one = make()
            try:
                if direction == "up":
                    whole = one.process(x if layout == "stream" else np.ascontiguousarray(x.T), fmt, layout)
                else:
                    whole = one.process(x, fmt, layout)
                    whole = whole if layout == "stream" else whole.T
                state = one.state()
                assert state.shape == (S, one.history) and state.any()
                for schedule in ((1, 2, 37, "rest"), ("rest", 1)):
                    h = make()
                    try:
                        parts, at = [], 0
                        for c in _cuts(x.shape[1], unit, schedule):
                            piece = x[:, at:at + c]
                            at += c
                            if direction == "up":
                                parts.append(h.process(piece if layout == "stream" else np.ascontiguousarray(piece.T), fmt, layout))
                            else:
                                o = h.process(piece, fmt, layout)
                                parts.append(o if layout == "stream" else o.T)
                        got = np.concatenate(parts, axis=1)
                        assert at == x.shape[1] and np.array_equal(got, whole), (fmt, layout, schedule)
                        assert np.array_equal(h.state().view(np.uint32), state.view(np.uint32)), (fmt, layout, schedule)
                    finally:
                        h.close()
            finally:
                one.close()


@pytest.mark.parametrize("direction", ["up", "down"])
def test_reset_and_state_carry(direction):
    wm = _wm()
    S, L, n = 7, 3, 40
    taps = _taps(L, 13)
    make = (lambda: wm.Upsampler(L, S, taps=taps)) if direction == "up" else (lambda: wm.Downsampler(L, S, taps=taps))
    x = _narrow("s16")[:S, :2 * n] if direction == "up" else _wide()[:S, :2 * n * L]
    half = x.shape[1] // 2

    def run(h, a):
        return h.process(a, "s16")

    a, twin, fresh = make(), make(), make()
    try:
        first = run(a, x[:, :half])
        st = a.state()
        assert st.any(axis=1).all()
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


# ---- end to end: a 48 kHz engine behind and in front of 8 kHz trunk audio ------------------------------------------------------------
S_TRIP = 65


def _payloads():
    rng = np.random.default_rng(8000)
    return [bytes(rng.integers(0, 256, int(rng.integers(1, 41))).astype(np.uint8)) for _ in range(S_TRIP)]


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_round_trip_at_8_khz(prec):
    """Bell 202, 65 streams, random payloads of 1 .. 40 bytes, every trunk format and both layouts: every payload comes back"""
    wm = _wm()
    payloads = _payloads()
    tx, rx = wm.FSKEngine(S_TRIP, BELL, precision=_prec(prec)), wm.FSKEngine(S_TRIP, BELL, precision=_prec(prec))
    down, up = wm.Downsampler(6, S_TRIP, precision=_prec(prec)), wm.Upsampler(6, S_TRIP, precision=_prec(prec))
    try:
        assert len(down.taps) == 97 and up.taps == [6.0 * t for t in down.taps]
        for fmt in ("mulaw", "alaw", "s16"):
            for layout in LAYOUTS:
                for h in (down, up):
                    h.reset()
                rx.reset()
                samples, lens = tx.modulate_samples_at(payloads, fmt, layout, down)
                n = down.low_rate_length(tx.modulated_length(40))
                assert samples.dtype == sr.DTYPES[fmt] and samples.shape == ((S_TRIP, n) if layout == "stream" else (n, S_TRIP))
                assert lens.tolist() == [down.low_rate_length(tx.modulated_length(len(p))) for p in payloads]
                got, _eod = rx.demodulate_samples_at(samples, fmt, layout, up)
                assert got == payloads, (fmt, layout, [s for s in range(S_TRIP) if got[s] != payloads[s]])
    finally:
        for h in (tx, rx, down, up):
            h.close()


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_modulate_samples_at_is_the_decimated_float_call(prec):
    wm = _wm()
    payloads = _payloads()
    tx = wm.FSKEngine(S_TRIP, BELL, precision=_prec(prec))
    down = wm.Downsampler(6, S_TRIP, precision=_prec(prec))
    fir = wm.FIRFilterBatch(down.taps, S_TRIP, precision=_prec(prec))
    try:
        sigs = tx.modulate_data(payloads)
        n = down.low_rate_length(max(s.size for s in sigs))
        x = np.zeros((S_TRIP, n * 6), np.float32)
        for s, sig in enumerate(sigs):
            x[s, :sig.size] = sig
        y = fir.processBuffer(x)[:, ::6]
        for fmt in ("mulaw", "alaw", "s16", "f32"):
            want = sr.encode(y, fmt).view(BITS[fmt])
            for layout in LAYOUTS:
                down.reset()
                got, lens = tx.modulate_samples_at(payloads, fmt, layout, down)
                rows = got if layout == "stream" else np.ascontiguousarray(got.T)
                assert np.array_equal(rows.view(BITS[fmt]), want), (fmt, layout)
                assert lens.tolist() == [down.low_rate_length(s.size) for s in sigs]
                for s in range(S_TRIP):
                    assert (rows[s, lens[s]:].view(BITS[fmt]) == np.asarray(sr.silence(fmt)).view(BITS[fmt])).all()
        # a slab too short for the longest signal is the modulator's refusal
        before = down.state()
        with pytest.raises(wm.FskHipError) as ei:
            tx.modulate_samples_at(payloads, "s16", "stream", down, n_per_stream=100)
        from webaudio_modem_amd import _lib
        assert ei.value.code == _lib.E_OVERFLOW and np.array_equal(down.state(), before)      # ... made before the decimator runs
    finally:
        for h in (tx, down, fir):
            h.close()
