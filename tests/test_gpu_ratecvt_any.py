"""The rate converter's calls of any length on the GPU (include/fskhip_next.h: "Rate conversion in calls of any length";
csrc/fsk_ratecvt.hip: the ANY form of ratecvt_body).  Both directions, fp32 and fp64, s16 / mu-law / A-law / float, both layouts; ratios
3 / 2 and 2 / 3 with 7 and 8 taps, 160 / 147 and 147 / 160 with the default 2 561 taps; 1, 5 and 67 streams (a partly filled
64-stream tile behind a full one).

  1. a stream cut into calls of 1, M - 1, M + 1 and H - 1 samples, a call that writes nothing (where L < M), and one call long
     enough to span two workgroups in either layout equals, bit for bit, the existing whole-period call on a twin handle over the
     zero-padded stream, truncated; fp64 handles equal the model (tests/ratecvt_any_ref.py); state() and position are the model's
     after every call;
  2. three random cuts of the same stream give the same samples, state and position;
  3. a handle carried by hand with state() and position continues sample for sample; reset(s) zeroes one row and leaves the
     position; reset() returns the handle to creation;
  4. after process_any(5), process(k M) equals process_any(k M) on a twin and leaves the position;
  5. d_lens: garbage behind a stream's length does not show, the tail is the format's silence; one length ends inside the first
     partial period;
  6. refusals come in the header's order and leave state and position untouched; position_set(down) is refused; the whole-period
     processor call refuses a handle at a non-zero position."""
import numpy as np
import pytest

import ratecvt_any_ref as ra
import ratecvt_ref as rc
import samples_ref as sr

pytestmark = [pytest.mark.gpu]

DESIGNS = ((3, 2, 7), (2, 3, 8), (160, 147, 2561), (147, 160, 2561))
STREAMS = (1, 5, 67)
FORMATS = ("f32", "s16", "mulaw", "alaw")
LAYOUTS = ("stream", "sample")
BITS = {"f32": np.uint32, "s16": np.uint16, "mulaw": np.uint8, "alaw": np.uint8}
SMAX, NMAX = max(STREAMS), 6400

_CACHE = {}


def _wm():
    import webaudio_modem_amd as wm
    return wm


def _prec(name):
    wm = _wm()
    return wm.PRECISION_F64 if name == "f64" else wm.PRECISION_F32


def _taps(L, M, n_taps):
    if n_taps == 2561:
        return rc.default_taps(M * 300, L * 300)
    return np.random.default_rng(1000 * L + n_taps).uniform(-1.0, 1.0, n_taps)


def _narrow(fmt):
    """[SMAX, NMAX] samples of the format, made once and never written to"""
    if ("narrow", fmt) not in _CACHE:
        rng = np.random.default_rng(21)
        if fmt == "f32":
            a = rng.uniform(-1.2, 1.2, (SMAX, NMAX)).astype(np.float32)
        elif fmt == "s16":
            a = rng.integers(-32768, 32768, (SMAX, NMAX)).astype(np.int16)
        else:
            a = rng.integers(0, 256, (SMAX, NMAX)).astype(np.uint8)
        _CACHE[("narrow", fmt)] = a
    return _CACHE[("narrow", fmt)]


def _wide():
    if "wide" not in _CACHE:
        _CACHE["wide"] = np.random.default_rng(22).uniform(-1.2, 1.2, (SMAX, NMAX)).astype(np.float32)
    return _CACHE["wide"]


@pytest.fixture(scope="module", autouse=True)
def _drop_cache():
    yield
    _CACHE.clear()


def _length(L, M):
    """inputs of the cut stream: more than 4 (1024 / L) periods, one stream-major workgroup's (csrc/fsk_ratecvt_plan.h), which is
    more than the 64 / L periods of a sample-major one, and no whole number of periods"""
    n = (4 * max(1024 // L, 1) + 8) * M + M // 2 + 1
    assert n <= NMAX
    return n


def _make(direction, L, M, n_taps, S, prec):
    wm = _wm()
    cls = wm.CaptureConverter if direction == "capture" else wm.PlaybackConverter
    h = cls(M * 300, L * 300, S, taps=_taps(L, M, n_taps), precision=_prec(prec))
    assert (h.up, h.down, h.history, h.position) == (L, M, rc.history(L, n_taps), 0)
    return h


def _source(direction, fmt, S, N):
    """(what the calls take, [S, N]; the floats the converter sees)"""
    if direction == "capture":
        x = _narrow(fmt)[:S, :N]
        return x, sr.decode(x, fmt)
    return _wide()[:S, :N], _wide()[:S, :N]


def _run(h, direction, piece, fmt, layout, any_length=True, lens=None):
    """one host call on columns `piece` of the source; returns [S, n_out] whatever the layout"""
    fn = h.process_any if any_length else h.process
    if direction == "capture":
        return fn(piece if layout == "stream" else np.ascontiguousarray(piece.T), fmt, layout)
    o = fn(piece, fmt, layout, lens=lens)
    return o if layout == "stream" else np.ascontiguousarray(o.T)


def _whole(direction, prec, fmt, layout, L, M, n_taps, S, N):
    """the existing whole-period call on a fresh twin over the zero-padded stream, truncated to ceil(N L / M): made once per shape"""
    key = ("whole", direction, prec, fmt, layout, L, M, n_taps, S, N)
    if key not in _CACHE:
        src, _ = _source(direction, fmt, S, N)
        pad = np.zeros((S, -(-N // M) * M), src.dtype)      # (whatever the padding decodes to: the filter is causal, it cannot reach them)
        pad[:, :N] = src
        twin = _make(direction, L, M, n_taps, S, prec)
        try:
            _CACHE[key] = _run(twin, direction, pad, fmt, layout, any_length=False)[:, :ra.first_output(L, M, N)].copy()
        finally:
            twin.close()
    return _CACHE[key]


def _schedule(L, M, H, N):
    """the lengths of the cut: 1, M - 1, M + 1, H - 1, a call that writes nothing where there is one (L < M; a call in front of it
    brings the position there), the long call that spans two workgroups, and a tail of 5"""
    lens, pos = [], 0
    for n in (1, M - 1, M + 1, H - 1):
        if n > 0:
            lens.append(n)
            pos = (pos + n) % M
    if L < M:
        d = next(d for d in range(M) if ra.out_count_any(L, M, (pos + d) % M, 1) == 0)
        lens += [d, 1] if d else [1]
    lens += [N - sum(lens) - 5, 5]
    assert all(n > 0 for n in lens) and sum(lens) == N and lens[-2] > 4 * max(1024 // L, 1) * M
    return lens


def _view(a, direction, fmt):
    return np.ascontiguousarray(a).view(np.uint32 if direction == "capture" else BITS[fmt])


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("direction", ["capture", "playback"])
def test_cut_against_a_whole_period_twin(direction, prec, fmt, layout):
    zero_calls = 0
    for i, (L, M, n_taps) in enumerate(DESIGNS):
        N, H = _length(L, M), rc.history(L, n_taps)
        sched = _schedule(L, M, H, N)
        for S in STREAMS:
            if n_taps == 2561 and S == 5 and (i + FORMATS.index(fmt)) % 2:
                continue                                                 # (the long designs take 5 streams with every other format)
            src, floats = _source(direction, fmt, S, N)
            want = _whole(direction, prec, fmt, layout, L, M, n_taps, S, N)
            padded = np.concatenate([np.zeros((S, H), np.float32), floats], axis=1)
            h = _make(direction, L, M, n_taps, S, prec)
            try:
                parts, at = [], 0
                for n in sched:
                    assert h.out_count_any(n) == ra.out_count_any(L, M, at % M, n)
                    y = _run(h, direction, src[:, at:at + n], fmt, layout)
                    assert y.shape == (S, ra.out_count_any(L, M, at % M, n)), (L, M, S, at, n, y.shape)
                    zero_calls += y.shape[1] == 0
                    parts.append(y)
                    at += n
                    assert h.position == at % M and np.array_equal(h.state().view(np.uint32), padded[:, at:at + H].view(np.uint32)), (L, M, S, at, n)
                got = np.concatenate(parts, axis=1)
                assert got.shape == want.shape
                bad = np.argwhere(_view(got, direction, fmt) != _view(want, direction, fmt))
                assert bad.size == 0, "%s %s %s %s %d/%d S=%d: %d elements differ from the twin's, first at %r (cuts %r)" % (
                    direction, prec, fmt, layout, L, M, S, len(bad), bad[0].tolist(), sched)
                if prec == "f64":
                    model = ra.convert_whole(floats, _taps(L, M, n_taps), L, M)
                    model = model if direction == "capture" else sr.encode(model, fmt)
                    assert np.array_equal(_view(got, direction, fmt), _view(model, direction, fmt)), (L, M, S)
            finally:
                h.close()
    assert zero_calls >= 2                                                # (2 / 3 and 147 / 160 each had their call that writes nothing)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("direction", ["capture", "playback"])
def test_any_cut_is_one_call(direction, prec):
    rng = np.random.default_rng(7)
    for (L, M, n_taps), (fmt, layout), S in zip(DESIGNS, (("mulaw", "stream"), ("s16", "sample"), ("alaw", "sample"), ("f32", "stream")), (5, 67, 67, 67)):
        N = _length(L, M)
        src, _ = _source(direction, fmt, S, N)
        one = _make(direction, L, M, n_taps, S, prec)
        try:
            whole = _run(one, direction, src, fmt, layout)                # one call of N, no multiple of M
            state, pos = one.state(), one.position
            assert pos == N % M and state.any()
            assert np.array_equal(_view(whole, direction, fmt), _view(_whole(direction, prec, fmt, layout, L, M, n_taps, S, N), direction, fmt))
            for _ in range(3):
                cuts = [0] + sorted(set(rng.choice(np.arange(1, N), size=6, replace=False).tolist())) + [N]
                h = _make(direction, L, M, n_taps, S, prec)
                try:
                    parts = [_run(h, direction, src[:, a:b], fmt, layout) for a, b in zip(cuts[:-1], cuts[1:])]
                    assert np.array_equal(_view(np.concatenate(parts, axis=1), direction, fmt), _view(whole, direction, fmt)), (L, M, cuts)
                    assert h.position == pos and np.array_equal(h.state().view(np.uint32), state.view(np.uint32)), (L, M, cuts)
                finally:
                    h.close()
        finally:
            one.close()


@pytest.mark.parametrize("direction", ["capture", "playback"])
def test_position_and_reset(direction):
    S, fmt = 7, "s16"
    for L, M, n_taps in ((3, 2, 7), (147, 160, 2561)):
        N = 5 * M + 3
        src, _ = _source(direction, fmt, S, 2 * N)
        a, twin, fresh = (_make(direction, L, M, n_taps, S, "f32") for _ in range(3))
        try:
            first = _run(a, direction, src[:, :N], fmt, "stream")
            st, pos = a.state(), a.position
            assert pos == N % M and pos != 0 and st.any(axis=1).all()
            # carried by hand: state() and position on a twin continue sample for sample
            twin.set_state(st)
            twin.position = pos
            assert twin.position == pos
            cont = _run(a, direction, src[:, N:], fmt, "stream")
            assert np.array_equal(_run(twin, direction, src[:, N:], fmt, "stream"), cont)
            assert twin.position == a.position == 2 * N % M and np.array_equal(twin.state(), a.state())
            whole = _run(fresh, direction, src, fmt, "stream")
            assert np.array_equal(np.concatenate([first, cont], axis=1), whole)
            # without the position the twin would have been on another grid
            with pytest.raises(ValueError):
                twin.position = M
            with pytest.raises(ValueError):
                twin.position = -1
            # reset(s) zeroes one row and leaves the position: that stream goes on as one that has received zeros
            a.reset()
            fresh.reset()
            assert a.position == 0 and not a.state().any()
            _run(a, direction, src[:, :N], fmt, "stream")
            a.reset(2)
            after = a.state()
            assert a.position == pos and not after[2].any() and np.array_equal(np.delete(after, 2, 0), np.delete(st, 2, 0))
            cont2 = _run(a, direction, src[:, N:], fmt, "stream")
            assert np.array_equal(np.delete(cont2, 2, 0), np.delete(cont, 2, 0))
            zeros = src.copy()
            zeros[:, :N] = 0
            assert np.array_equal(_run(fresh, direction, zeros, fmt, "stream")[2, first.shape[1]:], cont2[2])
            # reset() returns the handle to creation
            a.reset()
            assert a.position == 0 and not a.state().any()
            assert np.array_equal(_run(a, direction, src, fmt, "stream"), whole)
        finally:
            for h in (a, twin, fresh):
                h.close()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("direction", ["capture", "playback"])
def test_existing_calls_at_a_position(direction, layout):
    for (L, M, n_taps), S, fmt, prec in (((3, 2, 7), 5, "s16", "f32"), ((160, 147, 2561), 67, "mulaw", "f64"), ((147, 160, 2561), 67, "f32", "f32")):
        k = 4 * max(1024 // L, 1) + 2                                     # (past one workgroup in either layout)
        src, _ = _source(direction, fmt, S, 5 + k * M)
        a, b = _make(direction, L, M, n_taps, S, prec), _make(direction, L, M, n_taps, S, prec)
        try:
            for h in (a, b):
                _run(h, direction, src[:, :5], fmt, layout)
            assert a.position == b.position == 5 % M
            got = _run(a, direction, src[:, 5:], fmt, layout, any_length=False)
            want = _run(b, direction, src[:, 5:], fmt, layout)
            assert got.shape == (S, k * L) and np.array_equal(_view(got, direction, fmt), _view(want, direction, fmt)), (L, M)
            assert a.position == b.position == 5 % M and np.array_equal(a.state().view(np.uint32), b.state().view(np.uint32))
        finally:
            a.close()
            b.close()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_playback_lens_hide_what_lies_behind_a_stream(fmt, layout):
    wm = _wm()
    S, L, M, lead, n = 67, 147, 160, 73, 160 * 9 + 51
    x = _wide()[:S, lead:lead + n].copy()
    # (3: inside the first partial period, which ends 160 - 73 = 87 inputs into the call)
    lens = np.array([(0, 1, 3, 86, 87, 480, n - 1, n, n + 80)[s % 9] for s in range(S)], np.uint32)
    clean = np.where(np.arange(n)[None, :] < lens[:, None].astype(np.int64), x, np.float32(0.0))
    for prec in (wm.PRECISION_F32, wm.PRECISION_F64):
        a, b = wm.PlaybackConverter(48000, 44100, S, precision=prec), wm.PlaybackConverter(48000, 44100, S, precision=prec)
        try:
            for h in (a, b):
                h.process_any(_wide()[:S, :lead], fmt, layout)
            assert a.position == lead and a.history == 18
            before = a.state()
            got = a.process_any(x, fmt, layout, lens=lens)                # garbage behind every length ...
            want = b.process_any(clean, fmt, layout)                      # ... against zeros there
            n_out = ra.out_count_any(L, M, lead, n)
            assert got.shape == want.shape == ((S, n_out) if layout == "stream" else (n_out, S))
            assert np.array_equal(got.view(BITS[fmt]), want.view(BITS[fmt]))
            state = a.state()
            assert np.array_equal(state, b.state()) and a.position == b.position == (lead + n) % M
            rows = got if layout == "stream" else got.T
            q0 = ra.first_output(L, M, lead)
            for s in range(S):
                # the last output that a sample of the stream reaches, on the grid; behind it the format's silence
                end = rc.out_length(L, M, 2561, lead + min(int(lens[s]), n)) - q0
                assert (np.ascontiguousarray(rows[s, max(end, 0):]).view(BITS[fmt]) == np.asarray(sr.silence(fmt)).view(BITS[fmt])).all(), s
                assert not state[s, max(0, 18 - (n - min(int(lens[s]), n))):].any()
            if prec == wm.PRECISION_F64:
                model, hist, pos = ra.playback_any(x, a.taps, L, M, fmt, lens=lens, pos=lead, hist=before)
                assert np.array_equal(np.ascontiguousarray(rows).view(BITS[fmt]), model.view(BITS[fmt])) and np.array_equal(state, hist) and pos == a.position
        finally:
            a.close()
            b.close()


def test_refused_calls_in_order_leave_state_and_position():
    wm = _wm()
    from webaudio_modem_amd import _lib
    S = 3
    p, c, c2 = wm.PlaybackConverter(3, 2, S, taps=_taps(2, 3, 8)), wm.CaptureConverter(2, 3, S, taps=_taps(3, 2, 7)), wm.CaptureConverter(3, 2, S, taps=_taps(2, 3, 8))
    eng = wm.FSKEngine(S, {})
    proc = wm.FSKProcessorBatch(eng)
    try:
        assert (p.up, p.down, c.up, c.down) == (2, 3, 3, 2)
        x = _wide()[:S, :61].copy()
        assert p.process_any(x, "s16").shape == (S, 41)
        before, pos = p.state(), p.position
        assert before.any() and pos == 1
        out = np.zeros((S, 64), np.int16)
        n_out = np.full(1, 77, np.uint64)
        L_, X, O, NO = p._L, x.ctypes.data, out.ctypes.data, n_out.ctypes.data
        # from position 1 a call of 61 writes ceil(62 * 2 / 3) - 1 = 41; each call is wrong in everything behind what it is refused for as well
        for call, text in ((lambda: L_.fskhip_ratecvt_playback_any_host(p._h, None, 61, 0, None, None, 9, 5, 0, NO), "fskhip_ratecvt_playback_any_host: unknown sample format 9"),
                           (lambda: L_.fskhip_ratecvt_playback_any_host(p._h, None, 61, 0, None, None, 1, 5, 0, NO), "fskhip_ratecvt_playback_any_host: unknown layout 5"),
                           (lambda: L_.fskhip_ratecvt_playback_any_host(c2._h, None, 61, 0, None, O + 1, 1, 0, 0, NO), "fskhip_ratecvt_playback_any_host: null buffer"),
                           (lambda: L_.fskhip_ratecvt_playback_any_host(c2._h, X, 61, 60, None, O + 1, 1, 0, 0, NO), "fskhip_ratecvt_playback_any_host: float pitch 60 < 61 samples per stream"),
                           (lambda: L_.fskhip_ratecvt_playback_any_host(p._h, X, 61, 61, None, O + 1, 1, 0, 40, NO), "fskhip_ratecvt_playback_any_host: sample pitch 40 < 41 samples per stream"),
                           (lambda: L_.fskhip_ratecvt_playback_any_host(c2._h, X, 61, 61, None, O + 1, 1, 1, 2, NO), "fskhip_ratecvt_playback_any_host: frame pitch 2 < n_streams 3"),
                           (lambda: L_.fskhip_ratecvt_playback_any_host(c2._h, X, 61, 61, None, O + 1, 1, 0, 64, NO), "fskhip_ratecvt_playback_any_host: a buffer is not aligned to its element size"),
                           (lambda: L_.fskhip_ratecvt_playback_any_host(c2._h, X, 61, 61, None, O, 1, 0, 64, NO), "fskhip_ratecvt_playback_any_host: the handle converts for capture"),
                           (lambda: L_.fskhip_ratecvt_capture_any_host(p._h, O, 1, 0, 7, 7, X, 60, NO), "fskhip_ratecvt_capture_any_host: the handle converts for playback"),
                           (lambda: L_.fskhip_ratecvt_capture_any_host(c._h, O, 1, 0, 7, 7, X, 10, NO), "fskhip_ratecvt_capture_any_host: float pitch 10 < 11 samples per stream"),
                           (lambda: L_.fskhip_ratecvt_capture_any_host(c._h, O, 1, 0, 7, 6, X, 11, NO), "fskhip_ratecvt_capture_any_host: sample pitch 6 < 7 samples per stream"),
                           # the existing calls still want their multiple, in the existing words
                           (lambda: L_.fskhip_ratecvt_playback_host(p._h, X, 61, 61, None, O, 1, 0, 64), "fskhip_ratecvt_playback_host: n_in 61 is not a multiple of the down factor 3"),
                           (lambda: L_.fskhip_ratecvt_position_set(p._h, 3), "fskhip_ratecvt_position_set: position 3 is not below the down factor 3")):
            assert call() == _lib.E_INVALID and L_.fskhip_last_error().decode() == text
        assert n_out[0] == 77                                             # (a refused call reports nothing)
        # the wrong call for the handle is refused whatever its length; the right one with no samples does nothing and reports 0
        assert L_.fskhip_ratecvt_capture_any_host(p._h, None, 1, 0, 0, 0, None, 0, NO) == _lib.E_INVALID
        assert L_.fskhip_last_error().decode() == "fskhip_ratecvt_capture_any_host: the handle converts for playback"
        assert L_.fskhip_ratecvt_playback_any_host(p._h, None, 0, 0, None, None, 1, 0, 0, NO) == 0 and n_out[0] == 0
        assert np.array_equal(p.state(), before) and p.position == pos and not c.state().any() and c.position == 0 and c2.position == 0
        assert p.process_any(np.zeros((S, 0), np.float32), "s16").shape == (S, 0) and np.array_equal(p.state(), before) and p.position == pos
        # a call that is not refused reports what it wrote; NULL is taken as well
        assert L_.fskhip_ratecvt_playback_any_host(p._h, X, 4, 61, None, O, 1, 0, 64, NO) == 0 and n_out[0] == ra.out_count_any(2, 3, 1, 4) == 3
        assert L_.fskhip_ratecvt_playback_any_host(p._h, X, 1, 61, None, O, 1, 0, 64, None) == 0 and p.position == 0
        # the whole-period processor call wants its handles at a period boundary, behind everything else it refuses
        cap, play = wm.CaptureConverter(2, 3, S, taps=_taps(3, 2, 7)), wm.PlaybackConverter(3, 2, S, taps=_taps(2, 3, 8))
        try:
            cap.process_any(np.zeros((S, 1), np.int16), "s16")
            st = cap.state()
            with pytest.raises(wm.FskHipError, match="fskhip_processor_process_ratecvt_host: the capture handle is at position 1, not at a period boundary") as ei:
                proc.process_samples_at(np.zeros((S, 4), np.int16), "s16", "stream", cap)
            assert ei.value.code == _lib.E_INVALID
            with pytest.raises(wm.FskHipError, match="n_in 5 is not a multiple of the capture handle's down factor 2"):
                _lib.check(proc._L.fskhip_processor_process_ratecvt_host(proc._h, cap._h, None, out.ctypes.data, 1, 0, 5, 8, None, 1, 0, 0, 0, 0))
            play.process_any(np.zeros((S, 2), np.float32), "s16")
            assert play.position == 2
            with pytest.raises(wm.FskHipError, match="fskhip_processor_process_ratecvt_host: the playback handle is at position 2, not at a period boundary"):
                proc.process_samples_at(None, n_out=4, out_fmt="s16", out_layout="stream", downsampler=play)
            assert cap.position == 1 and play.position == 2 and np.array_equal(cap.state(), st)
        finally:
            cap.close()
            play.close()
    finally:
        for h in (p, c, c2):
            h.close()
        proc.close()
        eng.close()
