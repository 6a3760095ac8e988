"""The encode direction of the capture formats on the GPU (include/fskhip.h: fskhip_egress_device, fskhip_modulate_host_fmt;
csrc/fsk_samples.hip).

  * the egress kernel against numpy (tests/samples_ref.py, held against audioop in test_egress_cpu.py), BIT FOR BIT, for every format x
    layout: every value k / 32768, the rounding ties, the edges of the float range, stream counts and lengths around the 64 x 64 tile,
    the 16-byte vector and the per-workgroup span, every destination offset within 16 bytes, every source offset within a float4,
    pitches wider than the rows, with and without ragged per-stream lengths -- and the whole destination compared, sentinels
    included: nothing else is written;
  * FSKEngine.modulate_samples == samples_ref.encode of what fskhip_modulate_host returns, silence from lens[s] on, fp32 and fp64
    engines, ragged payloads, one, two and three 64-stream groups; the overflow refusal;
  * the round trip modulate_samples -> demodulate_samples through every trunk format and layout;
  * two engines writing their column blocks of one array of interleaved frames."""
import numpy as np
import pytest

import samples_ref as er

pytestmark = [pytest.mark.gpu]

BELL = dict(baudRate=1200, markFrequency=1200, spaceFrequency=2200)
SPAN = 8192                                   # elements of a row per workgroup of the stream-major kernel (csrc/fsk_samples.hip: kEgressSpan)
STREAMS = (1, 63, 64, 65, 130)
LENGTHS = (1, 3, 4, 5, 15, 16, 17, 63, 64, 65, SPAN + 7)
CORE = {(S, n) for S in (1, 65) for n in (5, 17, 65, SPAN + 7)}   # shapes that take EVERY destination offset x source offset
MARGIN = 16                                   # elements in front of and behind the destination's used span (keeps its alignment)
SENTINEL = {"f32": np.uint32(0x7FC5E417), "s16": np.uint16(0x5A5B), "mulaw": np.uint8(0xA5), "alaw": np.uint8(0xA5)}
BITS = {"f32": np.uint32, "s16": np.uint16, "mulaw": np.uint8, "alaw": np.uint8}    # the element as plain bits
FORMATS = ("f32", "s16", "mulaw", "alaw")
LAYOUTS = ("stream", "sample")


def _wm():
    import webaudio_modem_amd as wm
    return wm


@pytest.fixture(scope="module")
def eng():
    e = _wm().FSKEngine(1, {})
    yield e
    e.close()


_POOL = {}


def _pool():
    """float32 values, made once and never written to: the edges, every k / 32768, every tie (k + 0.5) / 32768, then random floats in
    +-1.2 (arbitrary mantissas) -- long enough for the largest shape, which therefore converts every one of them"""
    if "x" not in _POOL:
        rng = np.random.default_rng(5)
        edges = np.array([np.inf, -np.inf, np.nan, -0.0, 0.0, 1.0, -1.0, 1.0 + 2.0 ** -23, -(1.0 + 2.0 ** -23), 1e-45, -1e-45, 3.4e38, -3.4e38,
                          32767.5 / 32768, -32768.5 / 32768, 0.5 / 32768, -0.5 / 32768, 1.5 / 32768, -1.5 / 32768, 2.5 / 32768], np.float32)
        every = (np.arange(-32768, 32768, dtype=np.float64) / 32768.0).astype(np.float32)
        ties = ((np.arange(-33000, 33000, dtype=np.float64) + 0.5) / 32768.0).astype(np.float32)
        need = 3 + (max(STREAMS) - 1) * (((SPAN + 7 + 15) & ~15) + 16) + SPAN + 7
        rest = rng.uniform(-1.2, 1.2, need - edges.size - every.size - ties.size).astype(np.float32)
        mixed = np.concatenate([every, ties, rest])
        rng.shuffle(mixed)                     # (so that short rows meet ties and large values too)
        _POOL["x"] = np.concatenate([edges, mixed])
    return _POOL["x"]


def _encoded(fmt):
    """the pool in the format, as plain bits -- computed once per format"""
    if fmt not in _POOL:
        _POOL[fmt] = np.ascontiguousarray(er.encode(_pool(), fmt)).view(BITS[fmt])
    return _POOL[fmt]


def _ragged(S, n, rot):
    """per-stream lengths with 0, 1, n, n - 1 and values above n among them, whatever S is"""
    pat = (n // 2, 0, n + 3, 1, n, max(n - 1, 0), 2 * n + 1, min(7, n))
    return np.array([pat[(s + rot) % 8] for s in range(S)], np.uint32)


class _Device:
    """the source pool, a lengths array and one destination buffer on the device, for many launches"""

    def __init__(self, eng, fmt, dst_elems):
        self.eng, self.fmt, self.cap = eng, fmt, dst_elems
        pool = _pool()
        self.n_src = pool.size
        self.esz = np.dtype(BITS[fmt]).itemsize
        self.d_src = eng.device_malloc(pool.nbytes)
        self.d_lens = eng.device_malloc(4 * max(STREAMS))
        self.d_dst = eng.device_malloc(dst_elems * self.esz)
        eng.h2d(self.d_src, pool)
        self.fill = np.full(dst_elems, SENTINEL[fmt], BITS[fmt])
        self.got = np.zeros(dst_elems, BITS[fmt])

    def run(self, layout, S, n, src_off, src_pitch, lens, dst_off, dst_pitch):
        """(destination after one launch into sentinels, what it has to be) -- both over the used span and its margins"""
        rows, cols = (S, n) if layout == "stream" else (n, S)
        used = MARGIN + dst_off + (rows - 1) * dst_pitch + cols + MARGIN
        # the launch stays inside both buffers: checked here, before anything runs
        assert src_off + (S - 1) * src_pitch + n <= self.n_src and used <= self.cap and src_pitch >= n and dst_pitch >= cols
        self.eng.h2d(self.d_dst, self.fill[:used])
        if lens is not None:
            self.eng.h2d(self.d_lens, lens)
        _wm().egress_device(self.d_src + 4 * src_off, src_pitch, None if lens is None else self.d_lens, S, n, self.fmt, layout,
                            self.d_dst + (MARGIN + dst_off) * self.esz, dst_pitch)
        self.eng.synchronize()
        got = self.got[:used]
        self.eng.d2h(got, self.d_dst)
        enc = np.lib.stride_tricks.as_strided(_encoded(self.fmt)[src_off:], shape=(S, n), strides=(src_pitch * self.esz, self.esz))
        if lens is not None:
            enc = np.where(np.arange(n)[None, :] < lens[:, None].astype(np.int64), enc, np.asarray(er.silence(self.fmt)).view(BITS[self.fmt]))
        want = self.fill[:used].copy()
        view = np.lib.stride_tricks.as_strided(want[MARGIN + dst_off:], shape=(rows, cols), strides=(dst_pitch * self.esz, self.esz))
        view[...] = enc if layout == "stream" else enc.T
        return got, want

    def close(self):
        for p in (self.d_src, self.d_lens, self.d_dst):
            self.eng.device_free(p)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_egress_kernel_bit_for_bit(eng, fmt, layout):
    esz = np.dtype(BITS[fmt]).itemsize
    E = 16 // esz                                          # destination offsets within 16 bytes
    smax, nmax = max(STREAMS), max(LENGTHS)
    cap = 2 * MARGIN + E + (max(smax, 64) + 32) * (nmax + 32)
    dev = _Device(eng, fmt, cap)
    launches = i = 0
    seen_dst, seen_src = set(), set()
    try:
        for S in STREAMS:
            for n in LENGTHS:
                cols = n if layout == "stream" else S
                # pitches wider than the rows: odd ones, and ones that keep every row at the first row's alignment
                for src_pitch, dst_pitch in ((n + 5, cols + 3), (((n + 15) & ~15) + 16, ((cols + 15) & ~15) + 16)):
                    if (S, n) in CORE:
                        offsets = [(d, s) for d in range(E) for s in range(4)]
                    else:                                  # two of them, walking through all as the shapes go by
                        offsets = [(i % E, (i // E + i) % 4), ((i + E // 2 + 1) % E, (i // E + i + 2) % 4)]
                        i += 1
                    for dst_off, src_off in offsets:
                        for lens in (None, _ragged(S, n, launches)):
                            got, want = dev.run(layout, S, n, src_off, src_pitch, lens, dst_off, dst_pitch)
                            bad = np.flatnonzero(got != want)
                            assert bad.size == 0, "%s %s S=%d n=%d src +%d pitch %d, dst +%d pitch %d, lens %s: %d elements differ, first at %d (got %#x, want %#x)" % (
                                fmt, layout, S, n, src_off, src_pitch, dst_off, dst_pitch, None if lens is None else lens[:8].tolist(), bad.size,
                                bad[0] - MARGIN - dst_off, got[bad[0]], want[bad[0]])
                            launches += 1
                        seen_dst.add(dst_off)
                        seen_src.add(src_off)
    finally:
        dev.close()
    assert seen_dst == set(range(E)) and seen_src == set(range(4))
    assert launches == 2 * 2 * (len(CORE) * 4 * E + (len(STREAMS) * len(LENGTHS) - len(CORE)) * 2)


# ---- FSKEngine.modulate_samples == encode(fskhip_modulate_host) --------------------------------------------------------------------
def _ragged_payloads(S):
    """0 .. 11 bytes, the first one empty"""
    return [bytes((s * 31 + 7 * i + 1) & 0xFF for i in range((s * 7) % 12)) for s in range(S)]


def _modulate_host(e, payloads, n):
    """fskhip_modulate_host into float32 [S, n] -> (rows, lens)"""
    from webaudio_modem_amd.engine import payload_args
    pay, lens, ppitch = payload_args(payloads)
    out, out_lens = np.zeros((e.n_streams, n), np.float32), np.zeros(e.n_streams, np.uint32)
    rc = e._L.fskhip_modulate_host(e._h, pay.ctypes.data, lens.ctypes.data, ppitch, out.ctypes.data, n, out_lens.ctypes.data)
    assert rc == 0, e._L.fskhip_last_error()
    return out, out_lens


@pytest.mark.parametrize("S", [1, 65, 130])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_modulate_samples_is_the_encoded_float_call(prec, S):
    wm = _wm()
    from webaudio_modem_amd import _lib
    e = wm.FSKEngine(S, {}, precision=wm.PRECISION_F64 if prec == "f64" else wm.PRECISION_F32)
    try:
        payloads = _ragged_payloads(S)
        n = e.modulated_length(max(len(p) for p in payloads))
        floats, lens = _modulate_host(e, payloads, n)
        assert lens.max() == n and lens.tolist() == [e.modulated_length(len(p)) for p in payloads]
        live = np.arange(n)[None, :] < lens[:, None].astype(np.int64)
        for fmt in FORMATS:
            want = np.where(live, er.encode(floats, fmt).view(BITS[fmt]), np.asarray(er.silence(fmt)).view(BITS[fmt]))
            for layout in LAYOUTS:
                got, got_lens = e.modulate_samples(payloads, fmt, layout)
                assert got.dtype == er.DTYPES[fmt] and got.shape == ((S, n) if layout == "stream" else (n, S))
                rows = got if layout == "stream" else got.T
                assert np.array_equal(got_lens, lens), (fmt, layout)
                assert np.array_equal(rows.view(BITS[fmt]) if layout == "stream" else np.ascontiguousarray(rows).view(BITS[fmt]), want), (fmt, layout)
                # a longer call into a wider array: silence behind every signal, the array's other columns untouched
                wide = np.full((S, n + 13 + 5) if layout == "stream" else (n + 13, S + 5), SENTINEL[fmt], BITS[fmt]).view(er.DTYPES[fmt])
                view = wide[:, :n + 13] if layout == "stream" else wide[:, :S]
                got2, _ = e.modulate_samples(payloads, fmt, layout, n_per_stream=n + 13, out=view)
                assert got2 is view
                bits = wide.view(BITS[fmt])
                rows2 = bits[:, :n + 13] if layout == "stream" else bits[:, :S].T
                assert np.array_equal(rows2[:, :n], want) and (rows2[:, n:] == np.asarray(er.silence(fmt)).view(BITS[fmt])).all(), (fmt, layout)
                assert (bits[:, n + 13:] == SENTINEL[fmt]).all() if layout == "stream" else (bits[:, S:] == SENTINEL[fmt]).all()
        # f32 stream-major IS fskhip_modulate_host's output, byte for byte, for t < lens[s]
        got, _ = e.modulate_samples(payloads, "f32", "stream")
        assert np.array_equal(got.view(np.uint32)[live], floats.view(np.uint32)[live])
        # one sample short of the longest signal: the float call's refusal, and the true lengths all the same
        from webaudio_modem_amd.engine import payload_args
        pay, plens, ppitch = payload_args(payloads)
        for fmt, lay in ((_lib.SAMPLES_S16, 0), (_lib.SAMPLES_MULAW, 1)):
            out = np.zeros(S * n, er.DTYPES["s16" if fmt == _lib.SAMPLES_S16 else "mulaw"])
            out_lens = np.zeros(S, np.uint32)
            rc = e._L.fskhip_modulate_host_fmt(e._h, pay.ctypes.data, plens.ctypes.data, ppitch, fmt, lay, out.ctypes.data, n - 1, S if lay else n,
                                               out_lens.ctypes.data)
            assert rc == _lib.E_OVERFLOW and "needs %d samples, slab holds %d" % (n, n - 1) in e._L.fskhip_last_error().decode()
            assert np.array_equal(out_lens, lens)
        with pytest.raises(wm.FskHipError) as ei:
            e.modulate_samples(payloads, "alaw", "sample", n_per_stream=n - 1)
        assert ei.value.code == _lib.E_OVERFLOW
    finally:
        e.close()


# ---- modulate_samples -> demodulate_samples ----------------------------------------------------------------------------------------
S_TRIP = 65


def _payload(s):
    return bytes(0x41 + (s * 5 + 3 * i) % 26 for i in range(16))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("fmt", ["s16", "mulaw", "alaw"])
def test_round_trip_through_the_trunk_formats(fmt, layout):
    """Bell 202 at 48 kHz, 65 streams, one 16-byte frame each, no stream excused.  The payload list was fixed after running the same
    chain on the CPU: oracle.pyoracle modulate -> samples_ref.encode -> samples_ref.decode -> oracle demodulate returns every one of
    these 65 payloads exactly through s16, mu-law and A-law (and f32), with the signal as modulateData returns it and with 1000
    further samples of encoded silence behind it; none had to be dropped."""
    wm = _wm()
    payloads = [_payload(s) for s in range(S_TRIP)]
    tx, rx = wm.FSKEngine(S_TRIP, BELL), wm.FSKEngine(S_TRIP, BELL)
    try:
        samples, lens = tx.modulate_samples(payloads, fmt, layout)
        assert samples.dtype == er.DTYPES[fmt] and (lens == tx.modulated_length(16)).all()
        got, _eod = rx.demodulate_samples(samples, fmt=fmt, layout=layout)
        assert got == payloads
    finally:
        tx.close()
        rx.close()


# ---- column blocks of one array of interleaved frames ------------------------------------------------------------------------------
@pytest.mark.parametrize("pitch", [128, 130])
def test_two_engines_write_their_column_blocks_of_one_frame_array(pitch):
    wm = _wm()
    payloads = _ragged_payloads(128)
    one, a, b = wm.FSKEngine(128, {}), wm.FSKEngine(65, {}), wm.FSKEngine(63, {})
    try:
        n = one.modulated_length(11)
        for fmt in ("s16", "alaw"):
            want, want_lens = one.modulate_samples(payloads, fmt, "sample")
            frames = np.full((n, pitch), SENTINEL[fmt], BITS[fmt]).view(er.DTYPES[fmt])
            _, la = a.modulate_samples(payloads[:65], fmt, "sample", n_per_stream=n, out=frames[:, :65])
            _, lb = b.modulate_samples(payloads[65:], fmt, "sample", n_per_stream=n, out=frames[:, 65:128])
            assert np.array_equal(frames[:, :128], want) and np.array_equal(np.concatenate([la, lb]), want_lens)
            assert (frames.view(BITS[fmt])[:, 128:] == SENTINEL[fmt]).all()       # (pitch 130: the columns beyond n_streams)
        # ... which is what the sharded engine does with them
        sh = wm.FSKEngineSharded(128, {}, devices=[0, 0])
        try:
            frames = np.full((n, pitch), SENTINEL["s16"], np.uint16).view(np.int16)
            got, lens = sh.modulate_samples(payloads, "s16", "sample", out=frames[:, :128])
            want, want_lens = one.modulate_samples(payloads, "s16", "sample")
            assert np.array_equal(got, want) and np.array_equal(lens, want_lens) and (frames.view(np.uint16)[:, 128:] == SENTINEL["s16"]).all()
        finally:
            sh.close()
    finally:
        for e in (one, a, b):
            e.close()
