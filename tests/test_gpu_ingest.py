"""Capture formats on the GPU (include/fskhip.h: fskhip_ingest_device, fskhip_demodulate_host_fmt; csrc/fsk_samples.hip).

  * the ingest kernel against numpy (tests/samples_ref.py, held against audioop in test_ingest_cpu.py), BIT FOR BIT -- every value is
    an integer of at most 16 bits times 2^-15, exact in float32 -- for every format x layout, stream counts and lengths around
    the 64 x 64 tile and the four-element quad, every source and destination alignment, pitches that are no multiple of four;
    and nothing written outside [0, n) of a row;
  * every int16 value and every G.711 code;
  * fskhip_demodulate_host_fmt == converting on the host and calling fskhip_demodulate_host: bytes, counts, 'eod' counts per call,
    the status and every state word of every stream, directly and through the time pipeline, mid decimator-pair included;
  * the write-back flag's refusal, the Python argument checks, the sharded mirror."""

import numpy as np
import pytest

import samples_ref as ir

pytestmark = [pytest.mark.gpu]

SENTINEL = np.uint32(0x7FC5E417)   # a NaN no decode produces
MARGIN = 8                         # floats in front of and behind the destination's used span (32 bytes: keeps its alignment)
BELL = dict(baudRate=1200, markFrequency=1200, spaceFrequency=2200)
STREAMS = (1, 3, 64, 65, 130)
LENGTHS = (0, 1, 3, 15, 16, 17, 63, 64, 65, 257)
CHUNK = 4096                       # samples of a row per workgroup of the stream-major kernel (csrc/fsk_samples.hip: kIngestChunk)
LONG_STREAMS = (1, 3)              # the batches that also take rows of CHUNK + 7 samples, stream-major: workgroups c > 0 at every alignment


def _wm():
    import webaudio_modem_amd as wm
    return wm


@pytest.fixture(scope="module")
def eng():
    e = _wm().FSKEngine(1, {})
    yield e
    e.close()


def _pool(fmt, count, seed):
    """`count` random elements of the format: every int16 / every code appears; floats are arbitrary bit patterns"""
    rng = np.random.default_rng(seed)
    if fmt == "f32":
        return rng.integers(0, 1 << 32, count, dtype=np.uint64).astype(np.uint32).view(np.float32)
    if fmt == "s16":
        return rng.integers(-32768, 32768, count, dtype=np.int32).astype(np.int16)
    return rng.integers(0, 256, count, dtype=np.int32).astype(np.uint8)


def _expected(dec_bits, layout, off, S, n, src_pitch):
    """uint32 [S, n]: element (s, t) of a source that starts `off` elements into the pool"""
    st = (src_pitch * 4, 4) if layout == "stream" else (4, src_pitch * 4)
    return np.lib.stride_tricks.as_strided(dec_bits[off:], shape=(S, n), strides=st)


class _Device:
    """one source pool and one destination buffer on the device, for many launches"""

    def __init__(self, eng, pool, dst_words):
        self.eng, self.dst_words = eng, dst_words
        self.d_src = eng.device_malloc(pool.nbytes)
        self.d_dst = eng.device_malloc(dst_words * 4)
        eng.h2d(self.d_src, pool)
        self.esz = pool.dtype.itemsize
        self.fill = np.full(dst_words, SENTINEL, np.uint32)
        self.got = np.zeros(dst_words, np.uint32)

    def run(self, fmt, layout, S, n, src_off, src_pitch, dst_off, dst_pitch):
        """the whole destination buffer after one launch into sentinels"""
        self.eng.h2d(self.d_dst, self.fill)
        _wm().ingest_device(self.d_src + src_off * self.esz, fmt, layout, S, n, src_pitch, self.d_dst + (MARGIN + dst_off) * 4, dst_pitch)
        self.eng.synchronize()
        self.eng.d2h(self.got, self.d_dst)
        return self.got

    def close(self):
        self.eng.device_free(self.d_src)
        self.eng.device_free(self.d_dst)


@pytest.mark.parametrize("layout", ["stream", "sample"])
@pytest.mark.parametrize("fmt", ["f32", "s16", "mulaw", "alaw"])
def test_ingest_kernel_bit_for_bit(eng, fmt, layout):
    smax, nmax = max(STREAMS), max(LENGTHS)
    pool = _pool(fmt, (max(smax, nmax) + 4) * (max(smax, nmax) + 20) + 8, 11)
    dec_bits = ir.decode(pool, fmt).view(np.uint32)
    if fmt == "f32":
        assert np.array_equal(dec_bits, pool.view(np.uint32))
    dev = _Device(eng, pool, 2 * MARGIN + 4 + smax * (nmax + 8))
    launches = 0
    try:
        for S in STREAMS:
            for n in LENGTHS + ((CHUNK + 7,) if layout == "stream" and S in LONG_STREAMS else ()):
                # pitches that are no multiple of four, and 16-element-aligned ones (every row on the wide path when the offsets are 0)
                for src_pitch, dst_pitch in (((n + 1) if layout == "stream" else (S + 2), n + 1),
                                             (((n + 15) & ~15) if layout == "stream" else ((S + 15) & ~15), max((n + 3) & ~3, 4))):
                    for src_off in range(4):
                        want_rows = _expected(dec_bits, layout, src_off, S, n, src_pitch)
                        for dst_off in range(4):
                            got = dev.run(fmt, layout, S, n, src_off, src_pitch, dst_off, dst_pitch)
                            want = dev.fill.copy()
                            rows = np.lib.stride_tricks.as_strided(want[MARGIN + dst_off:], shape=(S, n), strides=(dst_pitch * 4, 4))
                            rows[...] = want_rows
                            bad = np.flatnonzero(got != want)
                            assert bad.size == 0, "%s %s S=%d n=%d src +%d pitch %d, dst +%d pitch %d: %d words differ, first at %d (row %d col %d)" % (
                                fmt, layout, S, n, src_off, src_pitch, dst_off, dst_pitch, bad.size, bad[0] - MARGIN - dst_off,
                                (bad[0] - MARGIN - dst_off) // dst_pitch, (bad[0] - MARGIN - dst_off) % dst_pitch)
                            launches += 1
    finally:
        dev.close()
    assert launches == (len(STREAMS) * len(LENGTHS) + (len(LONG_STREAMS) if layout == "stream" else 0)) * 2 * 16


@pytest.mark.parametrize("layout", ["stream", "sample"])
def test_ingest_every_value(eng, layout):
    s16 = np.arange(-32768, 32768, dtype=np.int32).astype(np.int16)
    codes = np.arange(256, dtype=np.uint8)
    for fmt, vals, shape in (("s16", s16, (4, 16384)), ("mulaw", codes, (4, 64)), ("alaw", codes, (4, 64))):
        S, n = shape
        x = vals.reshape(shape)                                    # [S, n]
        src = x if layout == "stream" else np.ascontiguousarray(x.T)   # frames [n, S]
        dev = _Device(eng, src.reshape(-1), 2 * MARGIN + S * n)
        try:
            got = dev.run(fmt, layout, S, n, 0, n if layout == "stream" else S, 0, n)
        finally:
            dev.close()
        want = ir.decode(x, fmt).view(np.uint32).reshape(-1)
        assert np.array_equal(got[MARGIN:MARGIN + S * n], want), fmt
        assert (got[:MARGIN] == SENTINEL).all() and (got[MARGIN + S * n:] == SENTINEL).all()
        # ... and what it is exact against: the float64 value
        assert np.array_equal(got[MARGIN:MARGIN + S * n].view(np.float32).astype(np.float64), ir.decode(x, fmt, np.float64).reshape(-1))


# ---- fskhip_demodulate_host_fmt == convert on the host, then fskhip_demodulate_host ------------------------------------------
S_HOST = 130                       # three 64-stream groups, the last one partial
CALLS = (1001, 16, 2481, 7)        # ... then the rest: odd lengths leave the fp32 engine mid decimator-pair (the three-float shift)
_SIGNALS = {}


def _payload(s):
    """16 letters (held with the CPU oracle: one such frame, quantised to every format, decodes under both configurations for every
    stream of the batch -- the reference itself, on floats, does not decode every arbitrary byte string behind a lead-in of zeros)"""
    return bytes(0x41 + (s * 5 + 3 * i) % 26 for i in range(16))


def _signal(cfg_name):
    """float32 [S_HOST, N]: s * 7 % 400 zeros, one 16-byte frame at amplitude 0.5, 3000 zeros -- made once per configuration"""
    if cfg_name not in _SIGNALS:
        wm = _wm()
        cfg = BELL if cfg_name == "bell202" else {}
        mod = wm.FSKEngine(S_HOST, cfg, precision=wm.PRECISION_F64)
        frames = mod.modulate_data([_payload(s) for s in range(S_HOST)])
        mod.close()
        flen = max(len(f) for f in frames)
        x = np.zeros((S_HOST, 399 + flen + 3000), np.float32)
        for s, f in enumerate(frames):
            lead = s * 7 % 400
            x[s, lead:lead + len(f)] = 0.5 * f
        _SIGNALS[cfg_name] = x
    return _SIGNALS[cfg_name]


_QUANTISED = {}


def _quantised(cfg_name, fmt):
    """(the signal in the format [S, N], its floats, the same as interleaved frames [N, S + 3]) -- made once, never written to"""
    if (cfg_name, fmt) not in _QUANTISED:
        q = ir.quantise(_signal(cfg_name), fmt)
        frames = np.zeros((q.shape[1], q.shape[0] + 3), q.dtype)
        frames[:, :q.shape[0]] = q.T
        _QUANTISED[(cfg_name, fmt)] = (q, ir.decode(q, fmt), frames)
    return _QUANTISED[(cfg_name, fmt)]


def _all_state(e):
    return [(e.get_status(s), e.debug_state(s)) for s in range(e.n_streams)]


@pytest.mark.parametrize("slab", [None, 512], ids=["direct", "slab512"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("cfg_name", ["default", "bell202"])
@pytest.mark.parametrize("layout", ["stream", "sample"])
@pytest.mark.parametrize("fmt", ["s16", "mulaw", "alaw"])
def test_host_fmt_equals_host_side_conversion(fmt, layout, cfg_name, prec, slab):
    wm = _wm()
    cfg = BELL if cfg_name == "bell202" else {}
    # [S, N] in the format; what a host-side conversion hands to fskhip_demodulate_host; interleaved frames of pitch S + 3
    q, floats, src = _quantised(cfg_name, fmt)
    S, N = q.shape
    precision = wm.PRECISION_F64 if prec == "f64" else wm.PRECISION_F32
    opts = {} if slab is None else {"host_slab": slab}
    a = wm.FSKEngine(S, cfg, precision=precision, options=opts)     # narrow samples in
    b = wm.FSKEngine(S, cfg, precision=precision, options=opts)     # floats in
    try:
        got = [b""] * S
        ref = [b""] * S
        off = 0
        for ln in CALLS + (N - sum(CALLS),):
            part = src[off:off + ln, :S] if layout == "sample" else q[:, off:off + ln]
            ab, ae = a.demodulate_samples(part, fmt=fmt, layout=layout)
            bb, be = b.demodulate_data(floats[:, off:off + ln])
            assert ab == bb, "bytes of the call at %d" % off
            assert np.array_equal(ae, be), "'eod' counts of the call at %d" % off
            got = [g + x for g, x in zip(got, ab)]
            ref = [g + x for g, x in zip(ref, bb)]
            off += ln
        # (not an empty comparison: every stream's frame decodes, from the quantised samples)
        assert ref == [_payload(s) for s in range(S)]
        assert got == ref
        sa, sb = _all_state(a), _all_state(b)
        for s in range(S):
            assert sa[s][0] == sb[s][0] or str(sa[s][0]) == str(sb[s][0]), "status of stream %d" % s   # (str: NaN gains compare equal)
            ra, ia = sa[s][1]
            rb, ib = sb[s][1]
            assert ia == ib, "integer state words of stream %d" % s
            assert np.array_equal(np.array(ra).view(np.uint64), np.array(rb).view(np.uint64)), "real state words of stream %d" % s
    finally:
        a.close()
        b.close()


def test_f32_sample_major_and_f32_stream_major_are_the_float_call():
    wm = _wm()
    x = _signal("default")
    S, N = x.shape
    frames = np.zeros((N, S + 3), np.float32)
    frames[:, :S] = x.T
    engs = [wm.FSKEngine(S, {}, options={"host_slab": 2048}) for _ in range(3)]
    try:
        r0 = engs[0].demodulate_data(x)
        r1 = engs[1].demodulate_samples(x)
        r2 = engs[2].demodulate_samples(frames[:, :S], layout="sample")
        assert r0[0] == [_payload(s) for s in range(S)]
        for r in (r1, r2):
            assert r[0] == r0[0] and np.array_equal(r[1], r0[1])
        st = [_all_state(e) for e in engs]
        assert str(st[1]) == str(st[0]) and str(st[2]) == str(st[0])
    finally:
        for e in engs:
            e.close()


def test_writeback_flag_with_a_narrow_format_is_refused_and_leaves_the_engine_alone():
    wm = _wm()
    from webaudio_modem_amd import _lib
    x = _signal("default")[:4]
    q = ir.quantise(x, "s16")
    a, b = wm.FSKEngine(4, {}), wm.FSKEngine(4, {})
    try:
        out, counts = np.zeros((4, 64), np.uint8), np.zeros(4, np.uint32)
        for fmt, lay, arr in ((_lib.SAMPLES_S16, 0, q), (_lib.SAMPLES_MULAW, 0, ir.quantise(x, "mulaw")),
                              (_lib.SAMPLES_F32, 1, np.ascontiguousarray(x.T))):
            rc = a._L.fskhip_demodulate_host_fmt(a._h, arr.ctypes.data, fmt, lay, x.shape[1], x.shape[1] if lay == 0 else 4, out.ctypes.data, 64,
                                                 counts.ctypes.data, None, wm.DEMOD_WRITEBACK_AGC)
            assert rc == _lib.E_INVALID and "WRITEBACK" in a._L.fskhip_last_error().decode()
        assert a.get_status(0)["demodulationCalls"] == 0
        ra, rb = a.demodulate_data(x), b.demodulate_data(x)
        assert ra[0] == rb[0] == [_payload(s) for s in range(4)] and np.array_equal(ra[1], rb[1])
        assert str(_all_state(a)) == str(_all_state(b))
        # float samples in stream-major layout may take the flag: it is fskhip_demodulate_host's own call
        y, z = x.copy(), x.copy()
        c, d = wm.FSKEngine(4, {}), wm.FSKEngine(4, {})
        try:
            rc = c._L.fskhip_demodulate_host_fmt(c._h, y.ctypes.data, _lib.SAMPLES_F32, 0, y.shape[1], y.shape[1], out.ctypes.data, 64, counts.ctypes.data,
                                                 None, wm.DEMOD_WRITEBACK_AGC)
            assert rc == 0
            d.demodulate_data(z, writeback_agc=True)
            assert np.array_equal(y.view(np.uint32), z.view(np.uint32)) and not np.array_equal(y, x)
        finally:
            c.close()
            d.close()
    finally:
        a.close()
        b.close()


def test_python_argument_errors(eng):
    with pytest.raises(ValueError, match="mulaw"):
        eng.demodulate_samples(np.zeros((1, 64), np.uint8))
    with pytest.raises(ValueError, match="dtype"):
        eng.demodulate_samples(np.zeros((1, 64), np.int32))
    with pytest.raises(ValueError, match="expected 1 streams"):
        eng.demodulate_samples(np.zeros((2, 64), np.int16))


@pytest.mark.parametrize("layout", ["stream", "sample"])
def test_sharded_demodulate_samples_equals_unsharded(layout):
    wm = _wm()
    q = ir.quantise(_signal("default"), "s16")
    S, N = q.shape
    src = q if layout == "stream" else np.ascontiguousarray(q.T)
    one = wm.FSKEngine(S, {})
    made = []

    def factory(count, cfg, dev, prec):
        made.append(count)
        return wm.FSKEngine(count, cfg, device=dev, precision=prec)

    two = wm.FSKEngineSharded(S, {}, devices=[0, 0], engine_factory=factory)     # a two-shard split on one device
    every = wm.FSKEngineSharded(S, {})                                           # the devices present
    try:
        assert made == [65, 65]
        off = 0
        for ln in (1001, N - 1001):
            part = src[:, off:off + ln] if layout == "stream" else src[off:off + ln]
            want = one.demodulate_samples(part, layout=layout)
            for sh in (two, every):
                got = sh.demodulate_samples(part, layout=layout)
                assert got[0] == want[0] and np.array_equal(got[1], want[1])
            off += ln
        assert [two.get_status(s) for s in range(S)] == [one.get_status(s) for s in range(S)]
        assert one.get_status(S - 1)["syncDetections"] == 1
    finally:
        one.close()
        two.close()
        every.close()
