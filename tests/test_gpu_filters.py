"""The batched FIR and IIR filters on the GPU (csrc/fsk_fir.hip, csrc/fsk_iir.hip) against the CPU models of tests/filter_ref.py,
which tests/test_filter_ref_cpu.py anchors to exact rational arithmetic, the oracle and the recorded reference outputs.

Every comparison is on bit patterns (uint32 / uint64 views): there is no tolerance in this file.  The fp32 FIR kernel is what the
fp32 resampler and rate converter tests are held to, so it is held to something independent here.

  a. FIR, fp64 and fp32, through processBuffer: 1 .. 9, 51, 257, 1021, 1024, 1025 and 4096 taps (every n_taps % 4, a history
     prefix of up to four tiles) x 1, 3, 4, 5, 1023, 1024, 1025, 2051 samples (the 1024-sample tile's edge, a last partial
     float4, three tiles) at 2 streams; 1, 63, 65, 130 streams on seven tap / length pairs;
  b. call cuts with two consecutive calls shorter than the history, then reset(3);
  c. fskhip_fir_process_device on a caller's stream: sources and destinations 0 .. 3 floats off the 16-byte grid, pitches that
     allow 16-byte stores and pitches that do not, the whole destination compared, sentinels included, the source unchanged;
  d. overlapping source and destination ranges are refused before anything is launched, and the delay line is as it was;
  e. IIR, Real x IO in {float32, float64}^2: the nine specialised length pairs and the run-time one, 1, 63, 64, 65, 130 streams,
     calls of 1, 15, 16, 17, 31, 32, 33, 100 samples (the tiles are 32 floats or 16 doubles); float and double calls interleaved
     on one handle; reset of one stream;
  f. fskhip_iir_process_device / _f64_device on a caller's stream: each of the four conditions of the 16-byte path broken on its
     own, whole destination compared; in place equals out of place, on the vector path and on the element path."""
import numpy as np
import pytest

import filter_ref as fr
from hip_caller import Caller

pytestmark = [pytest.mark.gpu]

PRECISIONS = ("f64", "f32")
FIR_TAPS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 51, 257, 1021, 1024, 1025, 4096)
FIR_LENGTHS = (1, 3, 4, 5, 1023, 1024, 1025, 2051)
FIR_STREAMS = (1, 63, 65, 130)
FIR_PAIRS = ((1, 1), (3, 2051), (6, 1025), (51, 1023), (257, 1025), (1025, 5), (4096, 3))     # (taps, samples) for every stream count
IIR_SHAPES = ((1, 1, 1.0), (2, 2, 1.25), (3, 3, 1.0), (5, 5, 0.8), (9, 9, 1.0),                # (nb, na, a[0]): the specialised kernels
              (2, 1, 2.0), (1, 2, 1.0), (2, 4, 1.0), (9, 2, 1.0), (3, 9, 1.5))                 # and the run-time lengths
IIR_STREAMS = (1, 63, 64, 65, 130)
IIR_LENGTHS = (1, 15, 16, 17, 31, 32, 33, 100)
SMAX, NMAX = 130, 2051
MARGIN = 8
E_INVALID = -1


def _wm():
    import webaudio_modem_amd as wm
    return wm


def _prec(name):
    wm = _wm()
    return wm.PRECISION_F64 if name == "f64" else wm.PRECISION_F32


def _u(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same(got, want, what):
    g, w = _u(got), _u(want)
    assert g.shape == w.shape, what
    bad = np.argwhere(g != w)
    assert bad.size == 0, "%s: %d of %d differ, first at %s: got %r, want %r" % (
        what, len(bad), g.size, tuple(bad[0]), np.asarray(got)[tuple(bad[0])], np.asarray(want)[tuple(bad[0])])


_X = {}


def _x(dtype=np.float32):
    """[SMAX, NMAX] inputs, made once and never written to; the doubles are not float32 values"""
    if dtype not in _X:
        _X[dtype] = fr.signed_uniform(np.random.default_rng(77), (SMAX, NMAX)).astype(dtype)
        _X[dtype].setflags(write=False)
    return _X[dtype]


def _taps(n_taps):
    return fr.signed_uniform(np.random.default_rng(9000 + n_taps), n_taps)


def _iir_coefficients(nb, na, a0):
    """a stable denominator: the feedback's magnitudes sum to at most 0.4 (0.5 after the division by a[0] = 0.8)"""
    r = np.random.default_rng(100 * nb + na)
    return list(fr.signed_uniform(r, nb)), [a0] + list(fr.signed_uniform(r, na - 1, 2.0 ** -8, 0.4 / max(1, na - 1)))


@pytest.fixture(scope="module")
def caller():
    eng = _wm().FSKEngine(1, {})
    c = Caller(eng)
    yield c
    c.close()
    eng.close()


# ---- a. FIR through processBuffer ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_taps", FIR_TAPS)
@pytest.mark.parametrize("prec", PRECISIONS)
def test_fir_every_tap_count_meets_every_length(prec, n_taps):
    """2 streams.  The model runs once over the longest input: it is causal, so from a zeroed delay line its output over the first n
    samples is the first n columns (tests/test_filter_ref_cpu.py checks that of the model itself)."""
    S = 2
    x = _x()[:S]
    want = fr.FIRModel(_taps(n_taps), S, prec).process_buffer(x)
    f = _wm().FIRFilterBatch(_taps(n_taps), S, precision=_prec(prec))
    try:
        for n in FIR_LENGTHS:
            f.reset()
            _same(f.processBuffer(x[:, :n]), want[:, :n], "fir %s, %d taps, %d samples" % (prec, n_taps, n))
    finally:
        f.close()
    print("compared[a %s %d taps] %d lengths" % (prec, n_taps, len(FIR_LENGTHS)))


@pytest.mark.parametrize("n_taps,n", FIR_PAIRS)
@pytest.mark.parametrize("prec", PRECISIONS)
def test_fir_every_stream_count(prec, n_taps, n):
    x = _x()[:, :n]
    want = fr.FIRModel(_taps(n_taps), SMAX, prec).process_buffer(x)          # (rows are independent: the first S rows are S streams')
    for S in FIR_STREAMS:
        f = _wm().FIRFilterBatch(_taps(n_taps), S, precision=_prec(prec))
        try:
            _same(f.processBuffer(x[:S]), want[:S], "fir %s, %d streams, %d taps, %d samples" % (prec, S, n_taps, n))
        finally:
            f.close()
    print("compared[a %s %d taps x %d] %d stream counts" % (prec, n_taps, n, len(FIR_STREAMS)))


# ---- b. FIR call cuts ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_taps,S", [(5, 65), (257, 65), (1025, 65), (4096, 2)])
@pytest.mark.parametrize("prec", PRECISIONS)
def test_fir_call_cuts_and_reset_of_one_stream(prec, n_taps, S):
    """Calls of 1, 3, n_taps-2, n_taps-2, 2, n_taps-1, 0, 1030 samples and the rest: two calls running that are shorter than the
    delay line (fir_hist_kernel takes part of it from the old one, twice), an empty call.  The model is cut the same way."""
    wm = _wm()
    lens = [1, 3, n_taps - 2, n_taps - 2, 2, n_taps - 1, 0, 1030, 9]
    cuts = np.concatenate([[0], np.cumsum(lens)])
    rng = np.random.default_rng(n_taps)
    x = fr.signed_uniform(rng, (S, cuts[-1])).astype(np.float32)
    model = fr.FIRModel(_taps(n_taps), S, prec)
    want = np.concatenate([model.process_buffer(x[:, p:q]) for p, q in zip(cuts, cuts[1:])], axis=1)
    f, whole = (wm.FIRFilterBatch(_taps(n_taps), S, precision=_prec(prec)) for _ in range(2))
    try:
        got = np.concatenate([f.processBuffer(x[:, p:q]) for p, q in zip(cuts, cuts[1:])], axis=1)
        _same(got, want, "fir %s, %d taps, cut into %s" % (prec, n_taps, lens))
        _same(whole.processBuffer(x), want, "fir %s, %d taps, one call of %d" % (prec, n_taps, cuts[-1]))
        z = fr.signed_uniform(rng, (S, 40)).astype(np.float32)
        r = min(3, S - 1)
        f.reset(r)
        model.reset(r)
        want2 = model.process_buffer(z)
        fresh = fr.FIRModel(_taps(n_taps), S, prec).process_buffer(z)
        assert np.array_equal(_u(want2[r]), _u(fresh[r])) and not np.array_equal(_u(want2[r - 1]), _u(fresh[r - 1]))   # (the model's own reset)
        _same(f.processBuffer(z), want2, "fir %s, %d taps, after reset(%d)" % (prec, n_taps, r))
    finally:
        f.close()
        whole.close()
    print("compared[b %s %d taps] cut, whole, after reset" % (prec, n_taps))


# ---- device buffers of a caller ------------------------------------------------------------------------------------------------------

class _Dev:
    """one device buffer of `total` elements; place(): rows at MARGIN + off, `pitch` apart, in a flat array of sentinels"""

    def __init__(self, caller, dtype, total):
        self.c, self.dtype, self.total = caller, np.dtype(dtype), total
        self.esz = self.dtype.itemsize
        self.sentinel = self.dtype.type(1234.5)
        self.base = caller.malloc(total * self.esz)
        assert self.base % 16 == 0

    def place(self, rows, pitch, off):
        used = MARGIN + off + (rows.shape[0] - 1) * pitch + rows.shape[1] + MARGIN
        assert used <= self.total and pitch >= rows.shape[1]       # the launch stays inside the buffer: checked before it runs
        flat = np.full(used, self.sentinel, self.dtype)
        view = np.lib.stride_tricks.as_strided(flat[MARGIN + off:], shape=rows.shape, strides=(pitch * self.esz, self.esz))
        view[...] = rows
        return flat

    def ptr(self, off):
        return self.base + (MARGIN + off) * self.esz

    def put(self, flat):
        self.c.upload(self.base, flat)

    def get(self, n):
        return self.c.download(self.base, np.empty(n, self.dtype))


def _device_call(caller, fn, h, src, dst, rows, want, ioff, ip, ooff, op, what):
    """rows -> src at (ioff, ip), sentinels -> dst, fn(h, ...) on the caller's stream; the whole of dst is `want` placed at
    (ooff, op) into sentinels and src is as it was"""
    n = rows.shape[1]
    host_in = src.place(rows, ip, ioff)
    host_want = dst.place(want, op, ooff)
    src.put(host_in)
    dst.put(np.full(host_want.size, dst.sentinel, dst.dtype))
    rc = fn(h, src.ptr(ioff), n, ip, dst.ptr(ooff), op, caller.stream)
    assert rc == 0, (what, rc, _wm()._lib.lib().fskhip_last_error().decode())
    caller.sync()
    _same(dst.get(host_want.size), host_want, what + ": destination")
    _same(src.get(host_in.size), host_in, what + ": source")


# ---- c. fskhip_fir_process_device ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [5, 1027])
@pytest.mark.parametrize("prec", PRECISIONS)
def test_fir_device_call_offsets_and_pitches(caller, prec, n):
    """65 streams, 7 taps.  16-byte stores need the destination on the grid and out_pitch % 4 == 0: n + 3 at n = 5 and n + 1 at
    n = 1027 have it at offset 0, every other combination stores float by float."""
    L = _wm()._lib.lib()
    S, n_taps = 65, 7
    x = _x()[:S, :n]
    want = fr.FIRModel(_taps(n_taps), S, prec).process_buffer(x)
    total = 2 * MARGIN + 4 + S * (n + 8)
    src, dst = _Dev(caller, np.float32, total), _Dev(caller, np.float32, total)
    f = _wm().FIRFilterBatch(_taps(n_taps), S, precision=_prec(prec))
    vec = 0
    try:
        for ooff in range(4):
            for k, oextra in enumerate((0, 1, 3, 4)):
                ioff, ip, op = (ooff + k) % 4, n + (1, 4, 2, 7)[(ooff + k) % 4], n + oextra
                vec += ooff == 0 and op % 4 == 0
                f.reset()
                _device_call(caller, L.fskhip_fir_process_device, f._h, src, dst, x, want, ioff, ip, ooff, op,
                             "fir %s device n=%d, source +%d pitch %d, destination +%d pitch %d" % (prec, n, ioff, ip, ooff, op))
    finally:
        f.close()
    assert vec >= 1
    print("compared[c %s n=%d] 16 placements, %d with 16-byte stores" % (prec, n, vec))


# ---- d. FIR aliasing -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECISIONS)
def test_fir_device_call_refuses_overlapping_buffers(caller, prec):
    """The ranges [p, p + (S-1) * pitch + n) of source and destination may not share a float: identical, the destination starting
    inside the source, the destination ending inside the source; FSKHIP_E_INVALID and nothing launched -- the destination keeps its
    sentinels and the delay line is as the call before left it.  Ranges that touch are taken."""
    L = _wm()._lib.lib()
    S, n, n_taps, pitch = 65, 33, 7, 36
    span = (S - 1) * pitch + n
    x = _x()[:S]
    model = fr.FIRModel(_taps(n_taps), S, prec)
    buf = _Dev(caller, np.float32, 2 * MARGIN + 3 * span + 8)
    f = _wm().FIRFilterBatch(_taps(n_taps), S, precision=_prec(prec))
    fn = L.fskhip_fir_process_device
    try:
        def rows_at(host, off):
            return np.lib.stride_tricks.as_strided(host[MARGIN + off:], shape=(S, n), strides=(pitch * 4, 4))

        def valid(cols, ooff, what):
            """n columns of x from the source at 0 to the destination at ooff, both in the one buffer"""
            host = np.full(buf.total, buf.sentinel, np.float32)
            rows_at(host, 0)[...] = x[:, cols:cols + n]
            buf.put(host)
            assert fn(f._h, buf.ptr(0), n, pitch, buf.ptr(ooff), pitch, caller.stream) == 0, what
            caller.sync()
            rows_at(host, ooff)[...] = model.process_buffer(x[:, cols:cols + n])
            _same(buf.get(buf.total), host, what)

        valid(0, span, "the destination begins where the source ends")
        host = buf.get(buf.total)
        for ooff, what in ((0, "identical"), (1, "one float on"), (span - 1, "the last float of the source"),
                           (pitch, "one row on")):
            assert fn(f._h, buf.ptr(0), n, pitch, buf.ptr(ooff), pitch, caller.stream) == E_INVALID, what
            assert L.fskhip_last_error().decode() == "fskhip_fir_process_device: the input and output buffers overlap", what
        # the destination in front of the source, its last float on the source's first
        assert fn(f._h, buf.ptr(span - 1), n, pitch, buf.ptr(0), pitch, caller.stream) == E_INVALID
        assert fn(f._h, buf.ptr(span), n, pitch, buf.ptr(1), pitch + 1, caller.stream) == E_INVALID       # (a wider destination)
        caller.sync()
        _same(buf.get(buf.total), host, "after the refusals")
        valid(n, span + 3, "the call after the refusals continues the delay line")
    finally:
        f.close()
    print("compared[d %s] 6 refusals, the calls before and after" % prec)


# ---- e. IIR through processBuffer / processSamples ---------------------------------------------------------------------------------------

IO = {"float": np.float32, "double": np.float64}


def _iir_run(f, x):
    return f.processBuffer(x) if x.dtype == np.float32 else f.processSamples(x)


@pytest.mark.parametrize("io", list(IO))
@pytest.mark.parametrize("prec", PRECISIONS)
def test_iir_every_shape_stream_count_and_length(prec, io):
    """Consecutive calls of every length on one handle, so that each call but the first starts from a history the one before left;
    the model runs once per coefficient set over 130 streams (rows are independent)."""
    wm = _wm()
    cuts = np.concatenate([[0], np.cumsum(IIR_LENGTHS)])
    x = _x(IO[io])[:, :cuts[-1]]
    for nb, na, a0 in IIR_SHAPES:
        b, a = _iir_coefficients(nb, na, a0)
        model = fr.IIRModel(b, a, SMAX, prec)
        want = [model.process(x[:, p:q], IO[io]) for p, q in zip(cuts, cuts[1:])]
        for S in IIR_STREAMS:
            f = wm.IIRFilterBatch(b, a, S, precision=_prec(prec))
            try:
                for k, (p, q) in enumerate(zip(cuts, cuts[1:])):
                    _same(_iir_run(f, x[:S, p:q]), want[k][:S], "iir %s/%s b %d a %d, %d streams, call of %d" % (prec, io, nb, na, S, q - p))
            finally:
                f.close()
    print("compared[e %s/%s] %d shapes x %d stream counts x %d lengths" % (prec, io, len(IIR_SHAPES), len(IIR_STREAMS), len(IIR_LENGTHS)))


@pytest.mark.parametrize("nb,na,a0", [(5, 5, 0.8), (2, 4, 1.0)])
@pytest.mark.parametrize("prec", PRECISIONS)
def test_iir_float_and_double_calls_share_the_histories(prec, nb, na, a0):
    """a float call, a double call, a float call on one handle; then reset(3): stream 3 starts over, the others carry on"""
    S = 65
    b, a = _iir_coefficients(nb, na, a0)
    x32, x64 = _x(np.float32)[:S], _x(np.float64)[:S]
    model = fr.IIRModel(b, a, S, prec)
    f = _wm().IIRFilterBatch(b, a, S, precision=_prec(prec))
    try:
        for k, x in enumerate((x32[:, :33], x64[:, 33:50], x32[:, 50:150], x64[:, 150:151])):
            _same(_iir_run(f, x), model.process(x, x.dtype.type), "iir %s b %d a %d, call %d (%s)" % (prec, nb, na, k, x.dtype))
        f.reset(3)
        model.reset(3)
        for k, x in enumerate((x64[:, 200:217], x32[:, 217:250])):
            want = model.process(x, x.dtype.type)
            _same(_iir_run(f, x), want, "iir %s b %d a %d, call %d after reset(3)" % (prec, nb, na, k))
            if k == 0:
                fresh = fr.IIRModel(b, a, S, prec).process(x, x.dtype.type)
                assert np.array_equal(_u(want[3]), _u(fresh[3])) and not np.array_equal(_u(want[4]), _u(fresh[4]))
    finally:
        f.close()
    print("compared[e %s b %d a %d] 4 interleaved calls, 2 after reset" % (prec, nb, na))


# ---- f. fskhip_iir_process_device / _f64_device ------------------------------------------------------------------------------------------

def _iir_device_fn(io):
    L = _wm()._lib.lib()
    return L.fskhip_iir_process_device if io == "float" else L.fskhip_iir_process_f64_device


@pytest.mark.parametrize("io", list(IO))
@pytest.mark.parametrize("prec", PRECISIONS)
def test_iir_device_call_offsets_and_pitches(caller, prec, io):
    """65 streams (a second workgroup with one live lane), 100 samples: whole tiles and a last part of one.  The 16-byte path needs
    both pitches to be multiples of VN (4 floats, 2 doubles) and both pointers on the grid: all four hold in the first two
    placements, each fails alone in the next four, then mixtures."""
    S, n, (nb, na, a0) = 65, 100, (3, 3, 1.25)
    dtype = IO[io]
    VN = 16 // np.dtype(dtype).itemsize
    b, a = _iir_coefficients(nb, na, a0)
    x = _x(dtype)[:S, :n]
    want = fr.IIRModel(b, a, S, prec).process(x, dtype)
    total = 2 * MARGIN + 4 + S * (n + 8)
    src, dst = _Dev(caller, dtype, total), _Dev(caller, dtype, total)
    f = _wm().IIRFilterBatch(b, a, S, precision=_prec(prec))
    placements = [(0, 0, 0, 0), (0, VN, 0, VN),                                    # (source offset, pitch extra, destination offset, pitch extra)
                  (0, 1, 0, 0), (0, 0, 0, 3), (1, 0, 0, 0), (0, 0, 1, 0),
                  (2, VN, 0, 1), (3, 3, 2, VN), (0, 1, 3, 1), (1, 0, 1, 0), (2, VN, 2, 0), (3, 3, 3, 3), (1, VN, 3, VN)]
    vec_ok = [all(v % VN == 0 for v in (n + ie, n + oe, io_, oo)) for io_, ie, oo, oe in placements]
    assert vec_ok[:6] == [True, True, False, False, False, False]
    try:
        for ioff, ie, ooff, oe in placements:
            f.reset()
            _device_call(caller, _iir_device_fn(io), f._h, src, dst, x, want, ioff, n + ie, ooff, n + oe,
                         "iir %s/%s device, source +%d pitch %d, destination +%d pitch %d" % (prec, io, ioff, n + ie, ooff, n + oe))
    finally:
        f.close()
    print("compared[f %s/%s] %d placements, %d on the 16-byte path" % (prec, io, len(placements), sum(vec_ok)))


@pytest.mark.parametrize("n,off,extra", [(96, 0, 4), (100, 1, 3)], ids=["vector-path", "element-path"])
@pytest.mark.parametrize("io", list(IO))
@pytest.mark.parametrize("prec", PRECISIONS)
def test_iir_device_call_in_place(caller, prec, io, n, off, extra):
    """d_out == d_in with one pitch: the rows become the model's output -- what the out-of-place call gives, which the same
    model holds in the test above --, the columns between the rows and the margins keep their sentinels.  96 samples at pitch 100
    on the grid are whole tiles on the 16-byte path; 100 samples at pitch 103, one element off the grid, go element by element."""
    S, (nb, na, a0) = 65, (5, 5, 0.8)
    dtype = IO[io]
    VN = 16 // np.dtype(dtype).itemsize
    assert (off == 0 and (n + extra) % VN == 0 and n % (8 * VN) == 0) or (off % VN and (n + extra) % VN)
    b, a = _iir_coefficients(nb, na, a0)
    x = _x(dtype)[:S, :n]
    want = fr.IIRModel(b, a, S, prec).process(x, dtype)
    buf, out = (_Dev(caller, dtype, 2 * MARGIN + 4 + S * (n + 8)) for _ in range(2))
    f = _wm().IIRFilterBatch(b, a, S, precision=_prec(prec))
    fn, pitch = _iir_device_fn(io), n + extra
    try:
        _device_call(caller, fn, f._h, buf, out, x, want, off, pitch, off, pitch, "iir %s/%s out of place, n=%d" % (prec, io, n))
        f.reset()
        host_want = buf.place(want, pitch, off)
        buf.put(buf.place(x, pitch, off))
        assert fn(f._h, buf.ptr(off), n, pitch, buf.ptr(off), pitch, caller.stream) == 0
        caller.sync()
        _same(buf.get(host_want.size), host_want, "iir %s/%s in place, n=%d" % (prec, io, n))
        _same(buf.get(host_want.size), out.get(host_want.size), "iir %s/%s in place against out of place, n=%d" % (prec, io, n))
    finally:
        f.close()
    print("compared[f %s/%s n=%d] out of place, in place" % (prec, io, n))
