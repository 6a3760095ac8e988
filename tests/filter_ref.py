"""CPU models of the batched filters (csrc/fsk_fir.hip, csrc/fsk_iir.hip), numpy only, vectorised over streams: what the kernels
compute operation by operation, so that the GPU tests compare bit patterns and need no tolerance.

  * FIR, fp64 handle: acc = 0; acc = acc + c[i] * x[t-i] for i = 0 .. n_taps-1, product and sum rounded separately in float64
    (fsk_mac_dev.h mac<double>; the library is built -ffp-contract=off), the result stored as float32.
  * FIR, fp32 handle: the taps rounded once to float32, acc = fma(c[i], x[t-i], acc) in float32 in the same order, one rounding
    per step (mac<float> is __builtin_fmaf).  fma32() below emulates that single rounding exactly in float64.
  * IIR (iir_step), Real in {float32, float64} x IO in {float32, float64}: coefficients normalised by a[0] in doubles as
    fskhip_iir_create does, rounded once to Real; out = 0; out += b[0]*x; out += b[i]*xh[i-1] ..; out -= a[i]*yh[i-1] ..; every
    product and sum rounded on its own in Real (csrc/Makefile: CXXFLAGS carries -ffp-contract=off for every unit, and the only
    per-unit addition, -fno-slp-vectorize, goes to other files); the history keeps the Real value of out, the caller gets it
    cast to IO; one history for both IO forms.

Every model asserts that no intermediate is subnormal (or not finite), so that no expected value depends on the device's denormal
mode: draw inputs and coefficients with signed_uniform() below."""
import numpy as np

_BITS = {np.dtype(np.float32): (np.uint32, 0x7FFFFFFF, 0x007FFFFF, 0x7F800000),
         np.dtype(np.float64): (np.uint64, 0x7FFFFFFFFFFFFFFF, 0x000FFFFFFFFFFFFF, 0x7FF0000000000000)}


def signed_uniform(rng, shape, lo=2.0 ** -8, hi=1.2):
    """magnitudes in [lo, hi] with random signs, as float64: no zeros, nothing near the subnormals"""
    return rng.uniform(lo, hi, shape) * rng.choice((-1.0, 1.0), shape)


def normal(v):
    """v (float32 or float64) holds only zeros and normal numbers of its own format -- no subnormals, infinities or NaNs"""
    v = np.asarray(v)
    if v.size:
        u, mag, frac, inf = _BITS[v.dtype]
        ab = np.atleast_1d(v).view(u) & u(mag)
        assert int(ab.max()) < inf, "an intermediate is not finite"
        # ab - 1 wraps a zero round to the largest integer; a subnormal's 1 .. frac becomes 0 .. frac - 1
        assert int(np.subtract(ab, u(1), out=ab).min()) >= frac, "an intermediate is subnormal"
    return v


def fma32(a, b, c):
    """float32(a * b + c) with ONE rounding, for float32 arrays or scalars a, b, c.

    The product of two float32 values is exact in float64 (48 significant bits).  s = p + c is rounded to float64, and TwoSum gives
    the error e = (p + c) - s exactly.  Rounding s on to float32 differs from rounding the exact sum only where s sits exactly
    halfway between two float32 values while the exact sum does not (e != 0): there s moves one float64 ulp towards e first."""
    for v in (a, b, c):
        assert np.asarray(v).dtype == np.float32
    p = np.multiply(a, b, dtype=np.float64)
    s = np.atleast_1d(np.add(p, c, dtype=np.float64))
    bits = s.view(np.uint64)
    half = np.flatnonzero((bits & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000))   # the 29 bits float32 drops are 1000..0
    if half.size:
        ph = np.broadcast_to(p, s.shape).reshape(-1)[half]
        ch = np.broadcast_to(c, s.shape).reshape(-1)[half].astype(np.float64)
        sh = s.reshape(-1)[half]
        bv = sh - ph                                 # TwoSum (Knuth): exact for any two doubles
        e = (ph - (sh - bv)) + (ch - bv)
        away = (e > 0) == (sh > 0)                   # the error points away from zero: one ulp up in magnitude, else one down
        flat = bits.reshape(-1)                      # (s is this call's own array: a view of it)
        flat[half[(e != 0) & away]] += np.uint64(1)
        flat[half[(e != 0) & ~away]] -= np.uint64(1)
    r = normal(s.astype(np.float32))
    assert np.count_nonzero(r) == np.count_nonzero(s), "a sum below the float32 range"
    return r.reshape(np.broadcast(p, c).shape)


class FIRModel:
    """FIRFilterBatch(taps, n_streams, precision) on the CPU; precision is "f64" or "f32" """

    def __init__(self, taps, n_streams, precision):
        assert precision in ("f64", "f32")
        self.precision, self.S = precision, n_streams
        self.c = normal(np.asarray(taps, np.float64))
        if precision == "f32":
            self.c = normal(self.c.astype(np.float32))
        self.h = self.c.size - 1
        self.delay = np.zeros((n_streams, self.h), np.float32)      # the n_taps-1 inputs before the next call, oldest first

    def process_buffer(self, x):
        x = np.asarray(x)
        assert x.dtype == np.float32 and x.ndim == 2 and x.shape[0] == self.S
        n, h = x.shape[1], self.h
        xx = np.concatenate([self.delay, normal(x)], axis=1)
        if self.precision == "f64":
            xx64 = xx.astype(np.float64)
            mags = np.abs(xx64[xx64 != 0])
            lo, hi = (mags.min(), mags.max()) if mags.size else (np.float64(1), np.float64(1))
            acc, p = np.zeros((self.S, n), np.float64), np.empty((self.S, n), np.float64)
            for i in range(self.c.size):
                # rounding is monotonic: every product is a zero or lies between these two, so they stand for all of them
                normal(np.abs(self.c[i]) * np.array([lo, hi]))
                np.multiply(self.c[i], xx64[:, h - i:h - i + n], out=p)
                normal(np.add(acc, p, out=acc))
            out = normal(acc.astype(np.float32))
            assert np.count_nonzero(out) == np.count_nonzero(acc), "a sum below the float32 range"
        else:
            out = np.zeros((self.S, n), np.float32)
            for i in range(self.c.size):
                out = fma32(self.c[i], xx[:, h - i:h - i + n], out)
        self.delay = xx[:, n:].copy()
        return out

    def reset(self, stream=-1):
        if stream < 0:
            self.delay[:] = 0
        else:
            self.delay[stream] = 0


class IIRModel:
    """IIRFilterBatch(b, a, n_streams, precision) on the CPU: process(x, io) is processBuffer (io = np.float32) or processSamples
    (io = np.float64) on an [S, n] block of that type, and the two share the histories"""

    def __init__(self, b, a, n_streams, precision):
        assert precision in ("f64", "f32")
        self.real = np.dtype(np.float64 if precision == "f64" else np.float32)
        b, a = np.array(b, np.float64), np.array(a, np.float64)
        if a[0] != 1.0:                              # fskhip_iir_create: b[i] /= a0, a[i] /= a0 for i >= 1, a[0] = 1, in doubles
            a0 = a[0]
            b = b / a0
            a[1:] = a[1:] / a0
            a[0] = 1.0
        self.b, self.a = normal(normal(b).astype(self.real)), normal(normal(a).astype(self.real))
        self.S = n_streams
        H = max(self.b.size, self.a.size) - 1
        self.xh, self.yh = np.zeros((H, n_streams), self.real), np.zeros((H, n_streams), self.real)   # [i] = x[n-1-i], y[n-1-i]

    def _ok(self, v):
        assert v.dtype == self.real
        return normal(v)

    def process(self, x, io):
        x = np.asarray(x)
        assert x.dtype == io and x.ndim == 2 and x.shape[0] == self.S
        xr = self._ok(normal(x).astype(self.real))
        assert np.count_nonzero(xr) == np.count_nonzero(x)
        y = np.empty(x.shape, io)
        for t in range(x.shape[1]):
            xt = xr[:, t]
            out = np.zeros(self.S, self.real)
            out = self._ok(out + self._ok(self.b[0] * xt))
            for i in range(1, self.b.size):
                out = self._ok(out + self._ok(self.b[i] * self.xh[i - 1]))
            for i in range(1, self.a.size):
                out = self._ok(out - self._ok(self.a[i] * self.yh[i - 1]))
            if self.xh.shape[0]:
                self.xh[1:] = self.xh[:-1].copy()
                self.yh[1:] = self.yh[:-1].copy()
                self.xh[0], self.yh[0] = xt, out
            y[:, t] = out.astype(io)
            assert np.count_nonzero(y[:, t]) == np.count_nonzero(out)
        return normal(y)

    def reset(self, stream=-1):
        if stream < 0:
            self.xh[:], self.yh[:] = 0, 0
        else:
            self.xh[:, stream], self.yh[:, stream] = 0, 0
