"""The model of the rational rate converter (include/fskhip_next.h: fskhip_ratecvt_*): the reference's FIRFilter over the input
zero-stuffed by L with every M-th output kept, written polyphase as the header writes it --
    y[j] = f32(sum over k = 0, 1, ... while p + kL < n_taps of c[p + kL] * x[m - k]),  p = (jM) mod L,  m = (jM) div L
-- in float64 with every product and every sum rounded on its own, the k ascending, then rounded to float32.  CAPTURE decodes
the format in front of it, PLAYBACK encodes behind it (tests/samples_ref.py).  Not a test; test_ratecvt_cpu.py holds it against
resample_ref.py and the oracle, and test_gpu_ratecvt.py the kernels against it."""
from math import gcd

import numpy as np

import samples_ref as sr
from oracle import pyoracle as po

MAX_TAPS = 4096


def ratio(in_rate, out_rate):
    """(L, M) of a converter from in_rate to out_rate: the rates over their gcd"""
    g = gcd(int(in_rate), int(out_rate))
    return int(out_rate) // g, int(in_rate) // g


def default_taps(in_rate, out_rate):
    """what CaptureConverter / PlaybackConverter design with taps=None, from the model's own sincLowpass: a low-pass at 0.45 of the
    lower rate, designed at L * in_rate, 16 taps per phase of the larger factor and one, with the gain L of the stuffed zeros"""
    L, M = ratio(in_rate, out_rate)
    taps = np.array(po.sinc("lowpass", 0.45 * min(in_rate, out_rate), float(L) * in_rate, 16 * max(L, M) + 1), np.float64)
    return taps * float(L)


def history(L, n_taps):
    return -(-(n_taps - 1) // L)


def out_length(L, M, n_taps, n):
    """outputs that can be non-zero for a signal of n inputs"""
    return ((n - 1) * L + n_taps - 1) // M + 1 if n else 0


def convert(x, taps, L, M, hist=None):
    """float32 [S, n], n a multiple of M -> (float32 [S, n / M * L], the history the call leaves, float32 [S, H]); hist: the history
    in front of x (None: zeros)"""
    x = np.atleast_2d(np.asarray(x, np.float32))
    taps = np.asarray(taps, np.float64)
    S, n = x.shape
    assert n % M == 0
    H = history(L, taps.size)
    hist = np.zeros((S, H), np.float32) if hist is None else np.asarray(hist, np.float32).reshape(S, H)
    xx = np.concatenate([hist, x], axis=1)
    x64 = xx.astype(np.float64)
    j = np.arange(n // M * L, dtype=np.int64)
    p, m = (j * M) % L, (j * M) // L + H
    acc = np.zeros((S, j.size), np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(-(-taps.size // L)):
            i = p + k * L
            ok = i < taps.size
            if not ok.any():
                break
            prod = taps[np.minimum(i, taps.size - 1)][None, :] * x64[:, np.where(ok, m - k, 0)]
            acc = np.where(ok[None, :], acc + prod, acc)
        y = acc.astype(np.float32)
    return y, xx[:, xx.shape[1] - H:].copy()


def capture(x, fmt, taps, L, M, hist=None):
    """[S, n] samples of `fmt` -> (float32 [S, n / M * L], history)"""
    return convert(sr.decode(np.atleast_2d(np.asarray(x)), fmt), taps, L, M, hist)


def playback(x, taps, L, M, fmt, lens=None, hist=None):
    """float32 [S, n] -> ([S, n / M * L] samples of `fmt`, history); lens: row s reads as 0.0 from lens[s] on"""
    x = np.atleast_2d(np.asarray(x, np.float32))
    if lens is not None:
        x = np.where(np.arange(x.shape[1])[None, :] < np.asarray(lens, np.int64)[:, None], x, np.float32(0.0))
    y, h = convert(x, taps, L, M, hist)
    return sr.encode(y, fmt), h
