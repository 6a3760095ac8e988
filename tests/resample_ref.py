"""The model of the resampler (include/fskhip_next.h: fskhip_resampler_*): the reference's FIRFilter over the zero-stuffed signal (up), and
with every L-th output kept and encoded (down).  Not a test; test_resample_cpu.py holds it against np.convolve, and test_gpu_resample.py
the kernels against it."""
import numpy as np

import samples_ref as sr
from oracle import pyoracle as po


def default_taps(factor, low_rate=8000.0, up=False):
    """what Upsampler / Downsampler design with taps=None, from the model's own sincLowpass"""
    taps = np.array(po.sinc("lowpass", 0.45 * low_rate, factor * low_rate, 16 * factor + 1), np.float64)
    return taps * float(factor) if up else taps


def stuff(x, fmt, L):
    """samples of format `fmt`, [S, n] -> their values with L - 1 zeros behind each, float32 [S, n L]"""
    x = np.atleast_2d(np.asarray(x))
    z = np.zeros((x.shape[0], x.shape[1] * L), np.float32)
    z[:, ::L] = sr.decode(x, fmt)
    return z


def fir(x, taps, filters=None):
    """FIRFilter(taps).processBuffer on every row of float32 [S, n]; `filters`: one po.FIR per row, to carry the delay lines"""
    x = np.atleast_2d(np.asarray(x, np.float32))
    filters = filters or [po.FIR(list(taps)) for _ in range(x.shape[0])]
    return np.stack([f.process_buffer(row) for f, row in zip(filters, x)]) if x.shape[1] else x.copy()


def up(x, fmt, taps, L, filters=None):
    """[S, n] samples of `fmt` -> float32 [S, n L]"""
    return fir(stuff(x, fmt, L), taps, filters)


def down(x, taps, L, fmt, lens=None, filters=None):
    """float32 [S, n], n a multiple of L -> [S, n / L] samples of `fmt`; lens: row s reads as 0.0 from lens[s] on"""
    x = np.atleast_2d(np.asarray(x, np.float32))
    assert x.shape[1] % L == 0
    if lens is not None:
        x = np.where(np.arange(x.shape[1])[None, :] < np.asarray(lens, np.int64)[:, None], x, np.float32(0.0))
    return sr.encode(fir(x, taps, filters)[:, ::L], fmt)
