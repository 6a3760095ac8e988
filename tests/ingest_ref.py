"""numpy reference of the capture formats (include/fskhip.h, FSKHIP_SAMPLES_*), shared by test_ingest_cpu.py -- which holds it against
Python's audioop -- and test_gpu_ingest.py, which holds the ingest kernel against it bit for bit."""
import numpy as np

FORMATS = {"f32": 0, "s16": 1, "mulaw": 2, "alaw": 3}
DTYPES = {"f32": np.float32, "s16": np.int16, "mulaw": np.uint8, "alaw": np.uint8}
LAYOUTS = {"stream": 0, "sample": 1}


def mulaw_to_linear(b):
    """G.711 mu-law code -> 16-bit linear value (int32 array), the header's formula"""
    u = (~np.asarray(b, np.uint8)).astype(np.int32) & 0xFF
    mag = ((((u & 15) << 3) + 0x84) << ((u >> 4) & 7)) - 0x84
    return np.where(u & 0x80, -mag, mag).astype(np.int32)


def alaw_to_linear(b):
    """G.711 A-law code -> 16-bit linear value (int32 array), the header's formula"""
    a = np.asarray(b, np.uint8).astype(np.int32) ^ 0x55
    e, m = (a >> 4) & 7, a & 15
    mag = np.where(e > 0, ((m << 4) + 0x108) << np.maximum(e - 1, 0), (m << 4) + 8)
    return np.where(a & 0x80, mag, -mag).astype(np.int32)


def decode(x, fmt, dtype=np.float32):
    """samples of format `fmt` -> their values in `dtype` (exact in float32: an integer of at most 16 bits times 2^-15)"""
    x = np.asarray(x)
    if fmt == "f32":
        return x.astype(dtype)
    lin = x.astype(np.int32) if fmt == "s16" else mulaw_to_linear(x) if fmt == "mulaw" else alaw_to_linear(x)
    return lin.astype(dtype) / dtype(32768)


def quantise(x, fmt):
    """float samples -> the nearest samples of format `fmt` (G.711: the nearest entry of the 256-value decode table)"""
    x = np.asarray(x, np.float32)
    if fmt == "f32":
        return x.copy()
    if fmt == "s16":
        return np.clip(np.rint(x.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16)
    table = decode(np.arange(256, dtype=np.uint8), fmt, np.float64)
    order = np.argsort(table, kind="stable")
    ts = table[order]
    xf = x.astype(np.float64)
    hi = np.clip(np.searchsorted(ts, xf), 1, 255)
    pick = np.where(np.abs(xf - ts[hi - 1]) <= np.abs(ts[hi] - xf), hi - 1, hi)
    return order[pick].astype(np.uint8)
