"""numpy reference of the encode direction of the capture formats (include/fskhip.h, "The same formats OUT"), shared by
test_egress_cpu.py -- which holds it against Python's audioop for every 16-bit value -- and test_gpu_egress.py, which holds the egress
kernel and fskhip_modulate_host_fmt against it bit for bit.  The decode direction is tests/ingest_ref.py."""
import numpy as np

from ingest_ref import DTYPES, FORMATS, LAYOUTS  # noqa: F401

SILENCE = {"f32": np.float32(0.0), "s16": np.int16(0), "mulaw": np.uint8(0xFF), "alaw": np.uint8(0xD5)}


def silence(fmt):
    """the element a stream is filled with from its length on: what 0.0f encodes to"""
    return SILENCE[fmt]


def to_s16(x):
    """float32 -> v = clamp(rne(x * 32768.0f), -32768, 32767) as int32; NaN gives 0, +-Inf saturate"""
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        y = np.rint(x * np.float32(32768.0))           # float32 arithmetic: the product is exact (or +-Inf)
    y = np.where(np.isnan(y), np.float32(0.0), y)
    return np.clip(y, -32768.0, 32767.0).astype(np.int32)


def _floor_log2(m):
    """floor(log2 m) of positive int32 values (m < 2^16)"""
    lg = np.zeros(m.shape, np.int32)
    for k in range(1, 16):
        lg += (m >> k) > 0
    return lg


def linear_to_mulaw(v):
    """16-bit linear value -> G.711 mu-law code, the header's formula"""
    m = np.asarray(v, np.int32) >> 2
    neg = m < 0
    m = np.minimum(np.abs(m), 8158) + 33
    seg = _floor_log2(m) - 5
    code = (seg << 4) | ((m >> (seg + 1)) & 15)
    return (code ^ np.where(neg, 0x7F, 0xFF)).astype(np.uint8)


def linear_to_alaw(v):
    """16-bit linear value -> G.711 A-law code, the header's formula"""
    m = np.asarray(v, np.int32) >> 3
    neg = m < 0
    m = np.where(neg, -m - 1, m)
    seg = np.maximum(_floor_log2(np.maximum(m, 1)) - 4, 0)
    code = (seg << 4) | ((m >> np.where(seg < 2, 1, seg)) & 15)
    return (code ^ np.where(neg, 0x55, 0xD5)).astype(np.uint8)


def encode(x, fmt):
    """float32 samples -> samples of format `fmt`, by the header's formulas (f32: the same bits)"""
    x = np.asarray(x, np.float32)
    if fmt == "f32":
        return x.copy()
    v = to_s16(x)
    if fmt == "s16":
        return v.astype(np.int16)
    return linear_to_mulaw(v) if fmt == "mulaw" else linear_to_alaw(v)
