"""numpy reference of the capture formats in both directions (include/fskhip.h, FSKHIP_SAMPLES_* and "The same formats OUT"), shared by
test_ingest_cpu.py and test_egress_cpu.py -- which hold it against Python's audioop, for every code and for every 16-bit value -- and
test_gpu_ingest.py and test_gpu_egress.py, which hold the kernels and the host calls against it bit for bit."""
import numpy as np

FORMATS = {"f32": 0, "s16": 1, "mulaw": 2, "alaw": 3}
DTYPES = {"f32": np.float32, "s16": np.int16, "mulaw": np.uint8, "alaw": np.uint8}
LAYOUTS = {"stream": 0, "sample": 1}
SILENCE = {"f32": np.float32(0.0), "s16": np.int16(0), "mulaw": np.uint8(0xFF), "alaw": np.uint8(0xD5)}


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
