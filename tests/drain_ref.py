"""What the compacted RX drain's tests share (no test in here): processor snapshot images rewritten in numpy -- ring words, ring
bytes, checksum, after the layout in include/fskhip_next.h -- so that a test sets every stream's ring state directly instead
of demodulating a signal for it, and the numpy expectation of fskhip_processor_rx_drain_sparse_host over such an image: which
streams, their CSR offsets, their bytes, and the image afterwards.  Nothing here calls the code under test."""
import numpy as np

HEADER_BYTES = 48
REC_FIXED = 64
MAGIC = 0x504B5346   # "FSKP"


def checksum(image):
    """the stream snapshot's function over the image's little-endian u64 words w, the checksum field (bytes 32..39) taken as 0:
    a += w, b += a (mod 2^64); a * 0x9E3779B97F4A7C15 ^ b"""
    w = np.frombuffer(bytes(image), dtype="<u8").copy()
    w[4] = 0
    n = np.uint64(len(w))
    with np.errstate(over="ignore"):
        a = w.sum(dtype=np.uint64)
        b = (w * (n - np.arange(len(w), dtype=np.uint64))).sum(dtype=np.uint64)   # w[j] is added to b once for every word from j on
        return int(a * np.uint64(0x9E3779B97F4A7C15) ^ b)


def blank_image(n_streams, rx_capacity):
    """the image of n_streams freshly created processors (nothing pending: payload_capacity 0), checksum included"""
    rec = REC_FIXED + ((rx_capacity + 15) & ~15)
    img = np.zeros(HEADER_BYTES + n_streams * rec, np.uint8)
    img[:32].view("<u4")[:] = [MAGIC, 1, HEADER_BYTES, rec, n_streams, rx_capacity, 0, 0]
    return seal(img)


def seal(img):
    img[32:40].view("<u8")[0] = 0
    img[32:40].view("<u8")[0] = checksum(img)
    return img


class Rings:
    """the ring part of an image of processors with nothing pending: r (readIndex), n (_length) per stream, and the ring bytes
    [n_streams][rx_capacity]; writeIndex follows (r + n mod capacity)"""

    def __init__(self, r, n, ring):
        self.r, self.n, self.ring = np.asarray(r, np.int64), np.asarray(n, np.int64), np.asarray(ring, np.uint8)
        self.n_streams, self.cap = self.ring.shape

    def live(self):
        """[n_streams][cap] bool: the bytes inside [r, r + n) modulo cap"""
        x = np.arange(self.cap)[None, :]
        return (x - self.r[:, None]) % self.cap < self.n[:, None]

    def image(self, fresh=None):
        """the canonical image (ring bytes outside the live span are zero): the records of `fresh` -- the processor image of a newly
        created batch of this shape; None: blank_image's -- rewritten"""
        img = blank_image(self.n_streams, self.cap) if fresh is None else np.frombuffer(bytes(fresh), np.uint8).copy()
        assert list(img[:32].view("<u4")[[0, 1, 2, 4, 5, 6]]) == [MAGIC, 1, HEADER_BYTES, self.n_streams, self.cap, 0]
        rec = int(img[12:16].view("<u4")[0])
        recs = img[HEADER_BYTES:].reshape(self.n_streams, rec)
        words = np.zeros((self.n_streams, 4), "<u4")
        words[:, 0], words[:, 1], words[:, 2] = (self.r + self.n) % self.cap, self.r, self.n
        recs[:, :16] = words.view(np.uint8).reshape(self.n_streams, 16)
        recs[:, REC_FIXED:REC_FIXED + self.cap] = np.where(self.live(), self.ring, 0)
        return seal(img).tobytes()

    def stream_bytes(self, s):
        """what a drain returns for stream s: its live bytes, oldest first"""
        return self.ring[s, (self.r[s] + np.arange(self.n[s])) % self.cap].tobytes()

    def drained(self, mask=None, min_len=1):
        """(streams, offsets, data, Rings afterwards) of a sparse drain with these arguments"""
        sel = self.n >= max(min_len, 1)
        if mask is not None:
            sel &= np.asarray(mask, bool)
        streams = np.flatnonzero(sel)
        offsets = np.concatenate([[0], np.cumsum(self.n[streams])])
        data = b"".join(self.stream_bytes(s) for s in streams)
        after = Rings(np.where(sel, (self.r + self.n) % self.cap, self.r), np.where(sel, 0, self.n), self.ring)
        return streams.astype(np.uint32), offsets.astype(np.uint32), np.frombuffer(data, np.uint8), after


def random_rings(rng, n_streams, cap, density):
    """density: 'empty', 'full', 'one_in_500' or 'random30' -- which streams hold bytes; those hold 1..cap (a quarter of them exactly
    cap: full rings), from a random readIndex (so about half the spans wrap)"""
    if density == "empty":
        has = np.zeros(n_streams, bool)
    elif density == "full":
        has = np.ones(n_streams, bool)
    elif density == "one_in_500":
        has = np.arange(n_streams) % 500 == int(rng.integers(0, min(500, n_streams)))
    else:
        has = rng.random(n_streams) < 0.3
    n = np.where(rng.random(n_streams) < 0.25, cap, rng.integers(1, cap + 1, n_streams))
    n = np.where(has, cap if density == "full" else n, 0)
    r = rng.integers(0, cap, n_streams)
    ring = rng.integers(1, 256, (n_streams, cap), dtype=np.uint8)   # (no zero byte: a byte taken from outside the live span shows)
    return Rings(r, n, ring)
