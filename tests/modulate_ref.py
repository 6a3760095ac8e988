"""What the modulator tests share (tests/test_oracle_modulate_edges.py on the CPU, tests/test_gpu_modulate.py on the GPU): the goldens
of oracle/refrun/golden_harness_modulate.js, the comparisons, the configurations and ragged payloads of the sweeps, the oracle's
signals (computed once per configuration and payload), and a sentinel-framed device buffer for ragged rows."""
import functools
import hashlib
import json
import os

import numpy as np

from conftest import GOLDEN_DIR, load_npz

SENTINEL = 0xDEADBEEF
GUARD = 256                 # sentinel words in front of the first row's allocation slot and behind the last row

# samplesPerBit -> sampleRate, baudRate, mark, space (golden_harness_modulate.js's table, plus 3 for the pitches that cut at 31 .. 33)
RATES = {3: (48000, 16000, 6000, 12000), 5: (48000, 9600, 9600, 14400), 10: (48000, 4800, 9600, 14400), 20: (48000, 2400, 2400, 4800),
         31: (48000, 1548, 1200, 2200), 32: (48000, 1500, 1200, 2200), 33: (48000, 1454, 1200, 2200), 40: (48000, 1200, 1200, 2200),
         64: (48000, 750, 1200, 2200), 147: (44100, 300, 1070, 1270)}
SPBS = [5, 10, 20, 31, 32, 33, 40, 64, 147]
FRAMINGS = {"8n1": {}, "even_stop2": {"parity": "even", "stopBits": 2}, "odd_start2": {"parity": "odd", "startBits": 2},
            "nopre": {"preamblePattern": [], "sfdPattern": []}, "pre4": {"preamblePattern": [0xAA, 0x55, 0xAA, 0x55]}}


def config(spb, framing="8n1", tones=None):
    sr, baud, mark, space = RATES[spb]
    assert sr // baud == spb
    if tones is not None:
        mark, space = tones
    return dict(sampleRate=sr, baudRate=baud, markFrequency=mark, spaceFrequency=space, **FRAMINGS[framing])


class GoldenModulate:
    """tests/golden/golden_modulate.npz + manifest_modulate.json: `short` cases with their whole signal; `long` cases with n, the
    index `cross` of the first sample whose phase is beyond the case's limit, a SHA-256 of the samples before it and the samples
    from it on.  limit "stated": 2^19 * pi/2, what fdlibm's comment names; "actual": the high-word test its code makes, 2^20 * pi/2."""

    def __init__(self):
        with open(os.path.join(GOLDEN_DIR, "manifest_modulate.json")) as fh:
            self.manifest = json.load(fh)
        self.arrays = load_npz("golden_modulate.npz")
        self.short = self.manifest["modulate"]
        self.long = self.manifest["modulate_long"]

    def array(self, name):
        return self.arrays[name]


_GOLDEN = None


def golden_modulate():
    global _GOLDEN
    if _GOLDEN is None:
        _GOLDEN = GoldenModulate()
    return _GOLDEN


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a, "<f4").tobytes()).hexdigest()


def differing(sig, ref):
    """number of samples whose bits differ"""
    return int(np.count_nonzero(bits(sig) != bits(ref)))


def within_one_spacing(sig, ref):
    """every sample within one float32 spacing (at the larger magnitude of the two) of the reference's"""
    a, b = sig.astype(np.float64), ref.astype(np.float64)
    return bool(np.all(np.abs(a - b) <= np.spacing(np.maximum(np.abs(sig), np.abs(ref)).astype(np.float32)).astype(np.float64)))


def check_signal(sig, ref, exact, what=""):
    """fp64 engines (exact): the reference's bits.  fp32 engines: tests/test_gpu_parity.py's bar for test_modulate_matches_reference_golden
    per signal -- |diff| <= 1.2e-7, at most max(1, n // 10000) differing samples -- with the exactly-zero samples and the length
    identical.  Returns the number of differing samples."""
    assert sig.size == ref.size, (what, sig.size, ref.size)
    if exact:
        assert np.array_equal(bits(sig), bits(ref)), (what, "first differing sample", int(np.flatnonzero(bits(sig) != bits(ref))[0]))
        return 0
    if sig.size == 0:
        return 0
    assert np.array_equal(bits(sig) == 0, bits(ref) == 0), (what, "exactly-zero samples differ")
    diff = np.abs(sig.astype(np.float64) - ref.astype(np.float64))
    n_diff = int(np.count_nonzero(diff))
    assert diff.max() <= 1.2e-7, (what, float(diff.max()))
    assert n_diff <= max(1, sig.size // 10000), (what, n_diff, sig.size)
    return n_diff


def _key(cfg):
    return json.dumps(cfg, sort_keys=True)


@functools.lru_cache(maxsize=None)
def _oracle_signal(cfg_key, payload):
    from oracle import pyoracle as po
    sig = po.OracleCore(json.loads(cfg_key)).modulate(payload)
    sig.setflags(write=False)
    return sig


def oracle_signal(cfg, payload):
    """OracleCore(cfg).modulate(payload): read-only, computed once"""
    return _oracle_signal(_key(cfg), bytes(payload))


def ragged_payloads(S, max_len, seed):
    """S payloads of seeded random bytes and lengths 0 .. max_len: 0, 1 and max_len always among them, a 0-length stream in the last
    wave (the partly filled one where S is no multiple of 64), and -- from two streams on -- stream 0 neither empty nor the longest"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, max_len + 1, S)
    if S >= 4:
        lens[0], lens[1], lens[2], lens[S - 1] = max(1, max_len // 2), 0, max_len, 0
        lens[3] = 1
        first = 64 * ((S - 1) // 64)
        if first > 0 and S - first >= 2:
            lens[first] = max_len                         # ... beside a stream with tones to its end
    elif S == 1:
        lens[0] = max_len
    return [bytes(rng.integers(0, 256, int(n), dtype=np.uint8)) for n in lens]


class RaggedRows:
    """An [S, pitch] float32 device buffer whose first element lies `shift` bytes behind a 16-byte boundary, inside an allocation of
    sentinel words (tests/test_gpu_workload.py's Rows, for rows of different lengths): check(signals, lens) asserts that row s holds
    signals[s][:lens[s]] from column 0 and that every other word -- the rest of the row, the words in front of the buffer and behind
    it -- still holds its sentinel, and returns the largest number of differing samples of one row."""

    def __init__(self, caller, S, pitch, shift=0):
        assert shift % 4 == 0
        self.c, self.S, self.pitch, self.lead = caller, S, pitch, GUARD + shift // 4
        self.words = self.lead + S * pitch + GUARD
        self.base = caller.malloc(self.words * 4)
        assert self.base % 16 == 0
        self.ptr = self.base + 4 * self.lead
        caller.upload(self.base, np.full(self.words, SENTINEL, np.uint32))

    def read(self):
        self.c.sync()
        host = self.c.download(self.base, np.empty(self.words, np.uint32))
        assert (host[:self.lead] == SENTINEL).all(), "written in front of the buffer"
        assert (host[self.lead + self.S * self.pitch:] == SENTINEL).all(), "written behind the last row"
        return host[self.lead:self.lead + self.S * self.pitch].reshape(self.S, self.pitch)

    def check(self, signals, lens, exact):
        body, worst = self.read(), 0
        for s in range(self.S):
            n = int(lens[s])
            assert (body[s, n:] == SENTINEL).all(), ("row %d written from column %d on" % (s, n), np.flatnonzero(body[s, n:] != SENTINEL)[:4] + n)
            worst = max(worst, check_signal(body[s, :n].view(np.float32), signals[s][:n], exact, "row %d" % s))
        return worst
