"""CPU model of the two device-side generators every noisy test and every throughput number starts from, restated in numpy from
their contract in include/fskhip.h (fskhip_synth_device / fskhip_add_awgn_device) -- nothing here calls the library:

  fmix64                     the splitmix64 finaliser on uint64 arrays, wrapping
  payload_byte, stream_params  the synthesiser's payload bytes and per-stream lead-in / level
  gauss                      the counter-based standard normal keyed by (seed, stream, sample): Box-Muller in float64
  awgn                       x + sigma_s * gauss, sigma_s^2 = mean square of row s over its n columns / 10^(snr_db / 10)
  synth                      lead_s zeros, then modulateData frames back to back, every sample float32(float64(sample) * amp_s)

plus the cases tests/test_workload_cpu.py and tests/test_gpu_workload.py share."""
import numpy as np

from oracle import pyoracle as po

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
_M1, _M2 = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)
_LEAD_KEY = np.uint64(0xA5A5A5A5A5A5A5A5)
_TWO_M53 = 1.0 / 9007199254740992.0
TAIL_3SIGMA = 0.0026997960632601866          # P(|g| > 3) of a standard normal: erfc(3 / sqrt(2))


def _u64(v):
    """a uint64 array of v, which may be a Python int up to 2^64 - 1 or any integer array (never through float64)"""
    if isinstance(v, np.ndarray):
        return v.astype(np.uint64)
    if isinstance(v, (list, tuple, range)):
        return np.array([int(x) for x in v], dtype=np.uint64)
    return np.array(int(v), dtype=np.uint64)


def fmix64(z):
    z = _u64(z)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * _M1
        z = (z ^ (z >> np.uint64(27))) * _M2
        return z ^ (z >> np.uint64(31))


def _step(k):
    """GOLDEN * (1 + k), wrapping"""
    with np.errstate(over="ignore"):
        return GOLDEN * (np.uint64(1) + _u64(k))


def payload_byte(seed, s, frame, i):
    with np.errstate(over="ignore"):
        x = fmix64(_u64(seed) + _step(s))
        x = fmix64(x ^ _step(frame))
        x = fmix64(x + _step(i))
    return (x >> np.uint64(56)).astype(np.uint8)


def stream_params(seed, s, lead_max, amp_lo, amp_hi):
    """(lead_s, amp_s): lead_s = hash mod (lead_max + 1), amp_s = amp_lo + (amp_hi - amp_lo) * u with u in [0, 1)"""
    with np.errstate(over="ignore"):
        a = fmix64((_u64(seed) ^ _LEAD_KEY) + _step(s))
        b = fmix64(a + GOLDEN)
    lead = a % (_u64(lead_max) + np.uint64(1))
    u = (b >> np.uint64(11)).astype(np.float64) * _TWO_M53
    return lead, np.float64(amp_lo) + (np.float64(amp_hi) - np.float64(amp_lo)) * u


def gauss(seed, s, i):
    """standard normal sample i of stream s (s and i broadcast against each other), float64"""
    with np.errstate(over="ignore"):
        h = fmix64(fmix64(_u64(seed) + _step(s)) ^ _step(i))
        h2 = fmix64(h + GOLDEN)
    u1 = ((h >> np.uint64(11)).astype(np.float64) + 1.0) * _TWO_M53          # (0, 1]
    u2 = (h2 >> np.uint64(11)).astype(np.float64) * _TWO_M53                 # [0, 1)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * 3.14159265358979323846 * u2)


def awgn(x, snr_db, seed, first_stream=0):
    """(x + sigma_s * g as float64, sigma): x is [S, n], row r is stream first_stream + r of the whole batch"""
    x = np.asarray(x, dtype=np.float64)
    S, n = x.shape
    power = np.mean(x * x, axis=1) if n else np.zeros(S)
    sigma = np.sqrt(power / 10.0 ** (snr_db / 10.0))
    s = (np.arange(S, dtype=np.uint64) + np.uint64(first_stream))[:, None]
    g = gauss(seed, s, np.arange(n, dtype=np.uint64)[None, :])
    return x + sigma[:, None] * g, sigma


def spacing_f32(v):
    """the distance between neighbouring float32 values in the binade that holds |v| (subnormals: 2^-149)"""
    _, e = np.frexp(np.abs(np.asarray(v, dtype=np.float64)))                # |v| in [2^(e-1), 2^e); e = 0 for v = 0
    return np.ldexp(1.0, np.maximum(e.astype(np.int64) - 24, -149))


# ---- the synthesiser ------------------------------------------------------------------------------------------------

def _cfg_key(cfg):
    return tuple(sorted((k, tuple(v) if isinstance(v, (list, tuple)) else v) for k, v in (cfg or {}).items()))


class _Frames:
    """modulateData frames of one configuration: the oracle's, or float32(np.sin) / the V8 sine over the same phase chain"""

    def __init__(self, cfg):
        self.core = po.OracleCore(cfg)
        c = self.core.cfg
        self.spb = int(np.floor(c.sampleRate / c.baudRate))
        self.bits_per_byte = 8 + c.startBits + c.stopBits + (1 if c.parity != 0 else 0)
        self.head = [c.preamblePattern[i] for i in range(c.preambleLen)] + [c.sfdPattern[i] for i in range(c.sfdLen)]
        self.w = {1: 2 * np.pi * c.markFrequency / c.sampleRate, 0: 2 * np.pi * c.spaceFrequency / c.sampleRate}

    def frame_len(self, n_payload):
        n_bytes = len(self.head) + n_payload
        return (2 * self.spb if n_bytes else 0) + n_bytes * self.bits_per_byte * self.spb + self.bits_per_byte * self.spb

    def bits(self, payload):
        c, out = self.core.cfg, []
        for byte in self.head + list(payload):
            out += [0] * c.startBits + [(byte >> k) & 1 for k in range(7, -1, -1)]
            if c.parity != 0:
                par = bin(byte & 0xFF).count("1") & 1
                out.append(par if c.parity == 1 else 1 - par)
            out += [1] * c.stopBits
        return out

    def phases(self, payload):
        """the unwrapped float64 phase of every tone sample: 0, then one addition per sample in order"""
        inc = np.repeat(np.array([self.w[b] for b in self.bits(payload)], dtype=np.float64), self.spb)
        return np.concatenate([[0.0], np.cumsum(inc)[:-1]]) if inc.size else inc

    def frame(self, payload, sin="oracle"):
        want = self.frame_len(len(payload))
        if sin == "oracle":
            f = self.core.modulate(bytes(payload))
        else:
            ph = self.phases(payload)
            f = np.zeros(want, np.float32)
            lo = 2 * self.spb if ph.size else 0
            f[lo:lo + ph.size] = (np.sin(ph) if sin == "libm" else po.v8_sin(ph)).astype(np.float32)
        # the layout every frame offset below rests on: 2 bits of padding, the bytes, one byte time of silence
        assert f.size == want, "frame of %d samples, expected 2*spb + bytes*bitsPerByte*spb + bitsPerByte*spb = %d" % (f.size, want)
        return f


def stream_cfgs(cfgs, S):
    return [dict(cfgs)] * S if isinstance(cfgs, dict) else [dict(c) for c in cfgs]


def synth(cfgs, S, n, payload_len, seed, lead_max, amp_lo, amp_hi, sin="oracle"):
    """[S, n] float32: what fskhip_synth_device writes.  sin = "oracle": frames from OracleCore.modulate; "libm" / "v8": np.sin / the
    V8 sine over the model's own phase chain."""
    per = stream_cfgs(cfgs, S)
    assert len(per) == S
    gens = {}
    lead, amp = stream_params(seed, np.arange(S), lead_max, amp_lo, amp_hi)
    out = np.zeros((S, n), np.float32)
    for s in range(S):
        key = _cfg_key(per[s])
        if key not in gens:
            gens[key] = _Frames(per[s])
        gen = gens[key]
        t, k = int(lead[s]), 0
        while t < n:
            payload = payload_byte(seed, s, k, np.arange(payload_len)).tolist()
            f = (gen.frame(payload, sin).astype(np.float64) * amp[s]).astype(np.float32)
            m = min(f.size, n - t)
            out[s, t:t + m] = f[:m]
            t += f.size
            k += 1
    return out


# ---- the cases of the synthesiser checks (tests/test_gpu_workload.py; the cap check of tests/test_workload_cpu.py) ----------------

BASE = dict(baudRate=1200, markFrequency=1200, spaceFrequency=2200)          # Bell-202 at 48 kHz: 40 samples per bit
N_BASE = 6007          # two whole 2 480-sample frames and a cut third behind any lead-in; no multiple of the 32-sample tile nor of 4
SEED = 0xF5C0DE
MAX_DIFFERENT = 2      # samples of one case that may differ from the model at all (device sine against the V8 sine)


def tone_pairs(S):
    """BASELINE config #4's rule: stream s has its own mark / space pair"""
    return [dict(BASE, markFrequency=1000 + 10 * (s % 100), spaceFrequency=1200 + 10 * (s % 100)) for s in range(S)]


def synth_cases():
    """name -> dict(cfgs, S, n, payload_len, seed, lead_max, amp_lo, amp_hi)"""
    def case(cfgs=BASE, S=70, n=N_BASE, payload_len=2, seed=SEED, lead_max=400, amp_lo=0.1, amp_hi=1.0):
        return dict(cfgs=cfgs, S=S, n=n, payload_len=payload_len, seed=seed, lead_max=lead_max, amp_lo=amp_lo, amp_hi=amp_hi)
    cases = {
        "one-stream": case(S=1),
        "ragged-wave": case(),
        "tone-pairs": case(cfgs=tone_pairs(70)),
        "parity-two-stop": case(cfgs=dict(BASE, parity="even", stopBits=2), S=3),
        "odd-parity": case(cfgs=dict(BASE, parity="odd"), S=3),
        "no-lead": case(S=3, lead_max=0),
        "lead-beyond-n": case(lead_max=7000),
        "one-level": case(S=3, amp_lo=0.5, amp_hi=0.5),
    }
    for n in (1, 31, 32, 33, 97):          # 97: the first tone samples (from column 80) in a cut fourth tile
        cases["n-%d" % n] = case(n=n, lead_max=0)
    return cases
