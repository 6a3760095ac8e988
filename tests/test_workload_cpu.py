"""The CPU model of the synthesiser and the AWGN generator (tests/workload_ref.py) on its own, without a GPU:

  * its payload bytes and per-stream lead-in / level equal the library's host functions on a grid of seeds, streams and frames;
  * its Gaussian generator is standard normal and independent along every axis of its key, each statistic within 5 of its own
    standard errors, and the noise it adds realises the requested SNR within the same bound;
  * over the phases of the GPU synthesiser cases, float32(libm sine) and the oracle's V8 sine differ in no more samples than the GPU
    check (tests/test_gpu_workload.py) allows, so a correctly rounded device sine cannot miss it."""
import ctypes as C

import numpy as np
import pytest

import workload_ref as wr

SEEDS = [0, 1, 0xA36, 0xF5C0DE, 2 ** 64 - 1]
STREAMS = [0, 1, 63, 64, 32767, 32768, 2 ** 32 - 1]
N_SE = 5.0


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from webaudio_modem_amd import _lib
    return _lib.lib()


def test_fmix64_is_the_splitmix64_finaliser():
    """the first outputs of splitmix64 from state 0 (its published test vector): output k = fmix64(k * GOLDEN)"""
    got = wr.fmix64([(k * 0x9E3779B97F4A7C15) % 2 ** 64 for k in (1, 2, 3)])
    assert [int(v) for v in got] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    assert int(wr.fmix64(0)) == 0 and int(wr.fmix64(2 ** 64 - 1)) == int(wr.fmix64(np.array([2 ** 64 - 1], np.uint64))[0])


def test_payload_bytes_equal_the_host_function(L):
    n = 0
    for seed in SEEDS:
        for s in STREAMS:
            for frame in (0, 1, 1000):
                idx = [0, 1, 255]
                want = [L.fskhip_synth_payload_byte(seed, s, frame, i) for i in idx]
                assert wr.payload_byte(seed, s, frame, idx).tolist() == want, (seed, s, frame)
                n += len(idx)
    assert n == 5 * 7 * 3 * 3
    # ... and broadcast over streams and frames at once
    got = wr.payload_byte(0xF5C0DE, np.array(STREAMS, np.uint64)[:, None], np.array([0, 1, 1000], np.uint64)[None, :], 7)
    assert got.tolist() == [[L.fskhip_synth_payload_byte(0xF5C0DE, s, f, 7) for f in (0, 1, 1000)] for s in STREAMS]


def test_stream_params_equal_the_host_function(L):
    lead, amp = C.c_uint32(), C.c_double()
    for seed in SEEDS:
        for lead_max in (0, 1, 400, 2 ** 32 - 1):
            for lo, hi in ((0.1, 1.0), (0.37, 0.37)):
                m_lead, m_amp = wr.stream_params(seed, STREAMS, lead_max, lo, hi)
                for k, s in enumerate(STREAMS):
                    L.fskhip_synth_stream_params(seed, s, lead_max, lo, hi, C.byref(lead), C.byref(amp))
                    assert (int(m_lead[k]), float(m_amp[k])) == (lead.value, amp.value), (seed, s, lead_max, lo, hi)   # the double bit for bit
                    assert lead.value <= lead_max and lo <= amp.value <= hi
                    if lo == hi:
                        assert amp.value == lo
                    if lead_max == 0:
                        assert lead.value == 0
    # the lead-ins spread over their whole range
    m_lead, m_amp = wr.stream_params(0xF5C0DE, np.arange(4096), 400, 0.1, 1.0)
    assert len(set(m_lead.tolist())) > 380 and m_amp.min() < 0.11 and m_amp.max() > 0.99


# ---- the generator is standard normal and independent -------------------------------------------------------------------------

def _corr(a, b):
    a, b = a.ravel(), b.ravel()
    return float(np.mean((a - a.mean()) * (b - b.mean())) / (a.std() * b.std()))


def _moments(g):
    """(name, value, expected, standard error) of the sample moments and the 3-sigma tail of N samples"""
    n = g.size
    z = (g - g.mean()) / g.std()
    p = wr.TAIL_3SIGMA
    return [("mean", float(g.mean()), 0.0, 1 / np.sqrt(n)), ("variance", float(g.var()), 1.0, np.sqrt(2.0 / n)),
            ("skewness", float(np.mean(z ** 3)), 0.0, np.sqrt(6.0 / n)), ("excess kurtosis", float(np.mean(z ** 4)) - 3.0, 0.0, np.sqrt(24.0 / n)),
            ("beyond 3 sigma", float(np.mean(np.abs(g) > 3.0)), p, np.sqrt(p * (1 - p) / n))]


def _hold(stats, where):
    worst = 0.0
    for name, got, want, se in stats:
        dev = abs(got - want) / se
        print("%-34s %-28s %+.6f  expected %.6f  %.2f standard errors" % (where, name, got, want, dev))
        assert dev <= N_SE, (where, name, got, want, se)
        worst = max(worst, dev)
    return worst


@pytest.mark.parametrize("seed", [0xA36, 0xBEE, 0, 1])
def test_gauss_is_standard_normal_and_independent(seed):
    """2^20 samples of one stream, and a 4 096-stream x 256-sample grid: every statistic within 5 of its standard errors.
    (Largest deviation seen on these seeds: 2.6 standard errors.)"""
    n = 1 << 20
    i = np.arange(n, dtype=np.uint64)
    g = wr.gauss(seed, 0, i)
    assert np.isfinite(g).all() and np.abs(g).max() < 8.6            # sqrt(-2 ln 2^-53) = 8.57
    stats = _moments(g)
    for lag in (1, 2, 3, 4, 256):
        stats.append(("autocorrelation, lag %d" % lag, _corr(g[:-lag], g[lag:]), 0.0, 1 / np.sqrt(n - lag)))
    stats.append(("seed against seed + 1", _corr(g, wr.gauss(seed + 1, 0, i)), 0.0, 1 / np.sqrt(n)))
    _hold(stats, "seed %#x, one stream" % seed)

    S, m = 4096, 256
    s = np.arange(S, dtype=np.uint64)[:, None]
    j = np.arange(m, dtype=np.uint64)[None, :]
    grid = wr.gauss(seed, s, j)
    stats = _moments(grid)
    stats.append(("adjacent streams, equal i", _corr(grid[:-1], grid[1:]), 0.0, 1 / np.sqrt((S - 1) * m)))
    for lag in (1, 2, 3, 4):
        stats.append(("autocorrelation, lag %d" % lag, _corr(grid[:, :-lag], grid[:, lag:]), 0.0, 1 / np.sqrt(S * (m - lag))))
    stats.append(("seed against seed + 1", _corr(grid, wr.gauss(seed + 1, s, j)), 0.0, 1 / np.sqrt(S * m)))
    swapped = wr.gauss(seed, np.broadcast_to(j, (S, m)), np.broadcast_to(s, (S, m)))     # (i, s) for (s, i)
    off = np.broadcast_to(s, (S, m)) > np.broadcast_to(j, (S, m))                        # every unordered pair once, none with s = i
    stats.append(("(s, i) against (i, s)", _corr(grid[off], swapped[off]), 0.0, 1 / np.sqrt(off.sum())))
    _hold(stats, "seed %#x, 4096 x 256 grid" % seed)


def test_model_noise_realises_the_requested_snr():
    """sigma_s^2 * mean(g^2) over one synthesised row: the realised noise power is the requested one within 5 standard errors of a
    mean of n squared normals (sqrt(2 / n)), per stream and pooled"""
    c = wr.synth_cases()["ragged-wave"]
    x = wr.synth(**c)
    n = c["n"]
    for snr_db, seed in ((-3.0, 0xA36), (10.0, 0xBEE), (40.0, 0), (10.0, 1)):
        y, sigma = wr.awgn(x, snr_db, seed)
        power = np.mean(x.astype(np.float64) ** 2, axis=1)
        np.testing.assert_allclose(sigma ** 2, power / 10.0 ** (snr_db / 10.0), rtol=1e-14)
        ratio = np.mean((y - x) ** 2, axis=1) / (power / 10.0 ** (snr_db / 10.0))          # 1 at exactly the requested SNR
        worst = np.abs(ratio - 1).max() / np.sqrt(2.0 / n)
        pooled = abs(ratio.mean() - 1) / np.sqrt(2.0 / (n * c["S"]))
        print("snr %5.1f dB seed %#x: realised %.4f .. %.4f dB, worst stream %.2f standard errors, pooled %.2f"
              % (snr_db, seed, snr_db - 10 * np.log10(ratio.max()), snr_db - 10 * np.log10(ratio.min()), worst, pooled))
        assert worst <= N_SE and pooled <= N_SE


def test_model_rejects_a_frame_of_another_length():
    """the frame layout the model assumes is asserted, not trusted"""
    f = wr._Frames(wr.BASE)
    assert f.frame_len(2) == 2 * 40 + 5 * 10 * 40 + 10 * 40 == f.frame([1, 2]).size
    f.spb += 1
    with pytest.raises(AssertionError, match="frame of 2480 samples"):
        f.frame([1, 2])


def test_libm_sine_stays_within_the_gpu_cap():
    """Cap check for the synthesiser comparison: over every phase of the GPU cases, float32(np.sin(phase)) against the oracle's
    V8-sine frames.  Observed with glibc on these seeds: 0 different samples in every case (cap: 2 per case), so whatever
    differs on the device is the device's.  The model's own phase chain with the V8 sine is the oracle's frame bit for bit."""
    total = 0
    for name, c in wr.synth_cases().items():
        ref = wr.synth(**c)
        assert np.array_equal(wr.synth(sin="v8", **c).view(np.uint32), ref.view(np.uint32)), name
        # unscaled: the sine itself, one level for every stream
        plain = dict(c, amp_lo=1.0, amp_hi=1.0)
        a, b = wr.synth(sin="libm", **plain), wr.synth(**plain)
        d = a != b
        print("%-16s %7d samples, %7d tones: %d differ" % (name, a.size, int((b != 0).sum()), int(d.sum())))
        assert d.sum() <= wr.MAX_DIFFERENT, name
        assert (np.abs(a[d].astype(np.float64) - b[d]) == np.spacing(np.minimum(np.abs(a[d]), np.abs(b[d]))).astype(np.float64)).all(), name
        assert (wr.synth(sin="libm", **c) != ref).sum() <= wr.MAX_DIFFERENT, name
        total += int(d.sum())
    print("different samples over all cases: %d" % total)
