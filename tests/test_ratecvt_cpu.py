"""The rational rate converter's model without a GPU (tests/ratecvt_ref.py; include/fskhip_next.h: fskhip_ratecvt_*):
  * with M = 1 the model is resample_ref's interpolator and with L = 1 its decimator, bit for bit, and for a ratio it is the
    reference's FIRFilter over the zero-stuffed input, columns ::M;
  * it is cut-invariant over random cuts in multiples of M, the history included;
  * what the feature is for, through the model and the oracle: modulate at 48 kHz, convert to 44.1 kHz with the default
    PlaybackConverter design into s16, mu-law and A-law, convert back with the default CaptureConverter design, demodulate --
    every payload byte comes back for the default configuration, Bell 202 and 300 baud.  The default designs (2 561 taps, a
    Hamming-windowed sinc at 19 845 Hz, 16 taps per phase of the larger factor) carried every configuration as they are, so
    neither numTaps nor the cutoff was changed;
  * the host arithmetic (csrc/fsk_ratecvt_plan.h) from a stand-alone program under AddressSanitizer and UBSan, and the GPU tests'
    own copy of its cut (where they place a length one period past a segment) against what that program prints;
  * what a process call of this unit and of the resampler is refused for (csrc/fsk_rate_call.h), from another such program.
The model tests need nothing of the library, so they hold with or without the converter; what fails without it are the plan test
here, tests/test_ratecvt_refusals_cpu.py and tests/test_gpu_ratecvt.py."""
import os
import subprocess

import numpy as np
import pytest

import ratecvt_ref as rc
import resample_ref as rr
import samples_ref as sr
from conftest import ROOT
from oracle import pyoracle as po


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


@pytest.mark.parametrize("factor,n_taps", [(1, 5), (2, 1), (3, 13), (6, 97), (6, 5), (7, 3)])
def test_model_is_the_integer_resamplers(factor, n_taps):
    rng = np.random.default_rng(factor * 100 + n_taps)
    taps = rng.uniform(-1, 1, n_taps)
    x = rng.integers(-32768, 32768, (3, 50)).astype(np.int16)
    got, hist = rc.capture(x, "s16", taps, factor, 1)
    assert np.array_equal(_bits(got), _bits(rr.up(x, "s16", taps, factor)))
    H = rc.history(factor, n_taps)
    assert hist.shape == (3, H) and np.array_equal(hist, sr.decode(x, "s16")[:, 50 - H:])
    u = rng.uniform(-1, 1, (3, 20 * factor)).astype(np.float32)
    for fmt in ("f32", "s16", "mulaw", "alaw"):
        got, hist = rc.playback(u, taps, 1, factor, fmt)
        assert np.array_equal(_bits(got), _bits(rr.down(u, taps, factor, fmt)))
    assert hist.shape == (3, n_taps - 1) and np.array_equal(hist, u[:, u.shape[1] - (n_taps - 1):])
    lens = [0, 5, 20 * factor]
    got, hist = rc.playback(u, taps, 1, factor, "mulaw", lens=lens)
    assert np.array_equal(got, rr.down(u, taps, factor, "mulaw", lens=lens))
    assert (hist[0] == 0).all() and (got[1, rc.out_length(1, factor, n_taps, 5):] == sr.silence("mulaw")).all()


@pytest.mark.parametrize("L,M,n_taps", [(3, 2, 13), (2, 3, 13), (7, 5, 6), (7, 5, 113), (1, 1, 4), (160, 147, 2561), (147, 160, 159)])
def test_model_is_the_fir_over_the_stuffed_input(L, M, n_taps):
    rng = np.random.default_rng(L * 1000 + M + n_taps)
    taps = rng.uniform(-1, 1, n_taps)
    x = rng.uniform(-1, 1, (2, 3 * M)).astype(np.float32)
    got, _ = rc.convert(x, taps, L, M)
    want = rr.fir(rr.stuff(x, "f32", L), taps)[:, ::M]
    assert got.shape == (2, 3 * L) and np.array_equal(got, want)      # (== : a zero's sign may differ)


@pytest.mark.parametrize("L,M,n_taps", [(3, 2, 13), (2, 3, 1), (7, 5, 6), (160, 147, 2561), (147, 160, 2561), (1, 4, 9)])
def test_model_is_cut_invariant(L, M, n_taps):
    rng = np.random.default_rng(L + 7 * M + n_taps)
    taps = rng.uniform(-1, 1, n_taps)
    periods = 9
    x = rng.uniform(-1, 1, (3, periods * M)).astype(np.float32)
    whole, hist = rc.convert(x, taps, L, M)
    for _ in range(3):
        cuts = [0] + sorted(rng.choice(np.arange(1, periods), size=3, replace=False).tolist()) + [periods]
        h, parts = None, []
        for a, b in zip(cuts[:-1], cuts[1:]):
            y, h = rc.convert(x[:, a * M:b * M], taps, L, M, h)
            parts.append(y)
        assert np.array_equal(_bits(np.concatenate(parts, axis=1)), _bits(whole)) and np.array_equal(_bits(h), _bits(hist))
    assert rc.out_length(L, M, n_taps, 0) == 0
    # out_length: an impulse as the last of n inputs rings exactly that far when no tap is zero
    n = 2 * M
    imp = np.zeros((1, 4 * M + -(-n_taps // L) * M), np.float32)
    imp[0, n - 1] = 1.0
    y, _ = rc.convert(imp, np.ones(n_taps), L, M)
    nz = np.nonzero(y[0])[0]
    length = rc.out_length(L, M, n_taps, n)
    assert length <= y.shape[1] and not y[0, length:].any()
    if (length - 1) * M >= (n - 1) * L:          # (a kept output falls into the ringing at all)
        assert nz[-1] + 1 == length and nz[0] == -(-(n - 1) * L // M)
    else:
        assert nz.size == 0


CONFIGS = {"default": None, "bell202": dict(baudRate=1200, markFrequency=1200, spaceFrequency=2200),
           "300baud": dict(baudRate=300, markFrequency=1650, spaceFrequency=1850)}


@pytest.fixture(scope="module")
def designs():
    return rc.default_taps(48000, 44100), rc.default_taps(44100, 48000)


@pytest.mark.parametrize("fmt", ["s16", "mulaw", "alaw"])
@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_round_trip_at_44100_through_the_model(cfg, fmt, designs):
    """48 kHz modulate -> x 147 / 160 -> a format at 44.1 kHz -> x 160 / 147 -> demodulate, default designs: all 32 bytes"""
    down_taps, up_taps = designs
    assert len(down_taps) == len(up_taps) == 2561
    payload = bytes(range(40, 72))
    tx, rx = po.OracleCore(CONFIGS[cfg]), po.OracleCore(CONFIGS[cfg])
    x = np.concatenate([np.zeros(480, np.float32), np.asarray(tx.modulate(payload), np.float32), np.zeros(4800, np.float32)])
    x = x[:x.size // 160 * 160]
    low, _ = rc.playback(x, down_taps, 147, 160, fmt)
    assert low.shape == (1, x.size // 160 * 147) and low.dtype == sr.DTYPES[fmt]
    high, _ = rc.capture(low, fmt, up_taps, 160, 147)
    assert high.shape == (1, low.shape[1] // 147 * 160)
    got, _eod = rx.demodulate(high[0])
    assert got == payload


def test_plan_arithmetic_under_sanitizers(tmp_path):
    exe = str(tmp_path / "ratecvt_plan_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "webaudio_modem_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "ratecvt_plan_check.cpp")],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
    # the GPU tests place their lengths one period past the plan's segment and tile: their arithmetic is the header's
    import test_gpu_ratecvt as tg
    r = subprocess.run([exe, "table"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    table = {tuple(int(v) for v in line.split()[:4]): tuple(int(v) for v in line.split()[4:]) for line in r.stdout.splitlines()}
    want = {(L, M, t, pb): (tg._seg_periods(True, bool(pb), L, M, t), tg._seg_periods(False, bool(pb), L, M, t))
            for L, M in tg.PAIRS for t in tg._tap_counts(L, M) for pb in (0, 1)}
    assert table == want and len(want) == 2 * sum(len(tg._tap_counts(L, M)) for L, M in tg.PAIRS)


def test_call_refusals_under_sanitizers(tmp_path):
    """what a process call of either unit is refused for behind the null handle (csrc/fsk_rate_call.h): every refusal in the
    header's order with all behind it wrong as well, for both units and directions (tests/cpp/rate_call_check.cpp)"""
    exe = str(tmp_path / "rate_call_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "webaudio_modem_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "rate_call_check.cpp")],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
