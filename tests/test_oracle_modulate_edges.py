"""The CPU oracle's modulator against the real reference where tests/golden/golden.npz does not reach (its 13 modulation cases have 40,
147 or 160 samples per bit): tests/golden/golden_modulate.npz, recorded by oracle/refrun/golden_harness_modulate.js -- 5 to 147
samples per bit crossed with the framings and payloads of 0, 1 and 7 bytes, and four long signals whose phase passes the end of the
medium range of fdlibm's sine.  The GPU tests (tests/test_gpu_modulate.py) compare the kernels with the oracle wherever there is no
golden, so this is what pins "compare with the oracle" there.

Long cases: oracle/v8_sin.h restates V8's sine for arguments whose high word is <= 0x413921fb -- 2^20 * pi/2 = 1 647 099.3 rad; fdlibm's
comment calls it "2^19*(pi/2)" -- and takes the C library's sin() beyond it.  The "stated" cases pass 2^19 * pi/2 = 823 549.7 rad by
3.5 %: still inside the range, so they are identical to the end.  The "actual" cases pass 2^20 * pi/2 by 2.5 %: identical up to the
crossing (digest), within one float32 spacing behind it.  Observed: 0 differing samples in all four tails."""
import numpy as np
import pytest

from modulate_ref import golden_modulate, differing, sha256, within_one_spacing
from oracle import pyoracle as po


@pytest.mark.parametrize("mc", golden_modulate().short, ids=lambda m: m["name"])
def test_oracle_modulate_matches_reference_at_every_samples_per_bit(mc):
    ref = golden_modulate().array(mc["signal"])
    sig = po.OracleCore(mc["config"]).modulate(bytes(mc["payload"]))
    assert sig.size == mc["n"] == ref.size
    assert np.array_equal(sig.view(np.uint32), ref.view(np.uint32))


def test_the_short_cases_cover_the_cross():
    """every samples-per-bit value meets every framing; every payload length lies on both sides of 32 samples per bit"""
    short = golden_modulate().short
    spbs, framings = {m["samplesPerBit"] for m in short}, {m["framing"] for m in short}
    assert spbs == {5, 10, 20, 31, 32, 33, 40, 64, 147} and framings == {"8n1", "even_stop2", "odd_start2", "nopre", "pre4"}
    assert {(m["samplesPerBit"], m["framing"]) for m in short} == {(a, b) for a in spbs for b in framings}
    for side in (lambda v: v < 32, lambda v: v >= 32):
        assert {len(m["payload"]) for m in short if side(m["samplesPerBit"])} == {0, 1, 7}
    for m in short:
        c = m["config"]
        assert c["sampleRate"] // c["baudRate"] == m["samplesPerBit"] and max(c["markFrequency"], c["spaceFrequency"]) < c["sampleRate"] / 2
        assert m["framing"] != "nopre" or len(m["payload"]) > 0
    assert {b for m in short for b in m["payload"]} >= {0x00, 0xFF, 0x55}


@pytest.mark.parametrize("lc", golden_modulate().long, ids=lambda m: m["name"])
def test_oracle_modulate_long_signal_across_the_sine_limit(lc):
    g = golden_modulate()
    tail = g.array(lc["tail"])
    assert 1.02 <= lc["final_phase_over_limit"] <= 1.05 and tail.size == lc["n"] - lc["cross"] <= 32768
    sig = po.OracleCore(lc["config"]).modulate(bytes(g.array(lc["payload"])))
    assert sig.size == lc["n"]
    assert sha256(sig[:lc["cross"]]) == lc["prefix_sha256"]
    n_diff = differing(sig[lc["cross"]:], tail)
    print("%s: %d of %d tail samples differ from the reference's" % (lc["name"], n_diff, tail.size))
    assert within_one_spacing(sig[lc["cross"]:], tail)
    if lc["limit"] == "stated":          # 2^19 * pi/2 is inside the restated range: identity is by construction
        assert n_diff == 0
