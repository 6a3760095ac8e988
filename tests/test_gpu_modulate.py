"""The modulator kernels (webaudio_modem_amd/csrc/fsk_mod.hip) on every path and edge, against the real reference's goldens
(tests/golden/golden_modulate.npz, oracle/refrun/golden_harness_modulate.js) and the CPU oracle, which
tests/test_oracle_modulate_edges.py holds to the same goldens.

launch_modulate picks modulate_kernel (one wave per 64 streams) below 32 samples per bit and modulate_wide_kernel (seven waves) from
32 on; each has an fp64 body (V8's sine restated: fsk_fdlibm.h) and an fp32 one (the device library's sin()).  All four run here at
5, 10, 20, 31 | 32, 33, 40, 64 and 147 samples per bit -- a bit boundary at a tile's first sample, at its last, or nowhere in it --,
in one and several workgroups, with a partly filled last wave, ragged payloads, every store path of store_tile and pitches that cut.

The bar.  fp64 engines: the reference's or the oracle's bits, compared as uint32.  fp32 engines: tests/test_gpu_parity.py's bar for
test_modulate_matches_reference_golden per signal -- |diff| <= 1.2e-7, at most max(1, n // 10000) differing samples -- and the
exactly-zero samples and the lengths identical.

Observed on an MI355X (largest number of differing samples of one fp32 signal, per family): goldens, alone and at streams 0 / 63 /
64 of 65: 0 in all 45; sweep against the oracle: 0 in all 36 (samples per bit, S) cells; per-stream tone pairs: 0; store paths and
cutting pitches: 0.
Long cases (fp64; samples of the tail that differ from the reference's): long_stated_spb10 0 of 18 549, long_stated_spb32 0 of
18 858 (inside the restated range: asserted); long_actual_spb10 0 of 26 339, long_actual_spb32 0 of 26 703 (observed identical).

Value-only mutants of fsk_mod.hip, each run once against this file: the wide kernel's bit boundary off by one fails the goldens,
the sweep and every other wide-kernel test at 33, 40 and 147 samples per bit (at 32 and 64 no tile holds a boundary); frame_bit's
parity inverted for odd parity fails the odd-parity goldens and the whole sweep; the chain wave's payload prefetch one byte late
fails every wide-kernel test with payloads of three bytes or more; store_tile writing dst[3] unconditionally fails the store-path
and the cutting-pitch tests, in both kernels.
"""
import numpy as np
import pytest

from hip_caller import Caller
from modulate_ref import (SPBS, RaggedRows, bits, check_signal, config, differing, golden_modulate, oracle_signal, ragged_payloads, sha256,
                          within_one_spacing)

pytestmark = pytest.mark.gpu

PRECISIONS = [("f64", 1), ("f32", 0)]
E_INVALID, E_NOT_CONFIGURED, E_OVERFLOW = -1, -2, -7


def _engine(cfg, prec, S=1):
    import webaudio_modem_amd as wm
    return wm.FSKEngine(S, cfg, device=0, precision=prec)


def _payload_args(payloads, pitch=None):
    lens = np.array([len(p) for p in payloads], np.uint32)
    pitch = max(1, int(lens.max())) if pitch is None else pitch
    pay = np.zeros((len(payloads), pitch), np.uint8)
    for s, p in enumerate(payloads):
        pay[s, :len(p)] = np.frombuffer(p, np.uint8)
    return pay, lens, pitch


# ---- 1. every new golden: alone, and as stream 0, 63 and 64 of a 65-stream batch ------------------------------------------------------

@pytest.mark.parametrize("pname,prec", PRECISIONS)
@pytest.mark.parametrize("mc", golden_modulate().short, ids=lambda m: m["name"])
def test_modulate_matches_the_reference_alone_and_in_a_batch(mc, pname, prec):
    ref, payload = golden_modulate().array(mc["signal"]), bytes(mc["payload"])
    eng = _engine(mc["config"], prec)
    sig = eng.modulate_data([payload])[0]
    eng.close()
    worst = check_signal(sig, ref, prec == 1, "alone")
    # the other streams: payloads of every length from 0 to 12, so that in the full wave the golden's lanes are neither the only longest
    # nor the only shortest (a 0-byte golden has other empty streams beside it); stream 64 is the one lane of the last wave
    S = 65
    payloads = [bytes((7 * s + k) & 0xFF for k in range((5 * s + 3) % 13)) for s in range(S)]
    assert {len(p) for p in payloads[1:63]} == set(range(13))
    for s in (0, 63, 64):
        payloads[s] = payload
    eng = _engine(mc["config"], prec, S)
    sigs = eng.modulate_data(payloads)
    eng.close()
    for s in (0, 63, 64):
        worst = max(worst, check_signal(sigs[s], ref, prec == 1, "stream %d of %d" % (s, S)))
    for s in (1, 62):    # ... and its neighbours are the oracle's
        check_signal(sigs[s], oracle_signal(mc["config"], payloads[s]), prec == 1, "stream %d of %d" % (s, S))
    print("observed[golden %s %s] %d differing of %d" % (pname, mc["name"], worst, ref.size))


# ---- 2. sweep against the oracle ---------------------------------------------------------------------------------------------------

def _max_len(spb):
    return 12 if spb <= 40 else (5 if spb == 64 else 3)        # (<= 12 bytes; fewer where a bit is long: the same edges in fewer samples)


@pytest.mark.parametrize("pname,prec", PRECISIONS)
@pytest.mark.parametrize("S", [1, 64, 65, 130])
@pytest.mark.parametrize("spb", SPBS)
def test_modulate_sweep_matches_the_oracle(spb, S, pname, prec):
    """Ragged payloads in one, one full, one full + one partly filled and three workgroups, for the three framings and for no preamble
    and no SFD: there a 0-length stream has no tones and no 2-bit padding (fsk.ts:392) beside streams that have both, so the wide
    kernel's uniform sig_begin must not leak into its lane."""
    worst = 0
    for fi, framing in enumerate(("8n1", "even_stop2", "odd_start2", "nopre")):
        cfg = config(spb, framing)
        sets = [ragged_payloads(S, _max_len(spb), 1000 * spb + 10 * S + fi)] if S > 1 else [[b""], [b"\x55"], [bytes(range(200, 200 + _max_len(spb)))]]
        eng = _engine(cfg, prec, S)
        for payloads in sets:
            lens = [len(p) for p in payloads]
            if S > 1:
                assert {0, 1, _max_len(spb)} <= set(lens) and lens[S - 1] == 0
            sigs = eng.modulate_data(payloads)
            for s in range(S):
                ref = oracle_signal(cfg, payloads[s])
                assert sigs[s].size == ref.size == eng.modulated_length(lens[s]), (framing, s)       # out_lens, the oracle, fskhip_modulated_length
                worst = max(worst, check_signal(sigs[s], ref, prec == 1, "%s stream %d" % (framing, s)))
        eng.close()
    print("observed[sweep %s spb %d S %d] %d differing in one signal" % (pname, spb, S, worst))


@pytest.mark.parametrize("pname,prec", PRECISIONS)
@pytest.mark.parametrize("spb", [20, 40])
def test_modulate_sweep_with_per_stream_tone_pairs(spb, pname, prec):
    S = 130
    hi = 2400 if spb == 20 else 1000
    cfgs = [config(spb, "8n1", tones=(hi + 37 * s, 2 * hi + 41 * s)) for s in range(S)]
    assert all(max(c["markFrequency"], c["spaceFrequency"]) < c["sampleRate"] / 2 for c in cfgs)
    payloads = ragged_payloads(S, 12, 77 + spb)
    eng = _engine(cfgs, prec, S)
    sigs = eng.modulate_data(payloads)
    worst = 0
    for s in range(S):
        ref = oracle_signal(cfgs[s], payloads[s])
        assert sigs[s].size == ref.size == eng.modulated_length(len(payloads[s]))
        worst = max(worst, check_signal(sigs[s], ref, prec == 1, "stream %d" % s))
    eng.close()
    print("observed[tones %s spb %d] %d differing in one signal" % (pname, spb, worst))


# ---- 3. / 4. the store paths, stray writes, pitches that cut -----------------------------------------------------------------------

class DeviceCall:
    """fskhip_modulate_device on the caller's own HIP stream: payloads and lens uploaded, out_lens read back"""

    def __init__(self, eng, payloads):
        self.eng, self.c, self.S = eng, Caller(eng), len(payloads)
        pay, lens, self.ppitch = _payload_args(payloads)
        self.d_pay, self.d_lens, self.d_out_lens = self.c.malloc(pay.nbytes), self.c.malloc(lens.nbytes), self.c.malloc(4 * self.S + 8)
        self.c.upload(self.d_pay, pay)
        self.c.upload(self.d_lens, lens)

    def run(self, rows):
        """-> out_lens; the word in front of it and the one behind it keep their sentinels"""
        self.c.upload(self.d_out_lens, np.full(self.S + 2, 0xDEADBEEF, np.uint32))
        self.eng.modulate_device(self.d_pay, self.d_lens, self.ppitch, rows.ptr, rows.pitch, self.d_out_lens + 4, stream=self.c.stream)
        self.c.sync()
        got = self.c.download(self.d_out_lens, np.empty(self.S + 2, np.uint32))
        assert got[0] == got[-1] == 0xDEADBEEF
        return got[1:-1]

    def close(self):
        self.c.close()


def _store_case(spb, S=65):
    """a configuration, ragged payloads and the oracle's signals, the longest of them off the 4-sample grid"""
    for framing, max_len in (("nopre", 12), ("nopre", 11), ("8n1", 12), ("8n1", 11)):
        cfg = config(spb, framing)
        payloads = ragged_payloads(S, max_len, 4242 + spb)
        refs = [oracle_signal(cfg, p) for p in payloads]
        if max(r.size for r in refs) % 4:
            return cfg, payloads, refs
    raise AssertionError("no signal length off the 4-sample grid at %d samples per bit" % spb)


@pytest.mark.parametrize("pname,prec", PRECISIONS)
@pytest.mark.parametrize("spb", [31, 33])
def test_modulate_device_store_paths_and_no_stray_writes(spb, pname, prec):
    """store_tile's paths -- single stores at a pitch off the 4-sample grid (the longest signal itself; pitch + 6), 16-byte stores
    at a multiple of 4 on an aligned base, single stores again with the base 4 bytes behind a 16-byte boundary -- with ragged rows:
    row s is the oracle's signal in columns < out_lens[s]; every other word keeps its sentinel."""
    cfg, payloads, refs = _store_case(spb)
    longest = max(r.size for r in refs)
    up4 = (longest + 3) // 4 * 4
    assert longest % 4 != 0 and (up4 + 6) % 4 != 0
    eng = _engine(cfg, prec, len(payloads))
    call, worst = DeviceCall(eng, payloads), 0
    for pitch, shift in ((longest, 0), (up4, 0), (up4, 4), (up4 + 6, 0)):
        rows = RaggedRows(call.c, call.S, pitch, shift)
        out_lens = call.run(rows)
        assert list(out_lens) == [r.size for r in refs], (pitch, shift)
        worst = max(worst, rows.check(refs, out_lens, prec == 1))
    print("observed[store %s spb %d] %d differing in one row" % (pname, spb, worst))
    call.close()
    eng.close()


@pytest.mark.parametrize("pname,prec", PRECISIONS)
@pytest.mark.parametrize("spb", [3, 33])
def test_modulate_pitch_that_cuts_signals(spb, pname, prec):
    """out_pitch below a signal's length: out_lens[s] is the full length, row s holds the first min(out_lens[s], out_pitch) samples and
    nothing else is written; fskhip_modulate_host returns FSKHIP_E_OVERFLOW naming the first such stream, with the same prefixes in
    `out` and the full lengths in `out_lens`.  (3 samples per bit: a stream with nothing to send is 30 samples, so that 31, 32 and 33
    cut some rows and not others; from 32 samples per bit on the shortest signal is 320 samples, and the pitch halfway between the
    shortest and the longest signal and longest - 1 do.)"""
    S = 65
    cfg = config(spb, "nopre")
    payloads = ragged_payloads(S, 12, 99 + spb)
    refs = [oracle_signal(cfg, p) for p in payloads]
    full = np.array([r.size for r in refs], np.uint32)
    longest = int(full.max())
    eng = _engine(cfg, prec, S)
    call, worst = DeviceCall(eng, payloads), 0
    pay, lens, ppitch = _payload_args(payloads)
    middle = (int(full.min()) + longest) // 2
    for pitch in (1, 31, 32, 33, middle, longest - 1):
        cut = np.flatnonzero(full > pitch)
        assert cut.size > 0
        if pitch >= middle or (spb == 3 and pitch > 1):
            assert cut.size < S, "some rows fit"
        rows = RaggedRows(call.c, S, pitch)
        out_lens = call.run(rows)
        assert np.array_equal(out_lens, full), pitch
        worst = max(worst, rows.check(refs, np.minimum(full, pitch), prec == 1))
        # the host call
        out = np.full((S, pitch), np.float32(7.0))
        h_lens = np.zeros(S, np.uint32)
        rc = eng._L.fskhip_modulate_host(eng._h, pay.ctypes.data, lens.ctypes.data, ppitch, out.ctypes.data, pitch, h_lens.ctypes.data)
        assert rc == E_OVERFLOW
        assert eng._L.fskhip_last_error().decode() == "stream %d needs %d samples, slab holds %d" % (cut[0], full[cut[0]], pitch)
        assert np.array_equal(h_lens, full)
        for s in range(S):
            n = min(int(full[s]), pitch)
            worst = max(worst, check_signal(out[s, :n], refs[s][:n], prec == 1, "host row %d at pitch %d" % (s, pitch)))
    print("observed[cut %s spb %d] %d differing in one row" % (pname, spb, worst))
    call.close()
    eng.close()


# ---- 5. no carried state --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pname,prec", PRECISIONS)
@pytest.mark.parametrize("spb", [10, 40])
def test_modulate_carries_no_state(spb, pname, prec):
    """the phase starts at 0 in every call: the same call twice, a call after other payloads and a call after a demodulate_data on
    the same engine all give the bits of a fresh engine"""
    S = 65
    cfg = config(spb, "8n1")
    payloads, other = ragged_payloads(S, 12, 5 + spb), ragged_payloads(S, 9, 6 + spb)[::-1]
    eng = _engine(cfg, prec, S)
    first = eng.modulate_data(payloads)
    again = eng.modulate_data(payloads)
    eng.modulate_data(other)
    after_other = eng.modulate_data(payloads)
    n = max(s.size for s in first)
    x = np.zeros((S, n + 64), np.float32)
    for s in range(S):
        x[s, 3:3 + first[s].size] = first[s]
    eng.demodulate_data(x)
    after_demod = eng.modulate_data(payloads)
    eng.close()
    fresh = _engine(cfg, prec, S)
    want = fresh.modulate_data(payloads)
    fresh.close()
    for s in range(S):
        check_signal(want[s], oracle_signal(cfg, payloads[s]), prec == 1, "stream %d" % s)
        for name, got in (("first", first), ("again", again), ("after other payloads", after_other), ("after demodulate_data", after_demod)):
            assert np.array_equal(bits(got[s]), bits(want[s])), (name, s)


# ---- 6. the long cases: across the end of the sine's medium range -----------------------------------------------------------------------

@pytest.mark.parametrize("lc", golden_modulate().long, ids=lambda m: m["name"])
def test_modulate_long_signal_across_the_sine_limit(lc):
    """fp64 engines, one case per kernel and limit.  Up to the crossing the signal is the reference's (SHA-256 of the prefix); behind it
    every sample is within one float32 spacing of the reference's.  The "stated" limit, 2^19 * pi/2, lies inside the range in which
    fsk_fdlibm.h restates V8's sine (high word <= 0x413921fb: 2^20 * pi/2), so those tails are identical by construction; behind the
    "actual" limit ref_sin takes the device library's sin(), and the count is what was observed."""
    g = golden_modulate()
    tail = g.array(lc["tail"])
    eng = _engine(lc["config"], 1)
    sig = eng.modulate_data([bytes(g.array(lc["payload"]))])[0]
    eng.close()
    assert sig.size == lc["n"]
    assert sha256(sig[:lc["cross"]]) == lc["prefix_sha256"]
    n_diff = differing(sig[lc["cross"]:], tail)
    print("observed[long %s] %d of %d tail samples differ from the reference's" % (lc["name"], n_diff, tail.size))
    assert within_one_spacing(sig[lc["cross"]:], tail)
    if lc["limit"] == "stated":
        assert n_diff == 0


# ---- 7. refusals that need an engine ------------------------------------------------------------------------------------------------------

def test_modulate_refusals():
    S = 3
    eng = _engine(config(10), 0, S)
    L, h = eng._L, eng._h
    pay, lens, out, out_lens = np.zeros((S, 4), np.uint8), np.array([1, 4, 2], np.uint32), np.full((S, 64), np.float32(7.0)), np.full(S, 9, np.uint32)
    P, LN, O, OL = pay.ctypes.data, lens.ctypes.data, out.ctypes.data, out_lens.ctypes.data

    def refused(rc, code, text):
        assert (rc, L.fskhip_last_error().decode()) == (code, text)

    for args in ((P, None, 4, O, 64, OL), (P, LN, 4, None, 64, OL), (P, LN, 4, O, 64, None)):
        refused(L.fskhip_modulate_host(h, *args), E_INVALID, "null buffer")
        refused(L.fskhip_modulate_device(h, *args, None), E_INVALID, "null buffer")
    refused(L.fskhip_modulate_host(None, P, LN, 4, O, 64, OL), E_NOT_CONFIGURED, "FSK modulator not configured")
    refused(L.fskhip_modulate_device(None, P, LN, 4, O, 64, OL, None), E_NOT_CONFIGURED, "FSK modulator not configured")
    lens[1] = 5
    refused(L.fskhip_modulate_host(h, P, LN, 4, O, 64, OL), E_INVALID, "lens[1] = 5 exceeds payload_pitch 4")
    assert (out == np.float32(7.0)).all() and (out_lens == 9).all()
    eng.close()
