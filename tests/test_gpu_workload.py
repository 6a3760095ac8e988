"""The two device-side generators every noisy test and every throughput number starts from, against their CPU model
(tests/workload_ref.py, itself checked in tests/test_workload_cpu.py):

  synth_kernel (fskhip_synth_device)               the exactly-zero samples are the model's (lead-in, padding, frame seams); every
      other sample is within one float32 spacing of the model's, and at most 2 samples of a case differ at all (device sine
      against the V8 sine);
  power_kernel + awgn_kernel (fskhip_add_awgn_device)   every sample within 0.5 float32 spacing + 1e-11 sigma_s of the model's
      float64 value: one rounding, plus the device's log / cos / sqrt / pow and the summation order of the power pass;

over ragged waves, per-stream tones, parity, every store path (pitch off and on the 4-sample grid, a base off the 16-byte grid),
sentinel columns and guard words around the buffer, the second launch slab of the noise kernel, and the refusals."""
import numpy as np
import pytest

import workload_ref as wr

pytestmark = pytest.mark.gpu

E_INVALID = -1
SENTINEL = np.uint32(0x7FC0BEEF)          # a NaN no kernel produces: compared as bits
GUARD = 64                                # sentinel words behind the last row (and the one word in front of a shifted base)
AWGN_SLACK = 1e-11                        # x sigma_s, on top of the half spacing of the one rounding
SNR_SEEDS = {-3.0: 0xA36, 10.0: 0xBEE, 40.0: 0x5EED}


def _wm():
    import webaudio_modem_amd as wm
    return wm


def _engine(cfgs, S):
    wm = _wm()
    return wm.FSKEngine(S, cfgs, device=0, precision=wm.PRECISION_F64)


class Rows:
    """a [S, pitch] float32 device buffer whose first element lies `shift` bytes behind a 16-byte boundary, inside an allocation
    of sentinels: one readback shows the rows and that nothing around them -- the columns from n on, the words before the first
    row and behind the last -- was written"""

    def __init__(self, eng, S, n, pitch, shift=0, rows=None):
        assert shift % 4 == 0 and pitch >= n
        self.eng, self.S, self.n, self.pitch, self.lead = eng, S, n, pitch, shift // 4
        self.words = self.lead + S * pitch + GUARD
        self.base = eng.device_malloc(self.words * 4)
        assert self.base % 16 == 0
        self.ptr = self.base + shift
        host = np.full(self.words, SENTINEL, np.uint32)
        if rows is not None:
            host[self.lead:self.lead + S * pitch].reshape(S, pitch)[:, :n] = np.ascontiguousarray(rows, np.float32).view(np.uint32)
        eng.h2d(self.base, host)
        self.sent = host

    def read(self):
        """[S, n] float32 (a copy), after checking every word outside it"""
        self.eng.synchronize()
        host = np.empty(self.words, np.uint32)
        self.eng.d2h(host, self.base)
        body = host[self.lead:self.lead + self.S * self.pitch].reshape(self.S, self.pitch)
        assert (host[:self.lead] == SENTINEL).all(), "written in front of the buffer"
        assert (host[self.lead + self.S * self.pitch:] == SENTINEL).all(), "written behind the last row"
        assert (body[:, self.n:] == SENTINEL).all(), "written in columns n .. pitch"
        return body[:, :self.n].copy().view(np.float32)

    def untouched(self):
        self.eng.synchronize()
        host = np.empty(self.words, np.uint32)
        self.eng.d2h(host, self.base)
        return np.array_equal(host, self.sent)

    def free(self):
        self.eng.device_free(self.base)


GEOMETRY = [("pitch-n", 0, 0), ("pitch-n+5", 5, 0), ("pitch-n+6", 6, 0), ("pitch-n+9-base+4B", 9, 4)]
# n = 6 007: pitch n and n + 6 are off the 4-sample grid (single stores); n + 5 = 6 012 is on it with an aligned base (16-byte stores,
# the cut last chunk single); n + 9 = 6 016 is on it with the base 4 bytes behind a 16-byte boundary (single stores again)


def _synth(c, pad=0, shift=0, S_engine=None, twice=False):
    """the case on the device: [S, n] float32"""
    S = S_engine or c["S"]
    cfgs = c["cfgs"] if S_engine is None or isinstance(c["cfgs"], dict) else None
    eng = _engine(cfgs, S)
    buf = Rows(eng, S, c["n"], c["n"] + pad, shift)
    try:
        eng.synth_device(buf.ptr, c["n"], buf.pitch, c["payload_len"], c["seed"], c["lead_max"], c["amp_lo"], c["amp_hi"])
        got = buf.read()
        if twice:
            eng.synth_device(buf.ptr, c["n"], buf.pitch, c["payload_len"], c["seed"], c["lead_max"], c["amp_lo"], c["amp_hi"])
            assert np.array_equal(buf.read().view(np.uint32), got.view(np.uint32)), "the same call twice differs"
    finally:
        buf.free()
        eng.close()
    return got


_MODEL = {}


def _model(name):
    if name not in _MODEL:
        _MODEL[name] = wr.synth(**wr.synth_cases()[name])
        _MODEL[name].setflags(write=False)
    return _MODEL[name]


def _check_synth(got, want, what):
    assert got.shape == want.shape
    assert np.array_equal(got == 0, want == 0), "%s: the exactly-zero samples are not the model's (first at %s)" % (
        what, np.argwhere((got == 0) != (want == 0))[:1].tolist())
    assert not got.view(np.uint32)[got == 0].any(), "%s: a zero that is not +0.0" % what
    d = got != want
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    print("%s: %d of %d samples differ from the model, largest %.3g float32 spacings" % (
        what, int(d.sum()), got.size, float((err[d] / np.spacing(np.abs(want[d])).astype(np.float64)).max()) if d.any() else 0.0))
    assert (err <= np.spacing(np.abs(want)).astype(np.float64)).all(), "%s: a sample more than one float32 spacing from the model (first at %s)" % (
        what, np.argwhere(err > np.spacing(np.abs(want)))[:1].tolist())
    assert d.sum() <= wr.MAX_DIFFERENT, "%s: %d samples differ from the model" % (what, int(d.sum()))


# ---- a. the synthesiser ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(wr.synth_cases()))
def test_synth_matches_the_model(name):
    """Observed on an MI355X: 0 samples of any case differ from the model, in any buffer geometry."""
    c = wr.synth_cases()[name]
    got = _synth(c)
    want = _model(name)
    if name == "lead-beyond-n":
        lead, _ = wr.stream_params(c["seed"], np.arange(c["S"]), c["lead_max"], c["amp_lo"], c["amp_hi"])
        assert 1 <= (lead >= c["n"]).sum() <= c["S"] // 2 and not want[lead >= c["n"]].any()        # some rows are all zero, most are not
    if name == "one-level":
        assert np.abs(want).max() == np.float32(0.5)
    _check_synth(got, want, name)


@pytest.mark.parametrize("geo,pad,shift", GEOMETRY)
@pytest.mark.parametrize("name", ["ragged-wave", "tone-pairs"])
def test_synth_store_paths_and_sentinels(name, geo, pad, shift):
    """every store path of the tile writer gives the model's rows and leaves columns n .. pitch and the words around the buffer alone"""
    _check_synth(_synth(wr.synth_cases()[name], pad, shift), _model(name), "%s, %s" % (name, geo))


def test_synth_is_reproducible_and_keyed_by_stream():
    """the same call twice is byte-equal; stream s of a 70-stream engine is stream s of a 1 000-stream engine"""
    c = wr.synth_cases()["ragged-wave"]
    small = _synth(c, twice=True)
    big = _synth(c, S_engine=1000)
    assert np.array_equal(big[:c["S"]].view(np.uint32), small.view(np.uint32))
    assert len({row.tobytes() for row in big}) == 1000          # ... and no two streams of the thousand are the same


# ---- b. the noise -----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def base():
    """the synthesised S = 70, n = 6 007 buffer, copied back from the device"""
    x = _synth(wr.synth_cases()["ragged-wave"])
    x.setflags(write=False)
    return x


def _awgn(x, snr_db, seed, pad=0, shift=0, S_engine=None, passes=1):
    """x [S, n] through fskhip_add_awgn_device on an engine of S_engine streams (default S): the rows after each pass"""
    S, n = x.shape
    Se = S_engine or S
    rows = x if Se == S else np.concatenate([x, np.full((Se - S, n), 0.125, np.float32)])
    eng = _engine(wr.BASE, Se)
    buf = Rows(eng, Se, n, n + pad, shift, rows)
    out = []
    try:
        for k in range(passes):
            eng.add_awgn_device(buf.ptr, n, buf.pitch, snr_db, seed + k)
            out.append(buf.read()[:S])
    finally:
        buf.free()
        eng.close()
    return out[0] if passes == 1 else out


def _check_awgn(got, x, snr_db, seed, what, first_stream=0):
    """every sample within half a float32 spacing of the model's float64 value, plus AWGN_SLACK sigma_s"""
    v, sigma = wr.awgn(x, snr_db, seed, first_stream)
    err = np.abs(got.astype(np.float64) - v)
    over = err - 0.5 * wr.spacing_f32(v)
    live = sigma > 0
    excess = float((over[live] / sigma[live, None]).max()) if live.any() else -np.inf
    print("%s: largest (error - half a float32 spacing) %.3g sigma (allowed %.0e); %d of %d samples are not the model's value rounded" % (
        what, excess, AWGN_SLACK, int((got != v.astype(np.float32)).sum()), got.size))
    bad = over > AWGN_SLACK * sigma[:, None]
    assert not bad.any(), "%s: %d samples off the model, first at %s: got %r, model %r, sigma %r" % (
        what, int(bad.sum()), np.argwhere(bad)[0].tolist(), got[tuple(np.argwhere(bad)[0])], v[tuple(np.argwhere(bad)[0])], sigma[np.argwhere(bad)[0][0]])
    quiet = ~np.asarray(x, np.float32).any(axis=1)
    assert (got[quiet].view(np.uint32) == 0).all(), "%s: a row of zeros did not stay +0.0" % what
    return sigma


@pytest.mark.parametrize("snr_db", sorted(SNR_SEEDS))
def test_awgn_matches_the_model(base, snr_db):
    """Observed on an MI355X, over every noise case of this file: no sample is further than half a float32 spacing from the model's
    float64 value -- the largest (error - half a spacing) is -7.1e-15 sigma_s, so none of the 1e-11 sigma_s allowance is used."""
    got = _awgn(base, snr_db, SNR_SEEDS[snr_db])
    sigma = _check_awgn(got, base, snr_db, SNR_SEEDS[snr_db], "%g dB" % snr_db)
    # (what the bound stands on: the noise is there, at the level asked for -- a sample 3 dB weak is ~0.3 sigma off)
    noise = got.astype(np.float64) - base
    ratio = np.mean(noise ** 2, axis=1) / sigma ** 2
    assert np.abs(ratio - 1).max() <= 5 * np.sqrt(2.0 / base.shape[1])


@pytest.mark.parametrize("geo,pad,shift", GEOMETRY[1:])
def test_awgn_pitches_and_sentinels(base, geo, pad, shift):
    _check_awgn(_awgn(base, 10.0, 0xA36, pad, shift), base, 10.0, 0xA36, geo)


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_awgn_grid_edge(base, n):
    """one 256-thread block short of, at, and one past a whole block; pitch n + 3 behind it holds the sentinel"""
    x = np.ascontiguousarray(base[:, 1000:1000 + n])
    assert x.any(axis=1).all()
    _check_awgn(_awgn(x, 10.0, 0xBEE, pad=3), x, 10.0, 0xBEE, "n = %d" % n)


def test_awgn_leaves_rows_of_zeros_alone():
    """a stream whose lead-in exceeds n, and a whole batch of zeros: +0.0 everywhere, at any SNR"""
    x = _synth(wr.synth_cases()["lead-beyond-n"])
    quiet = ~x.any(axis=1)
    assert 1 <= quiet.sum() <= x.shape[0] // 2
    got = _awgn(x, -3.0, 0xA36)
    assert (got[quiet].view(np.uint32) == 0).all()
    _check_awgn(got, x, -3.0, 0xA36, "rows of zeros among others")
    z = np.zeros((70, 257), np.float32)
    assert (_awgn(z, 10.0, 0xBEE).view(np.uint32) == 0).all()


def test_awgn_second_launch_slab():
    """streams 32 768 and up take the noise kernel's second launch: they carry their global stream index, not the slab's"""
    S, n = 32768 + 70, 40
    x = np.full((S, n), 0.25, np.float32)
    got = _awgn(x, 10.0, 0xA36)
    hi = slice(32760, 32838)
    _check_awgn(got[hi], x[hi], 10.0, 0xA36, "rows 32 760 .. 32 837", first_stream=32760)
    _check_awgn(got[:78], x[:78], 10.0, 0xA36, "rows 0 .. 77")
    for r in range(78):
        assert not np.array_equal(got[32760 + r], got[r]) and not np.array_equal(got[32768 + r % 70], got[r % 70]), r
    _check_awgn(got, x, 10.0, 0xA36, "the whole batch")


def test_awgn_is_keyed_by_seed_stream_and_sample_alone(base):
    """stream s gets the same noise in a 70-stream engine as in a 1 000-stream one; another seed gives other noise"""
    x = np.ascontiguousarray(base[:, 600:1601])
    small = _awgn(x, 10.0, 0xA36)
    big = _awgn(x, 10.0, 0xA36, S_engine=1000)
    assert np.array_equal(small.view(np.uint32), big.view(np.uint32))
    other = _awgn(x, 10.0, 0xA37)
    assert (other != small).mean() > 0.99


def test_awgn_twice_takes_the_noisy_power(base):
    """a second call sees the first call's noise as signal: its sigma comes from the already noisy row"""
    x = np.ascontiguousarray(base[:, :3001])
    first, second = _awgn(x, 10.0, 0xA36, passes=2)          # seeds 0xA36, then 0xA37
    s1 = _check_awgn(first, x, 10.0, 0xA36, "first pass")
    s2 = _check_awgn(second, first, 10.0, 0xA37, "second pass")
    live = s1 > 0
    assert live.any() and (s2[live] > s1[live] * 1.03).all()          # power (1 + 10^-1) x, less 5 standard errors of 3 001 samples


# ---- c. refusals and edges ----------------------------------------------------------------------------------------------------------

def test_zero_samples_is_a_successful_no_op():
    eng = _engine(wr.BASE, 70)
    buf = Rows(eng, 70, 0, 16)
    try:
        L, h = eng._L, eng._h
        for pitch in (0, 16):
            assert L.fskhip_synth_device(h, buf.ptr, 0, pitch, 2, wr.SEED, 400, 0.1, 1.0, None) == 0
            assert L.fskhip_add_awgn_device(h, buf.ptr, 0, pitch, 10.0, 0xA36, None) == 0
            assert buf.untouched()
    finally:
        buf.free()
        eng.close()


def test_bad_buffers_and_snr_are_refused():
    wm = _wm()
    eng = _engine(wr.BASE, 70)
    buf = Rows(eng, 70, 40, 48)
    try:
        for call in (lambda p, n, pitch: eng.synth_device(p, n, pitch, 2, wr.SEED, 400, 0.1, 1.0),
                     lambda p, n, pitch: eng.add_awgn_device(p, n, pitch, 10.0, 0xA36)):
            for p, n, pitch in ((buf.ptr, 40, 39), (buf.ptr, 1, 0), (None, 40, 48), (None, 0, 0)):
                with pytest.raises(wm.FskHipError) as e:
                    call(p, n, pitch)
                assert e.value.code == E_INVALID and "bad buffer" in str(e.value)
        for snr_db in (float("nan"), float("inf"), float("-inf")):
            with pytest.raises(wm.FskHipError) as e:
                eng.add_awgn_device(buf.ptr, 40, 48, snr_db, 0xA36)
            assert e.value.code == E_INVALID and "snr_db is not finite" in str(e.value)
        assert buf.untouched()
    finally:
        buf.free()
        eng.close()
