"""GPU parity tests (run with -m gpu on the MI355X box): the HIP engine, called through the C ABI
(libfskhip.so via ctypes), against
  (1) the golden vectors captured from the real reference (tests/golden/), and
  (2) the CPU oracle on identical seeded inputs.
Bytes, eod counts and the integer status fields must be identical; floating-point status
(silence threshold, AGC gain) within 1e-12 (fp64 path) / 1e-5 (fp32 path) relative, the
north_star's tolerance for intermediates."""
import numpy as np
import pytest

from conftest import golden, case_names, run_chunked, STATUS_EXACT_KEYS

pytestmark = pytest.mark.gpu

PRECISIONS = [("f64", 1, 1e-12), ("f32", 0, 1e-5)]

# fixtures whose configuration the demodulator refuses by design (none of the golden set: the
# fractional sync-ring capacities at 44.1 kHz / parity / 2 stop bits are emulated)
UNSUPPORTED = set()
# very fine chunking of a long buffer = thousands of launches; covered by the c128 twins
SLOW_F32_ONLY = {"d_default_Hello_c1"}


def _engine(cfg, precision, n=1):
    import webaudio_modem_amd as wm
    return wm.FSKEngine(n, cfg, device=0, precision=precision)


def _check_status(st, ref, tol, agc_gain):
    for k in STATUS_EXACT_KEYS:
        assert st[k] == ref[k], k
    assert st["silenceThreshold"] == pytest.approx(ref["silenceThreshold"], rel=tol)
    if agc_gain is not None:
        assert st["agcGain"] == pytest.approx(agc_gain, rel=max(tol, 1e-12) * 10)


# the fp32 path has three kernels for whole tiles: four waves per 64 streams with a block-batched back wave (round 3, the
# default wherever dsSPB is a multiple of 4), and the round-2 kernels with one and two waves per group, which stay for the
# other configurations and as the per-sample reference of the block path.  FSKHIP_SPLIT (mapped to fskhip_set_option's
# "kernel" by tests/conftest.py) pins one of them at engine creation.
# (round 4: the four-wave kernel cuts batches that would leave CUs idle into groups of 32 / 16 / 8 streams -- a one-stream
# golden runs on an 8-lane group by default; "f32-four-wave-64" pins whole-wave groups)
# "-resets": demod_blk_kernel_r, whose block path takes 'eod' resets itself (the default picks it only after a call whose
# tiles mostly left the fast path); "-redo": the same, every such block then put back and redone sample by sample
# (round 5: "f32-seven-wave": demod_blk6_kernel, the small-batch kernel -- loader | AGC | pre-filter | iq + discriminator on the idle
# lanes of a narrow group | post filter running ahead of the frame logic with rewind | frame logic; a one-stream golden runs it
# on an 8-lane group; "-64" pins whole-wave groups, whose six parts are cut differently)
GOLDEN_VARIANTS = PRECISIONS + [("f32-one-wave", 0, 1e-5), ("f32-four-wave", 0, 1e-5), ("f32-four-wave-64", 0, 1e-5),
                                ("f32-four-wave-resets", 0, 1e-5), ("f32-four-wave-redo", 0, 1e-5),
                                ("f32-seven-wave", 0, 1e-5), ("f32-seven-wave-64", 0, 1e-5),
                                ("f32-seven-wave-per-stream", 0, 1e-5), ("f32-four-wave-per-stream", 0, 1e-5)]
# (round 6: "-per-stream": the golden's stream as stream 0 of a TWO-stream engine whose other stream has another tone pair, so that the
# engine is not uniform and runs the kernels' per-stream instantiations -- demod_blk6_kernel<., ., false>, demod_blk_kernel<., false, .>)


@pytest.mark.parametrize("pname,prec,tol", GOLDEN_VARIANTS)
@pytest.mark.parametrize("name", case_names())
def test_demod_matches_reference_golden(name, pname, prec, tol, monkeypatch):
    import webaudio_modem_amd as wm
    if pname == "f32-one-wave":
        monkeypatch.setenv("FSKHIP_SPLIT", "0")
    elif pname == "f32-four-wave":
        monkeypatch.setenv("FSKHIP_SPLIT", "4")
    elif pname == "f32-four-wave-64":
        monkeypatch.setenv("FSKHIP_SPLIT", "4")
        monkeypatch.setenv("FSKHIP_BLK_LANES", "64")
    elif pname in ("f32-four-wave-resets", "f32-four-wave-redo"):
        monkeypatch.setenv("FSKHIP_SPLIT", "4")
        monkeypatch.setenv("FSKHIP_BLK_RESETS", "1" if pname.endswith("resets") else "2")
    elif pname in ("f32-seven-wave", "f32-seven-wave-64"):
        monkeypatch.setenv("FSKHIP_SPLIT", "6")
        if pname.endswith("64"):
            monkeypatch.setenv("FSKHIP_BLK_LANES", "64")
    elif pname == "f32":
        monkeypatch.setenv("FSKHIP_SPLIT", "1")
    g = golden()
    c = g.cases[name]
    if name in UNSUPPORTED:
        eng = _engine(c["config"], prec)  # modulate-only engine: creation succeeds ...
        assert not eng.demod_supported()
        with pytest.raises(wm.FskHipError) as ei:  # ... and demodulating fails loudly
            eng.demodulate_data(g.case_input(c).reshape(1, -1))
        assert ei.value.code == -3  # FSKHIP_E_UNSUPPORTED
        eng.close()
        return
    if name in SLOW_F32_ONLY and pname == "f64":
        pytest.skip("covered by the coarser chunkings")
    per_stream = pname.endswith("-per-stream")
    if per_stream:
        monkeypatch.setenv("FSKHIP_SPLIT", "6" if "seven" in pname else "4")
        merged = dict(wm.engine.DEFAULT_FSK_CONFIG, **c["config"])
        other = dict(c["config"], markFrequency=merged["markFrequency"] + 30, spaceFrequency=merged["spaceFrequency"] + 30)
        eng = wm.FSKEngine(2, [c["config"], other], device=0, precision=prec)
    else:
        eng = _engine(c["config"], prec)
    x = g.case_input(c)

    def call(chunk):
        if per_stream:
            out, eod = eng.demodulate_data(np.stack([chunk, np.zeros_like(chunk)]))
        else:
            out, eod = eng.demodulate_data(chunk.reshape(1, -1))
        return out[0], int(eod[0])

    out, eod, nonempty, n_calls = run_chunked(call, x, c["chunk"])
    assert list(out) == c["bytes"]
    assert eod == c["eod_total"]
    assert n_calls == c["calls"]["count"]
    assert nonempty == c["calls"]["nonempty"]
    _check_status(eng.get_status(0), c["status"], tol, c["agc_gain"])
    eng.close()


@pytest.mark.parametrize("pname,prec,tol", PRECISIONS)
@pytest.mark.parametrize("name", [c["name"] for c in golden().manifest["cases"] if "trace" in c])
def test_intermediates_match_reference(name, pname, prec, tol):
    """north_star: intermediate I/Q magnitudes within 1e-5 relative of the reference (fp32 path);
    the fp64 path reproduces them to 1e-12.  Plain relative error wherever the amplitude is above
    1e-4 of the stream's peak (80 dB down: below that the fp32 filters' own rounding noise, ~1e-7 of
    the peak, is no longer 1e-5 of the sample), relative to that floor below it.  The slicer bits of
    these fixtures must be identical."""
    g = golden()
    c = g.cases[name]
    x = g.case_input(c)
    ref_amp = g.array(c["trace"]["amp"])
    ref_post = g.array(c["trace"]["post_out"])
    ref_bit = g.array(c["trace"]["bit"])
    eng = _engine(c["config"], prec)
    eng.trace_enable(0, ref_amp.size + 8)      # (capacity in decimated samples; the pre-filter trace holds twice as many)
    eng.demodulate_data(x.reshape(1, -1))
    tr = eng.trace_read()
    assert tr["amp"].size == ref_amp.size
    floor = 1.0e-4 * ref_amp.max()
    rel = np.abs(tr["amp"] - ref_amp) / np.maximum(ref_amp, floor)
    assert rel.max() <= tol, rel.max()
    assert np.abs(tr["post_out"] - ref_post).max() <= (1e-9 if prec == 1 else 2e-5)
    assert np.array_equal(tr["bit"], ref_bit)
    # the pre-filter's Float32Array (fsk.ts:202), one value per input sample: the fp64 path stores the very
    # float the reference stores; the fp32 path within 1e-5 of the stream's peak
    ref_pre = g.array(c["trace"]["pre_out"]).astype(np.float64)
    assert tr["pre_out"].size == ref_pre.size == x.size
    if prec == 1:
        assert np.array_equal(tr["pre_out"].astype(np.float32).view(np.uint32), ref_pre.astype(np.float32).view(np.uint32))
    else:
        assert np.abs(tr["pre_out"] - ref_pre).max() <= 1e-5 * np.abs(ref_pre).max()
    eng.close()


def test_digital_silence_stays_exactly_silent_across_resets():
    """The reference's discriminator gives phase 0 for an exactly-zero I/Q pair (Math.atan2(0, 0), fsk.ts:251), so digital
    silence stays f = 0, bit = 0 through every 'eod' resetState().  The fp32 whole-tile arithmetic keeps its I/Q branch in a
    frame that is NOT reset, where that phase 0 is the frame's offset -- exact only if its branch-free atan2 returns
    exactly +-0 for (0, 0) (fsk_pipe.hip: atan2_amp_fma), which is a property of the device's v_rcp_f32 / v_sqrt_f32 on
    powers of two; this pins it.  Then a frame after 3000 samples of such silence must decode."""
    import webaudio_modem_amd as wm
    from oracle import pyoracle as po
    cfg = {}
    o = po.OracleCore(cfg)
    payload = bytes(range(40, 60))
    sig = o.modulate(payload)
    lead = 3000                                   # ten 'eod' resets (280 samples each) inside the silence
    x = np.concatenate([np.zeros(lead, np.float32), sig, np.zeros(600, np.float32)]).astype(np.float32)
    eng = wm.FSKEngine(64, cfg, precision=wm.PRECISION_F32)
    eng.trace_enable(5, len(x))
    out, eod = eng.demodulate_data(np.tile(x, (64, 1)))
    assert "tail" in eng.last_kernel()            # a traced engine: fsk_pipe.hip's arithmetic, sample by sample
    tr = eng.trace_read()
    k = lead // 2
    assert int(eod[5]) >= 10
    assert np.all(tr["amp"][:k] == 0.0) and np.all(tr["post_out"][:k] == 0.0) and not tr["bit"][:k].any()
    ob, oe = o.demodulate(x)
    assert out[5] == ob == payload and int(eod[5]) == oe
    eng.close()


@pytest.mark.parametrize("pname,prec,tol", PRECISIONS)
def test_reconfigure_keeps_silence_threshold_and_debug_counters(pname, prec, tol):
    """configure() on a configured FSKCore (fsk.ts:133-157) rebuilds AGC / filters / rings and calls resetState(), which
    leaves silence.threshold (set at the last sync, fsk.ts:321-326) and the debug counters alone -- so the first 'eod' of
    the next burst is still judged against the OLD threshold.  The host classes re-configure with fskhip_create +
    fskhip_carry_over + fskhip_destroy; bytes, per-call eod counts and status must follow the oracle through it."""
    import webaudio_modem_amd as wm
    from oracle import pyoracle as po
    cfg_a = dict(baudRate=1200, markFrequency=1200, spaceFrequency=2200)
    cfg_b = dict(baudRate=1200, markFrequency=1650, spaceFrequency=1850)
    o = po.OracleCore(cfg_a)
    core = wm.FSKCore(precision=prec)
    core.configure(cfg_a)
    eods = []
    core.on("eod", lambda *_a: eods.append(1))
    burst_a = np.concatenate([o.modulate(b"first life") * np.float32(0.8), np.zeros(700, np.float32)])
    got = core.demodulateData(burst_a.copy())
    want, oe = o.demodulate(burst_a.copy())
    assert bytes(got) == want == b"first life" and len(eods) == oe
    thr_a = o.status()["silenceThreshold"]
    assert thr_a > 0.02                                   # the sync has replaced the initial 0.01
    core.configure(cfg_b)
    o.configure(cfg_b)
    st, ost = core.getStatus(), o.status()
    assert abs(st["silenceThreshold"] - thr_a) <= tol * thr_a and ost["silenceThreshold"] == thr_a
    assert st["syncDetections"] == ost["syncDetections"] == 1 and st["agcGain"] == 1.0
    # a weak second burst: its tail crosses the OLD threshold earlier than it would cross 0.01
    burst_b = np.concatenate([np.zeros(300, np.float32), o.modulate(b"second life") * np.float32(0.05), np.zeros(900, np.float32)])
    for lo in range(0, len(burst_b), 128):
        del eods[:]
        chunk = burst_b[lo:lo + 128]
        got = core.demodulateData(chunk.copy())
        want, oe = o.demodulate(chunk.copy())
        assert bytes(got) == want and len(eods) == oe, lo
    st, ost = core.getStatus(), o.status()
    for k in STATUS_EXACT_KEYS:
        assert st[k] == ost[k], k
    core.close() if hasattr(core, "close") else None


@pytest.mark.parametrize("pname,prec,tol", PRECISIONS)
def test_offset_sweep_batched(pname, prec, tol):
    """fsk-demodulation.node.test.ts:668-716 -- all 128 chunk offsets, here as 128 streams of ONE
    engine call sequence (stream k = k leading zeros + the frame), 128-sample chunks."""
    g = golden()
    sw = g.manifest["offset_sweep"]
    base = g.array(sw["base"])
    S = len(sw["runs"])
    N = base.size + 128
    N = (N + 127) // 128 * 128
    x = np.zeros((S, N), np.float32)
    for k in range(S):
        x[k, k:k + base.size] = base
    eng = _engine(sw["config"], prec, S)
    got = [b""] * S
    for off in range(0, N, 128):
        out, _ = eng.demodulate_data(x[:, off:off + 128])
        for s in range(S):
            got[s] += out[s]
    for k in range(S):
        assert list(got[k]) == sw["payload"], k
        assert list(got[k]) == sw["runs"][k]["bytes"], k
        assert eng.get_status(k)["syncDetections"] == sw["runs"][k]["status"]["syncDetections"]
    eng.close()


@pytest.mark.parametrize("pname,prec,tol", PRECISIONS)
@pytest.mark.parametrize("mc", golden().manifest["modulate"], ids=lambda m: m["name"])
def test_modulate_matches_reference_golden(mc, pname, prec, tol):
    """modulateData: identical length.  fp64 engines evaluate Math.sin with the operation sequence V8 uses
    (fsk_fdlibm.h): the Float32Array is bit-identical.  fp32 engines use the device library's sin(): identical except
    where its last double ulp differs from V8's AND that flips the float rounding -- at most 1 f32 ulp on at most
    0.01 % of the samples."""
    g = golden()
    eng = _engine(mc["config"], prec)
    sig = eng.modulate_data([bytes(mc["payload"])])[0]
    ref = g.array(mc["signal"])
    assert sig.size == mc["n"] == ref.size
    if pname == "f64":
        assert np.array_equal(sig.view(np.uint32), ref.view(np.uint32))
    elif sig.size:
        diff = np.abs(sig.astype(np.float64) - ref.astype(np.float64))
        assert diff.max() <= 1.2e-7
        assert np.count_nonzero(diff) <= max(1, sig.size // 10000)
    eng.close()


def test_modulate_batch_ragged_lengths():
    """Streams with different payload lengths in one call; each equals the 1-stream result."""
    from oracle import pyoracle as po
    payloads = [b"", b"A", b"Hello", bytes(range(64)), b"\x00\xff" * 10]
    eng = _engine({}, 1, len(payloads))
    sigs = eng.modulate_data(payloads)
    for p, s in zip(payloads, sigs):
        ref = po.OracleCore({}).modulate(p)
        assert s.size == ref.size
        assert np.array_equal(s, ref)
    eng.close()


def test_modulate_long_signals_bit_identical_to_oracle():
    """Phases in the tens of thousands of radians (1 000-byte payloads, 48 streams with their own tones): the GPU
    modulator and the oracle, both restating V8's Math.sin, agree on every bit of 20 million samples."""
    from oracle import pyoracle as po
    S = 48
    cfgs = [dict(baudRate=1200, markFrequency=1000 + 37 * s, spaceFrequency=1900 + 41 * s) for s in range(S)]
    rng = np.random.default_rng(0x51)
    payloads = [bytes(rng.integers(0, 256, 1000, dtype=np.uint8)) for _ in range(S)]
    eng = _engine(cfgs, 1, S)
    sigs = eng.modulate_data(payloads)
    for s in range(S):
        ref = po.OracleCore(cfgs[s]).modulate(payloads[s])
        assert sigs[s].size == ref.size > 400000
        assert np.array_equal(sigs[s].view(np.uint32), ref.view(np.uint32)), s
    eng.close()


@pytest.mark.parametrize("pname,prec,tol", PRECISIONS)
def test_per_stream_frequencies_vs_oracle(pname, prec, tol):
    """BASELINE config #4: per-stream mark/space (mark_s = 1000+10*(s mod 100), space = mark+200),
    300 baud.  GPU modulates each stream with its own tones, then demodulates; bytes, eod and
    status compared with the CPU oracle fed the SAME float32 buffers."""
    from oracle import pyoracle as po
    S = 70
    cfgs = [dict(baudRate=300, markFrequency=1000 + 10 * (s % 100), spaceFrequency=1200 + 10 * (s % 100)) for s in range(S)]
    rng = np.random.default_rng(0xC4)
    payloads = [bytes(rng.integers(0, 256, 6, dtype=np.uint8)) for _ in range(S)]
    eng = _engine(cfgs, prec, S)
    sigs = eng.modulate_data(payloads)
    N = max(s.size for s in sigs) + 300
    x = np.zeros((S, N), np.float32)
    for s in range(S):
        x[s, 37 * (s % 5):37 * (s % 5) + sigs[s].size] = sigs[s] * np.float32(0.2 + 0.01 * s)
    out, eod = eng.demodulate_data(x)
    for s in range(S):
        o = po.OracleCore(cfgs[s])
        ob, oe = o.demodulate(x[s])
        assert out[s] == ob, s
        assert out[s] == payloads[s], s
        assert int(eod[s]) == oe, s
        _check_status(eng.get_status(s), o.status(), tol, o.status()["agcGain"])
    eng.close()


@pytest.mark.parametrize("pname,prec,tol", PRECISIONS)
def test_awgn_roundtrip_vs_oracle(pname, prec, tol):
    """BASELINE config #5 shape at test size: GPU synth -> GPU AWGN (10 dB) -> GPU demod; the noisy
    buffers are copied back and the oracle must produce the same bytes per stream."""
    from oracle import pyoracle as po
    cfg = dict(baudRate=1200, markFrequency=1200, spaceFrequency=2200)
    S, N, P = 192, 48000, 40
    eng = _engine(cfg, prec, S)
    pitch = N
    d_x = eng.device_malloc(S * pitch * 4)
    eng.synth_device(d_x, N, pitch, P, 0xF5C0DE, 400, 0.1, 1.0)
    eng.add_awgn_device(d_x, N, pitch, 10.0, 0xA36)
    eng.synchronize()
    x = np.empty((S, pitch), np.float32)
    eng.d2h(x, d_x)
    eng.device_free(d_x)
    out, eod = eng.demodulate_data(x)
    n_frames_ok = 0
    for s in range(S):
        o = po.OracleCore(cfg)
        ob, oe = o.demodulate(x[s])
        assert out[s] == ob, "stream %d: GPU and oracle disagree" % s
        assert int(eod[s]) == oe
        if eng.synth_payload(0xF5C0DE, s, 0, P) in out[s]:
            n_frames_ok += 1
    assert n_frames_ok >= S * 0.5  # sanity only: at 10 dB the reference itself loses frames
    eng.close()


@pytest.mark.parametrize("pname,prec,tol", PRECISIONS)
def test_ragged_stream_count_and_odd_lengths(pname, prec, tol):
    """S not a multiple of 64, N not a multiple of the 32-sample tile nor of 4, odd chunk lengths
    (the /2 decimator straddles calls)."""
    from oracle import pyoracle as po
    g = golden()
    base = g.array("d_default_Hello_c128.in")
    S = 67
    x = np.zeros((S, base.size + 200), np.float32)
    for s in range(S):
        x[s, s:s + base.size] = base * np.float32(1.0 / (1 + s % 7))
    eng = _engine({}, prec, S)
    oracles = [po.OracleCore({}) for _ in range(S)]
    got = [b""] * S
    want = [b""] * S
    off = 0
    for n in [1, 3, 129, 31, 1000, 7, 513, 64, 2, 10 ** 9]:
        n = min(n, x.shape[1] - off)
        if n <= 0:
            break
        out, eod = eng.demodulate_data(x[:, off:off + n])
        for s in range(S):
            ob, oe = oracles[s].demodulate(x[s, off:off + n])
            got[s] += out[s]
            want[s] += ob
            assert int(eod[s]) == oe
        off += n
    for s in range(S):
        assert got[s] == want[s] == b"Hello", s
        _check_status(eng.get_status(s), oracles[s].status(), tol, oracles[s].status()["agcGain"])
    eng.close()


@pytest.mark.parametrize("baud", [600, 400, 240], ids=["dsSPB_40", "dsSPB_60", "dsSPB_100"])
def test_other_bit_cells_through_the_block_kernel(baud, monkeypatch):
    """The block kernel takes dsSPB = multiples of 4 whose sync-ring capacity -- (bits + 32) * dsSPB * 1.1 evaluated in
    doubles, fsk.ts:145,149 -- is an integer: 20 (the goldens' 1200 baud), 40, 80 (300 baud) with the default 24 pattern
    bits; 60 and 100 give 3696.0000000000005 and 6160.000000000001, fractional rings, the generic kernel.  Here 40 (other
    polyphase stride in LDS, register wraps at other blocks) and the two fractional ones for the routing: 130 streams
    with different payloads, lead-ins and levels, a ragged call schedule, against the oracle; FSKHIP_SPLIT=1 on the same
    buffers as a cross-check."""
    import webaudio_modem_amd as wm
    from oracle import pyoracle as po
    cfg = dict(baudRate=baud, markFrequency=2 * baud, spaceFrequency=3 * baud)
    S = 130
    rng = np.random.RandomState(baud)
    sigs = []
    for s in range(S):
        o = po.OracleCore(cfg)
        parts = [np.zeros(rng.randint(0, 300), np.float32)]
        for _ in range(3):
            parts += [o.modulate(bytes(rng.randint(0, 256, rng.randint(1, 9)).astype(np.uint8))) * np.float32(rng.uniform(0.1, 1.0)),
                      np.zeros(rng.randint(50, 2500), np.float32)]
        sigs.append(np.concatenate(parts))
    N = max(len(x) for x in sigs)
    x = np.zeros((S, N), np.float32)
    for s in range(S):
        x[s, :len(sigs[s])] = sigs[s]
    x[S // 2:] += (rng.standard_normal((S - S // 2, N)) * 0.02).astype(np.float32)      # half of them over a noise floor
    want, want_eod = [], []
    for s in range(S):
        b, e = po.OracleCore(cfg).demodulate(x[s])
        want.append(b)
        want_eod.append(e)
    assert sum(len(w) for w in want) > 2 * S      # (the reference itself drops frames that follow a gap too closely)
    for split in ("4", "1"):
        monkeypatch.setenv("FSKHIP_SPLIT", split)
        eng = wm.FSKEngine(S, cfg, precision=wm.PRECISION_F32)
        monkeypatch.delenv("FSKHIP_SPLIT")
        got = [b""] * S
        eods = np.zeros(S, np.int64)
        off = 0
        for n in [4096, 16, 1000, 48, 3, 8000, 129, 10 ** 9]:
            n = min(n, N - off)
            if n <= 0:
                break
            out, eod = eng.demodulate_data(x[:, off:off + n])
            for s in range(S):
                got[s] += out[s]
            eods += eod
            off += n
        if split == "4":
            d = 48000 // 2 // baud
            whole_tiles = ((24 + 32) * d * 1.1).is_integer()      # fsk.ts:145,149 in doubles: 2464.0 but 3696.0000000000005
            assert eng.last_kernel().startswith(("fsk::demod_blk_kernel", "fsk::demod_tail_kernel") if whole_tiles else "fsk::demod_kernel<float"), eng.last_kernel()
        eng.close()
        for s in range(S):
            assert got[s] == want[s], (split, s)
            assert int(eods[s]) == want_eod[s], (split, s)


def test_single_stream_reset_desynchronises_decimator():
    """reset(stream) at an odd sample count leaves that stream's /2 decimator out of phase with its
    neighbours (per-lane decimation path of the kernel)."""
    from oracle import pyoracle as po
    g = golden()
    base = g.array("d_default_AB.in")
    S = 5
    eng = _engine({}, 1, S)
    oracles = [po.OracleCore({}) for _ in range(S)]
    x = np.tile(base, (S, 1))
    eng.demodulate_data(x[:, :333])
    for o in oracles:
        o.demodulate(base[:333])
    eng.reset(2)
    oracles[2].reset()
    out, eod = eng.demodulate_data(np.ascontiguousarray(x[:, 333:]))
    out2, _ = eng.demodulate_data(x)
    for s in range(S):
        ob, oe = oracles[s].demodulate(base[333:])
        ob2, _ = oracles[s].demodulate(base)
        assert out[s] == ob and out2[s] == ob2, s
        assert int(eod[s]) == oe
        st, ost = eng.get_status(s), oracles[s].status()
        for k in STATUS_EXACT_KEYS:
            assert st[k] == ost[k], (s, k)
    eng.close()


def test_agc_writeback_matches_reference_mutation():
    """The reference mutates its input (AGC in place, fsk.ts:55); the golden 'agc_out' trace is
    that mutated buffer."""
    g = golden()
    c = g.cases["d_default_AB"]
    x = g.case_input(c).copy().reshape(1, -1)
    eng = _engine(c["config"], 1)
    eng.demodulate_data(x, writeback_agc=True)
    assert np.array_equal(x[0], g.array(c["trace"]["agc_out"]))
    x32 = g.case_input(c).copy().reshape(1, -1)
    eng32 = _engine(c["config"], 0)
    eng32.demodulate_data(x32, writeback_agc=True)
    ref = g.array(c["trace"]["agc_out"])
    assert np.max(np.abs(x32[0] - ref)) <= 1e-5 * np.max(np.abs(ref))
    eng.close()
    eng32.close()


def test_fskcore_mirror_events_and_errors():
    """FSKCore host class: 'configured' / 'eod' events, not-configured errors, reset semantics
    (tests/modems/fsk-demodulation.node.test.ts:31-36, 1133-1161; fsk-sfd 139-159)."""
    import webaudio_modem_amd as wm
    g = golden()
    core = wm.FSKCore()
    with pytest.raises(RuntimeError, match="not configured"):
        core.demodulateData(np.zeros(3, np.float32))
    with pytest.raises(RuntimeError, match="not configured"):
        core.modulateData(b"x")
    events = []
    core.on("configured", lambda e: events.append("configured"))
    core.on("eod", lambda e: events.append("eod"))
    core.configure({})
    assert core.isReady() and events == ["configured"]
    c = g.cases["d_two_frames"]
    out = core.demodulateData(g.case_input(c).copy())
    assert list(out) == c["bytes"]
    assert events.count("eod") == c["eod_total"] == 2
    core.reset()
    assert core.isReady()  # fsk.ts:464-469 keeps ready
    st = core.getStatus()
    assert st["syncDetections"] == 0 and st["demodulationCalls"] == 0 and st["receivedBitsLength"] == 0
    sig = core.modulateData(b"AB")
    assert sig.size == 2480
    assert list(core.demodulateData(sig)) == [65, 66]
    core.close()


def test_errors_are_loud():
    import webaudio_modem_amd as wm
    with pytest.raises(wm.FskHipError):
        wm.FSKEngine(4, [dict(baudRate=300), dict(baudRate=1200), {}, {}])  # per-stream baud not supported
    with pytest.raises(wm.FskHipError):
        wm.FSKEngine(1, dict(preamblePattern=[0x55] * 7)).demodulate_data(np.zeros((1, 8), np.float32))  # 80 pattern bits > 63
    # ring capacity 65*19*1.1 = 1358.5: the reference's fractional ring index becomes integral again
    # after two wraps -- a regime the engine refuses instead of approximating
    half = wm.FSKEngine(1, dict(parity="even", baudRate=1250))
    assert not half.demod_supported()
    assert half.modulate_data([b"ok"])[0].size == half.modulated_length(2)  # the modulator still works
    with pytest.raises(wm.FskHipError) as ei:
        half.demodulate_data(np.zeros((1, 8), np.float32))
    assert ei.value.code == -3
    half.close()
    eng = wm.FSKEngine(2, {})
    with pytest.raises(ValueError):
        eng.demodulate_data(np.zeros((3, 16), np.float32))
    eng.close()


def test_narrow_groups_leave_every_stream_exactly_as_whole_waves_do():
    """Round 4: batches too small to give every CU a 64-stream group run the four-wave kernel in groups of 32 / 16 / 8
    streams (fskhip_blk_lanes; fsk_blk.hip, launch_demod_blk).  The state arrays are indexed by stream and the polyphase
    registers blocked by 64, so group width must not show anywhere -- and neither must which of the two four-wave kernels ran
    (blk_resets: the block path that takes 'eod' resets, fsk_blk.hip's blk_medium): 150 streams (a ragged last group at every width) with
    their own payloads, lead-ins, levels and noise, a ragged call schedule with AGC write-back, per width -- bytes and eod
    against the oracle, and the written-back samples, every status field and the internal state words identical to the
    whole-wave run's."""
    import webaudio_modem_amd as wm
    from oracle import pyoracle as po
    cfg = dict(baudRate=1200, markFrequency=1200, spaceFrequency=2200)
    S = 150
    rng = np.random.RandomState(404)
    sigs = []
    for s in range(S):
        o = po.OracleCore(cfg)
        parts = [np.zeros(rng.randint(0, 300), np.float32)]
        for _ in range(3):
            parts += [o.modulate(bytes(rng.randint(0, 256, rng.randint(1, 9)).astype(np.uint8))) * np.float32(rng.uniform(0.1, 1.0)),
                      np.zeros(rng.randint(50, 2500), np.float32)]
        sigs.append(np.concatenate(parts))
    N = max(len(x) for x in sigs)
    x = np.zeros((S, N), np.float32)
    for s in range(S):
        x[s, :len(sigs[s])] = sigs[s]
    x[S // 2:] += (rng.standard_normal((S - S // 2, N)) * 0.02).astype(np.float32)
    want, want_eod = [], []
    for s in range(S):
        b, e = po.OracleCore(cfg).demodulate(x[s])
        want.append(b)
        want_eod.append(e)
    assert sum(len(w) for w in want) > 2 * S
    ref = None
    for lanes, resets in ((64, 0), (32, 0), (16, 1), (8, 0), ("auto", "auto"), (64, 1), (32, 2)):
        eng = wm.FSKEngine(S, cfg, precision=wm.PRECISION_F32, options={"kernel": "four-wave", "blk_lanes": lanes, "blk_resets": resets})
        assert eng.blk_lanes() == (8 if lanes == "auto" else lanes)       # (150 streams: 19 groups of 8 on any device)
        got = [b""] * S
        eods = np.zeros(S, np.int64)
        wb = []
        off = 0
        for n in [4096, 16, 1000, 48, 3, 8000, 129, 10 ** 9]:
            n = min(n, N - off)
            if n <= 0:
                break
            buf = np.ascontiguousarray(x[:, off:off + n])
            out, eod = eng.demodulate_data(buf, writeback_agc=True)
            wb.append(buf)
            for s in range(S):
                got[s] += out[s]
            eods += eod
            off += n
        assert "demod_blk_kernel" in eng.last_kernel() or "tail" in eng.last_kernel(), eng.last_kernel()
        state = [eng.debug_state(s) for s in (0, 7, 8, 63, 64, 71, 127, 128, 143, 144, 149)]
        status = [eng.get_status(s) for s in range(S)]
        eng.close()
        for s in range(S):
            assert got[s] == want[s], (lanes, resets, s)
            assert int(eods[s]) == want_eod[s], (lanes, resets, s)
        if ref is None:
            ref = (wb, state, status)
        else:
            for a, b in zip(ref[0], wb):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), lanes
            for a, b in zip(ref[1], state):
                assert np.array_equal(np.asarray(a[0]).view(np.uint64), np.asarray(b[0]).view(np.uint64)) and np.array_equal(a[1], b[1]), lanes
            assert ref[2] == status, lanes


def test_options_are_validated_and_none_changes_a_result():
    """fskhip_set_option (round 4: it replaces the library's environment switches): unknown names, values that are not
    numbers or out of range, a y-ring depth whose LDS does not fit, and options set after the engine has demodulated are
    FSKHIP_E_INVALID; valid ones choose a kernel / launch shape and leave the bytes alone."""
    import webaudio_modem_amd as wm
    from oracle import pyoracle as po
    bell = dict(baudRate=1200, markFrequency=1200, spaceFrequency=2200)
    for bad in ({"kernel": "fastest"}, {"blk_y_slots": "abc"}, {"blk_y_slots": 4}, {"blk_y_slots": 30}, {"blk_resident": 0},
                {"blk_lanes": 12}, {"blk_lanes": 4}, {"blk_lanes": "wide"}, {"blk_resets": 3}, {"blk_resets": "yes"},
                {"slice_tiles": "-3"}, {"force_generic": 2}, {"no_such_option": 1}, {"host_slab": "1e9"}):
        with pytest.raises(wm.FskHipError) as ei:
            wm.FSKEngine(64, bell, options=bad)
        assert ei.value.code == -1, bad
    o = po.OracleCore(bell)
    sig = np.concatenate([np.zeros(37, np.float32), o.modulate(b"options"), np.zeros(900, np.float32)])
    want, _ = po.OracleCore(bell).demodulate(sig)
    x = np.tile(sig, (130, 1))
    seen = set()
    for opts in ({}, {"kernel": "two-wave"}, {"kernel": "one-wave"}, {"kernel": "four-wave", "blk_y_slots": 7},
                 {"blk_resident": 2, "slice_tiles": 3}, {"force_generic": 1}, {"kernel": "auto-r02"}, {"slice_tiles": "off"},
                 {"blk_lanes": 16}, {"blk_lanes": "auto"}, {"blk_lanes": 64, "blk_y_slots": 9}, {"blk_resets": 1}, {"blk_resets": 0},
                 {"blk_resets": "auto"}, {"blk_resets": 2, "blk_lanes": 32}):
        eng = wm.FSKEngine(130, bell, options=opts)
        out, eod = eng.demodulate_data(x.copy())
        assert all(b == want for b in out), opts
        seen.add(eng.last_kernel().split("<")[0])
        with pytest.raises(wm.FskHipError):      # too late now
            eng.set_option("kernel", "auto")
        eng.close()
    assert {"fsk::demod_blk_kernel", "fsk::demod_pipe_kernel", "fsk::demod_fused_kernel"} <= seen, seen


@pytest.mark.parametrize("pname,prec,tol", PRECISIONS)
def test_single_stream_reset_at_odd_decimator_phase(pname, prec, tol):
    """Regression (tools/soak.py): a one-stream engine reset while its /2 decimator is mid-pair.  The device restarts the
    decimator; the host's notion of the phase has to follow, or a later odd-length call flips it the wrong way and the
    whole-tile kernels are handed a stream that is mid-pair."""
    from oracle import pyoracle as po
    g = golden()
    base = g.array("d_default_Hello_c128.in")
    x = np.concatenate([np.zeros(700, np.float32), base, np.zeros(300, np.float32)])
    eng = _engine({}, prec)
    o = po.OracleCore({})
    got = want = b""
    off = 0
    for step in (129, 128, "reset", 128, 129, 1000, 10 ** 9):
        if step == "reset":
            eng.reset(0)
            o.reset()
            continue
        n = min(step, x.size - off)
        out, eod = eng.demodulate_data(x[off:off + n].reshape(1, -1).copy())
        ob, oe = o.demodulate(x[off:off + n])
        got += out[0]
        want += ob
        assert int(eod[0]) == oe
        off += n
    assert got == want == b"Hello"
    _check_status(eng.get_status(0), o.status(), tol, o.status()["agcGain"])
    eng.close()


@pytest.mark.parametrize("after_reset", [5, 32, 60], ids=["direct_instance", "unretired_correction", "steady"])
def test_pipe_state_handed_to_generic_kernel_mid_pair(after_reset):
    """fskhip_reset(stream) on a multi-stream fp32 engine whose /2 decimators are mid-pair takes the
    batch out of lock step, so the NEXT call runs on the generic kernel -- which has to rebuild the reference's own state
    from the free-running representation with an open decimator pair.  While a stream is within kDirectPairs decimated
    samples of an internal resetState() the direct instance has not seen the pair's first sample yet, and a live ZIR
    correction sits one sample further along: both used to be ignored.  Stream 0 / 2: a frame, digital silence until the
    reference's 'eod', then a second frame right behind it, in light noise; the call is cut `after_reset` decimated samples
    and one input sample after that 'eod'."""
    from oracle import pyoracle as po
    rng = np.random.default_rng(77)
    o0 = po.OracleCore({})
    f1, f2 = o0.modulate(b"AB"), o0.modulate(b"Hello, generic kernel")
    S = 3
    xs = []
    for s in range(S):
        lead = 40 + 64 * s
        x = np.concatenate([np.zeros(lead, np.float32), f1 * np.float32(0.8), np.zeros(90, np.float32), f2 * np.float32(0.6), np.zeros(800, np.float32)])
        xs.append(x)
    N = max(len(x) for x in xs)
    x = np.zeros((S, N), np.float32)
    for s in range(S):
        x[s, :len(xs[s])] = xs[s]
    x += (rng.standard_normal(x.shape) * 2e-3).astype(np.float32)
    # where does the reference raise stream 0's first 'eod'?
    probe = po.OracleCore({})
    n_e = None
    for i in range(0, N, 2):
        _, oe = probe.demodulate(x[0, i:i + 2])
        if oe:
            n_e = i + 2
            break
    assert n_e is not None and n_e % 2 == 0
    cut = n_e + 2 * after_reset + 1
    assert cut % 2 == 1 and cut < N - 2000
    eng = _engine({}, 0, S)
    oracles = [po.OracleCore({}) for _ in range(S)]
    oracles[0].enable_trace(N, 16)
    got = [b""] * S
    want = [b""] * S
    for a, b, reset in ((0, cut, True), (cut, cut + 1001, False), (cut + 1001, N, False)):
        out, eod = eng.demodulate_data(np.ascontiguousarray(x[:, a:b]))
        for s in range(S):
            ob, oe = oracles[s].demodulate(x[s, a:b])
            got[s] += out[s]
            want[s] += ob
            assert int(eod[s]) == oe, (s, a)
        if reset:
            eng.reset(1)          # odd decimator phase -> the batch leaves lock step -> generic kernel from here on
            oracles[1].reset()
            assert "demod_kernel" not in eng.last_kernel()
            eng.trace_enable(0, N)   # stream 0's I/Q magnitudes from the hand-over on
    assert "demod_kernel<float" in eng.last_kernel()
    # the decimated samples right behind the hand-over are where a wrong pair / a shifted correction shows: magnitudes within
    # 1e-5 of the reference's (relative, floored at 1e-4 of the peak as in test_intermediates_match_reference)
    tr, ref = eng.trace_read()["amp"], oracles[0].trace()["amp"]
    ref_tail = ref[cut // 2:]
    assert tr.size == ref_tail.size and tr.size > 1000
    rel = np.abs(tr - ref_tail) / np.maximum(ref_tail, 1.0e-4 * ref.max())
    assert rel[:200].max() <= 1e-5, (int(np.argmax(rel[:200])), rel[:200].max())
    for s in range(S):
        assert got[s] == want[s], (s, got[s], want[s])
        st, ost = eng.get_status(s), oracles[s].status()
        for k in STATUS_EXACT_KEYS:
            assert st[k] == ost[k], (s, k)
    assert b"Hello, generic kernel" in got[0]
    eng.close()


def test_host_calls_after_an_odd_length_call_stay_on_whole_tiles():
    """after one odd-length call the /2 decimators are mid-pair; an aligned staging buffer then needs an odd head
    for the parity and a multiple of four for the alignment, so every later even-length host call used to run sample by
    sample.  fskhip_demodulate_host now stages such calls three floats into the row (a head of one sample closes the pair AND
    reaches the 16-byte boundary)."""
    import webaudio_modem_amd as wm
    from oracle import pyoracle as po
    g = golden()
    base = g.array("d_default_Hello_c128.in")
    S = 64
    x = np.zeros((S, 12000), np.float32)
    for s in range(S):
        x[s, 100 + 3 * s:100 + 3 * s + base.size] = base
    eng = wm.FSKEngine(S, {}, precision=wm.PRECISION_F32)
    oracles = [po.OracleCore({}) for _ in range(S)]
    got = [b""] * S
    for a, b in ((0, 333), (333, 333 + 4096), (333 + 4096, 12000)):
        out, eod = eng.demodulate_data(np.ascontiguousarray(x[:, a:b]))
        if a == 333:
            assert "tail" not in eng.last_kernel(), eng.last_kernel()     # whole tiles although the call started mid-pair
        for s in range(S):
            ob, oe = oracles[s].demodulate(x[s, a:b])
            got[s] += out[s]
            assert out[s] == ob and int(eod[s]) == oe, (s, a)
    assert all(g_ == b"Hello" for g_ in got)
    eng.close()


def test_fp64_path_is_cut_invariant_bit_for_bit():
    """Round 6: the exact path must be exact under ANY cut of a stream into calls, like the reference
    (fsk-demodulation.node.test.ts:668-753 chunk sweeps) -- not only its bytes: every carried state word and every traced
    intermediate.  Rounds 1-5 re-evaluated the fp64 NCO's phasor every 32 samples counted from the start of each CALL (and did not
    carry it), so two cuts could differ by ~1e-14 in the I/Q branch; it is now part of the state and re-evaluated where the
    stream's absolute sample count is a multiple of 32.  One call against ragged schedules (odd lengths, single samples, lengths
    that put the refresh point at every position of a 16-sample block) on a noisy multi-frame batch."""
    import webaudio_modem_amd as wm
    g = golden()
    base = g.array("d_noise_bell_10dB_0.in")
    bell = dict(baudRate=1200, markFrequency=1200, spaceFrequency=2200)
    S = 70
    x = np.zeros((S, 3 * base.size + 700), np.float32)
    for s in range(S):
        for k in range(3):
            o = 11 * s + k * (base.size + 97)
            x[s, o:o + base.size] = base[:x.shape[1] - o] * (0.3 + 0.01 * s)
    N = x.shape[1]
    schedules = [[N], [1, 31, 17, 128, 5, 1000, 333, 2, 2, 7, 4096], [33] * 3 + [15, 1, 16, 1, 1, 13, 997], [128], [4095, 1]]
    results = []
    for sched in schedules:
        eng = wm.FSKEngine(S, bell, precision=wm.PRECISION_F64)
        eng.trace_enable(5, N // 2 + 8)
        rows = [b""] * S
        eods = np.zeros(S, np.int64)
        off = ci = 0
        while off < N:
            n = min(sched[ci % len(sched)], N - off)
            ci += 1
            out, eod = eng.demodulate_data(x[:, off:off + n].copy())
            for s in range(S):
                rows[s] += out[s]
            eods += np.asarray(eod, np.int64)
            off += n
        tr = eng.trace_read()
        state = [eng.debug_state(s) for s in range(S)]
        results.append((rows, eods, state, tr))
        eng.close()
    r0 = results[0]
    for sched, r in zip(schedules[1:], results[1:]):
        assert r[0] == r0[0], sched
        assert np.array_equal(r[1], r0[1]), sched
        for s in range(S):
            assert np.array_equal(np.asarray(r[2][s][0]).view(np.uint64), np.asarray(r0[2][s][0]).view(np.uint64)), (sched, s)
            assert r[2][s][1] == r0[2][s][1], (sched, s)
        for k in ("amp", "post_out", "pre_out"):
            assert np.array_equal(r[3][k].view(np.uint64), r0[3][k].view(np.uint64)), (sched, k)
        assert np.array_equal(r[3]["bit"], r0[3]["bit"]), sched


def test_exact_path_on_two_waves_is_the_one_wave_kernel_bit_for_bit():
    """Round 6 (second half): the fp64 kernel cut in two where resetState() never reaches -- loads + AGC + pre-filter | NCO
    ... frame logic, the pre-filter's floats handed over through LDS (option exact_waves = 2).  Exact by construction; here: bytes, 'eod'
    counts, every state word and the AGC write-back identical to the one-wave kernel on a ragged schedule.  (Not the default: at two
    waves per SIMD the back wave spills, 156 against 180 Gsamples/s -- DESIGN section 4.3.)"""
    import webaudio_modem_amd as wm
    g = golden()
    base = g.array("d_noise_bell_10dB_0.in")
    bell = dict(baudRate=1200, markFrequency=1200, spaceFrequency=2200)
    S = 150
    x = np.zeros((S, 2 * base.size + 500), np.float32)
    for s in range(S):
        for k in range(2):
            o = 7 * s + k * (base.size + 60)
            x[s, o:o + base.size] = base[:x.shape[1] - o] * (0.2 + 0.005 * s)
    N = x.shape[1]
    res = []
    for waves in (1, 2):
        eng = wm.FSKEngine(S, bell, precision=wm.PRECISION_F64, options={"exact_waves": waves})
        rows, eods, wb = [b""] * S, np.zeros(S, np.int64), []
        off = 0
        for n in [4096, 33, 1, 128, 5000, 17, 10 ** 9]:
            n = min(n, N - off)
            if n <= 0:
                break
            chunk = x[:, off:off + n].copy()
            out, eod = eng.demodulate_data(chunk, writeback_agc=True)
            wb.append(chunk)
            rows = [a + b for a, b in zip(rows, out)]
            eods += np.asarray(eod, np.int64)
            off += n
        assert ("two waves" in eng.last_kernel()) == (waves == 2), eng.last_kernel()
        res.append((rows, eods, [eng.debug_state(s) for s in range(S)], np.concatenate(wb, axis=1)))
        eng.close()
    assert res[0][0] == res[1][0] and np.array_equal(res[0][1], res[1][1])
    assert sum(len(r) for r in res[0][0]) > 10 * S
    assert np.array_equal(res[0][3], res[1][3])
    for (ra, ia), (rb, ib) in zip(res[0][2], res[1][2]):
        assert np.array_equal(np.asarray(ra).view(np.uint64), np.asarray(rb).view(np.uint64)) and ia == ib


@pytest.mark.gpu
def test_hand_off_fault_word_stays_clear_on_every_multi_wave_kernel():
    """ABI 8: every hand-off wait of the two-, four- and seven-wave kernels, of the exact path's two-wave cut and of the wide
    modulator is bounded (csrc/fsk_wait.h): a wave that gets nowhere in 2^22 polls of one wait flags the engine's fault word and ends
    its launch, and fskhip_synchronize / fskhip_get_faults / the next call report FSKHIP_E_HANDOFF.  A healthy launch never comes near
    the bound: here every such kernel runs a batch with resets in it, and synchronize() (which raises on the fault word) and
    faults() stay clean.  (The bound itself is exercised by tools/handoff_check.py on a -DFSK_SPIN_CAP_LOG2=0 build: profiles/.)"""
    import webaudio_modem_amd as wm
    from webaudio_modem_amd import _lib
    assert _lib.E_HANDOFF == -9
    g = golden()
    base = g.array("d_noise_bell_10dB_0.in")
    bell = dict(baudRate=1200, markFrequency=1200, spaceFrequency=2200)
    S = 200
    x = np.zeros((S, 2 * base.size + 4000), np.float32)
    for s in range(S):
        for k in range(2):
            o = 37 * (s % 50) + k * (base.size + 900)
            x[s, o:o + base.size] = base[:x.shape[1] - o] * (0.3 + 0.002 * s)
    ref = None
    for prec, opts, expect in ((wm.PRECISION_F32, {"kernel": "four-wave", "blk_resets": 0}, "demod_blk_kernel<"),
                               (wm.PRECISION_F32, {"kernel": "four-wave", "blk_resets": 1}, "demod_blk_kernel_r<"),
                               (wm.PRECISION_F32, {"kernel": "seven-wave"}, "demod_blk6_kernel"),
                               (wm.PRECISION_F32, {"kernel": "two-wave"}, "demod_pipe_kernel"),
                               (wm.PRECISION_F64, {"exact_waves": 2}, "two waves")):
        eng = wm.FSKEngine(S, bell, precision=prec, options=opts)
        rows, _ = eng.demodulate_data(x.copy())
        assert expect in eng.last_kernel(), (opts, eng.last_kernel())
        eng.synchronize()
        assert int(eng.faults().sum()) == 0
        if ref is None:
            ref = rows
            assert sum(len(r) for r in rows) > 10 * S
        assert rows == ref, opts
        eng.close()
    eng = wm.FSKEngine(S, bell, precision=wm.PRECISION_F64)
    sig = eng.modulate_data([b"hand-off %03d" % s for s in range(S)])
    eng.synchronize()
    assert len(sig) == S and all(len(v) > 0 for v in sig)
    eng.close()


@pytest.mark.gpu
def test_phase_wrap_within_rounding_of_pi_fp64_follows_the_reference():
    """tests/golden/soak_67001_phase_wrap.npy is the one stream in ~6 M soak stream-runs (tools/soak.py 1700 67001, round 6; default
    configuration, frames at 10-20 dB over noise) on which an fp32 engine decoded another byte than the reference for a reason that is
    neither of the two known marginal decisions: at decimated sample 1869 two consecutive I/Q samples of the noise in front of a frame
    point in opposite directions and the reference's phase difference is -3.141592052 -- 6.0e-7 from -pi, where fsk.ts:254-256 wraps.
    fp32 phases carry ~2e-7 of rounding: the fp32 engines wrap the other way, their post filter sees +pi instead of -pi and is
    somewhere else for the next few dozen samples (the slicer bits from sample 1872 on differ, one decoded byte with them).  That is
    the discontinuity of the reference's own function, not a defect -- the fp32 byte parity is a measured rate and
    the soak now classifies this case as it does the other two.  What IS asserted: the exact path gets it right -- the fp64 engine's
    bytes, 'eod' count and slicer bits are the oracle's on this stream, in one call and cut at the soak's 4096 -- and the fp32
    engine's amplitudes still agree to 1e-6 of the peak and its post filter to 1e-5 up to the wrap."""
    import webaudio_modem_amd as wm
    from oracle import pyoracle as po
    import os
    x = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "soak_67001_phase_wrap.npy"))
    o = po.OracleCore({})
    o.enable_trace(len(x), len(x))
    want, want_eod = o.demodulate(x)
    ot = o.trace()
    k = 1869
    assert abs(abs(float(ot["post_in"][k])) - np.pi) < 1e-6 and float(ot["post_in"][k]) < 0          # the case itself
    assert not np.any(np.abs(np.abs(ot["post_in"][:k]) - np.pi) < 1e-5)                              # ... and the first of its kind
    tr = {}
    for prec in (wm.PRECISION_F64, wm.PRECISION_F32):
        e = wm.FSKEngine(1, {}, precision=prec)
        e.trace_enable(0, len(x))
        out, eod = e.demodulate_data(x.reshape(1, -1).copy())
        tr[prec] = e.trace_read()
        if prec == wm.PRECISION_F64:
            assert out[0] == want and int(eod[0]) == want_eod
        e.close()
    t64, t32 = tr[wm.PRECISION_F64], tr[wm.PRECISION_F32]
    n = len(ot["bit"])
    assert np.array_equal(t64["bit"][:n], ot["bit"]) and np.allclose(t64["post_out"][:n], ot["post_out"], rtol=0, atol=1e-10)
    # (magnitudes do not see the phase: within 1e-6 of the stream's peak -- this is noise 40 dB under the frames, where the fp32 filters'
    # own rounding, ~1e-7 of the peak, is more than 1e-5 of the sample)
    assert np.abs(t32["amp"][:k + 200] - ot["amp"][:k + 200]).max() <= 1e-6 * ot["amp"].max()
    assert np.allclose(t32["post_out"][:k], ot["post_out"][:k], rtol=0, atol=1e-5)
    assert abs(t32["post_out"][k] - ot["post_out"][k]) > 1e-2                                        # (documented, not wished for)
    # cut where the soak cut it
    e = wm.FSKEngine(1, {}, precision=wm.PRECISION_F64)
    o2 = po.OracleCore({})
    for a, b in ((0, 4096), (4096, len(x))):
        out, eod = e.demodulate_data(x[a:b].reshape(1, -1).copy())
        ob, oe = o2.demodulate(x[a:b])
        assert out[0] == ob and int(eod[0]) == oe
    e.close()
