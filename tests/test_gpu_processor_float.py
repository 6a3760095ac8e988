"""FSKProcessorBatch.process(), the float-in, float-out streaming quantum (processor_io_kernel<EXACT> in webaudio_modem_amd/csrc/fsk_mod.hip:
the sequential generator FrameGen / frame_bit / frame_next_block<4, EXACT> resumed from its state words at every quantum, store_tile, the
RX ring puts), against the real reference's signals (tests/golden/golden_modulate.npz) and oracle.next_oracle.ProcessorOracle, which
tests/test_processor_ref_cpu.py holds to the same goldens in every schedule family.  No comparison here is against another GPU entry
point: the twin tests (test_gpu_processor_fmt, _rate, _ratecvt, _ratecvt_any, test_gpu_graph_replay) anchor on what this file pins.

The bar for samples is modulate_ref.check_signal per signal -- one modulation of one stream, whatever quanta it was cut into: fp64
engines the reference's bits; fp32 engines |diff| <= 1.2e-7 on at most max(1, n // 10000) samples, the exactly-zero samples (as
0x00000000 words) and the lengths identical.  Outside a modulation every word is 0x00000000.

A payload of no bytes stays pending for ever and emits zeros (chunked-modulator.ts:31-35), also where FSKCore.modulateData(empty) is a
signal: the twelve goldens with 0 payload bytes are held to that, and the coverage assertions count the other 33.

Observed on an MI355X (largest number of differing samples of one fp32 signal, per family): goldens, alone and at streams 0 / 63 / 64
of 65: 0 in all 45; sweep: 0 in all 20 (samples per bit, S) cells; store paths: 0; RX runs: 0, and every fp32 stream's bytes and ring
lengths the oracle's; long fp32 case: 0 of 542 920.  Long fp64 cases (tail samples that differ from the reference's, alone and as
stream 64 of 65 alike): long_stated_spb10 0 of 18 549, long_stated_spb32 0 of 18 858 (asserted); long_actual_spb10 0 of 26 339,
long_actual_spb32 0 of 26 703 (observed).  Quanta of 4096 are taken by the entry point as they are.

Value-only mutants of fsk_mod.hip, each run once against this file: frame_bit's parity inverted for odd parity fails the odd-parity
goldens and the sweep; frame_next_block advancing G.pos for a disabled sample fails the goldens, the sweep, the store paths, the long
cases and the RX runs in quanta of 37 and 1030; store_tile's scalar branch writing dst[3] unconditionally fails the store-path tests
(alone: the host entry point's padded pitch hides it); processor_io_kernel saving G.phase one increment late fails all but two
tests; the RX put loop not advancing r on a full ring fails the RX runs at capacities 3 and 16 and the off-grid input case.
"""
import functools

import numpy as np
import pytest

import processor_ref as pr
from hip_caller import Caller
from modulate_ref import (FRAMINGS, SENTINEL, RaggedRows, bits, check_signal, config, differing, golden_modulate, oracle_signal, ragged_payloads,
                          sha256, within_one_spacing)

pytestmark = pytest.mark.gpu

PRECISIONS = [("f64", 1), ("f32", 0)]


def _engine(cfg, prec, S=1):
    import webaudio_modem_amd as wm
    return wm.FSKEngine(S, cfg, device=0, precision=prec)


def _processor(eng, **kw):
    import webaudio_modem_amd as wm
    return wm.FSKProcessorBatch(eng, **kw)


def run_gpu(proc, ref, lens, modulations=None, resets=None, inputs=None, drains=(), n_out=None, process=None):
    """processor_ref.run_oracle's schedule on a FSKProcessorBatch, beside the oracle's Run `ref`: after every quantum tx_state() and
    rx_lengths() are the oracle's, at every drain demodulate() gives the oracle's bytes in order, and a modulate() call the oracle
    refused is refused here (such a call names refused streams only).  process(q, x, k) -> [S, k] float32 replaces proc.process.
    Returns the per-quantum outputs."""
    S, outs, t = proc.n_streams, [], 0
    base = proc.tx_state()["completed"].copy()
    for q, n in enumerate(lens):
        for s in (resets or {}).get(q, ()):
            proc.reset(s)
        starts = (modulations or {}).get(q, {})
        if starts:
            payloads, refused = [starts.get(s, b"") for s in range(S)], {s for (qq, s) in ref.refused if qq == q}
            if refused:
                assert refused == set(starts)
                before = proc.tx_state()
                with pytest.raises(RuntimeError, match="Modulation already in progress"):
                    proc.modulate(payloads, mask=[s in starts for s in range(S)])
                after = proc.tx_state()
                assert all(np.array_equal(before[k], after[k]) for k in ("samplePosition", "totalSamples", "pendingModulation", "completed"))
            else:
                proc.modulate(payloads, mask=[s in starts for s in range(S)])
        k = n if n_out is None else n_out
        x = None if inputs is None else inputs[:, t:t + n]
        outs.append(proc.process(x, k) if process is None else process(q, x, k))
        st = proc.tx_state()
        assert np.array_equal(st["pendingModulation"], ref.pending[q]), ("pendingModulation", q, np.flatnonzero(st["pendingModulation"] != ref.pending[q])[:4])
        assert np.array_equal(st["totalSamples"], ref.total[q]), ("totalSamples", q, np.flatnonzero(st["totalSamples"] != ref.total[q])[:4])
        assert np.array_equal(st["completed"] - base, ref.completed[q]), ("completed", q, np.flatnonzero(st["completed"] - base != ref.completed[q])[:4])
        got = proc.rx_lengths()
        assert np.array_equal(got, ref.ring_lens[q]), ("rx_lengths", q, np.flatnonzero(got != ref.ring_lens[q])[:4], got[:4], ref.ring_lens[q][:4])
        if q in drains:
            if q == min(drains):
                for s in (0, S - 1):
                    assert proc.status(s)["demodulatedBufferLength"] == int(ref.ring_lens[q][s]), (q, s)
            got = proc.demodulate()
            for s in range(S):
                assert got[s] == ref.drained[q][s], ("demodulate", q, s, got[s], ref.drained[q][s])
        t += n
    return outs


def check_streams(outs, ref, lens, cfgs, modulations, exact, streams=None, what=""):
    """every modulation of every stream as one signal under check_signal, against the oracle's samples over the span the modulation
    would take (a reset cuts it short: zeros in both from there on); 0x00000000 words everywhere else.  Returns the largest number of
    differing samples of one signal."""
    S = outs[0].shape[0]
    t_of = np.concatenate([[0], np.cumsum(lens)])
    worst = 0
    for s in (range(S) if streams is None else streams):
        got, want = np.concatenate([o[s] for o in outs]), ref.signal(s)
        assert got.size == want.size
        covered = np.zeros(got.size, bool)
        for q in sorted(modulations or {}):
            if s in modulations[q] and (q, s) not in ref.refused and len(modulations[q][s]):
                cfg = cfgs[s] if isinstance(cfgs, (list, tuple)) else cfgs
                a = int(t_of[q])
                b = min(a + oracle_signal(cfg, modulations[q][s]).size, got.size)
                worst = max(worst, check_signal(got[a:b], want[a:b], exact, "%s stream %d, modulation of quantum %d" % (what, s, q)))
                covered[a:b] = True
        assert not bits(want[~covered]).any()
        assert not bits(got[~covered]).any(), (what, "stream %d: not a 0x00000000 word outside a modulation" % s, np.flatnonzero(bits(got) * ~covered)[:4])
    return worst


# ---- a. the goldens through the generator ---------------------------------------------------------------------------------------------

NONEMPTY = [m for m in golden_modulate().short if m["payload"]]


def families_of(mc):
    """three schedule families per golden: over the 33 goldens with a payload every family meets every samples-per-bit value and every
    framing (asserted below).  The goldens without one (pending for ever, zeros) take theirs by their position in the list."""
    short = golden_modulate().short
    if not mc["payload"]:
        i = short.index(mc)
        return [pr.FAMILIES[(i + 3 * t) % 8] for t in range(3)]
    spbs = sorted({m["samplesPerBit"] for m in short})
    i = spbs.index(mc["samplesPerBit"])
    j = [m for m in NONEMPTY if m["samplesPerBit"] == mc["samplesPerBit"]].index(mc)
    return [pr.FAMILIES[(3 * j + 2 * i + t) % 8] for t in range(3)]


def test_the_rotation_of_families_covers_the_cross():
    assert len(NONEMPTY) == 33 and len(pr.FAMILIES) == 8
    met_spb = {(f, m["samplesPerBit"]) for m in NONEMPTY for f in families_of(m)}
    met_framing = {(f, m["framing"]) for m in NONEMPTY for f in families_of(m)}
    assert met_spb == {(f, spb) for f in pr.FAMILIES for spb in (5, 10, 20, 31, 32, 33, 40, 64, 147)}
    assert met_framing == {(f, fr) for f in pr.FAMILIES for fr in FRAMINGS}
    assert all(len(set(families_of(m))) == 3 for m in golden_modulate().short)


def _golden_plan(name, S, fam):
    """(lens, modulations, the golden's streams, the quantum in front of which they start): the golden as stream 0 alone, or as streams
    0, 63 and 64 of 65 started in front of quantum 2, while the other streams take payloads of 0 to 12 bytes in front of quantum 0
    (even streams) or quantum 4 (odd ones)"""
    mc = next(m for m in golden_modulate().short if m["name"] == name)
    payload, cfg, n = bytes(mc["payload"]), mc["config"], mc["n"]
    body = pr.quanta(n, fam, pr.tones_end(cfg, n))
    if S == 1:
        return body, {0: {0: payload}}, (0,), 0
    q = fam if isinstance(fam, int) else 128
    mine = (0, 63, 64)
    other = {s: bytes((7 * s + k) & 0xFF for k in range((5 * s + 3) % 13)) for s in range(S) if s not in mine}
    mods = {0: {s: p for s, p in other.items() if s % 2 == 0}, 2: {s: payload for s in mine}, 4: {s: p for s, p in other.items() if s % 2}}
    return [q, q] + body + [q, q], mods, mine, 2


@functools.lru_cache(maxsize=8)
def _golden_oracle(name, S, fam):
    """the oracle's run of one golden, S and family: computed once for both precisions"""
    mc = next(m for m in golden_modulate().short if m["name"] == name)
    lens, mods, mine, first = _golden_plan(name, S, fam)
    return pr.run_oracle(mc["config"], S, lens, mods)


@pytest.mark.parametrize("pname,prec", PRECISIONS)
@pytest.mark.parametrize("mc", golden_modulate().short, ids=lambda m: m["name"])
def test_process_gives_the_golden_alone_and_in_a_batch(mc, pname, prec):
    ref_sig, payload, cfg = golden_modulate().array(mc["signal"]), bytes(mc["payload"]), mc["config"]
    n, exact, worst = ref_sig.size, prec == 1, 0
    for S in (1, 65):
        eng = _engine(cfg, prec, S)
        proc = _processor(eng)
        for fam in families_of(mc):
            lens, mods, mine, first = _golden_plan(mc["name"], S, fam)
            ref = _golden_oracle(mc["name"], S, fam)
            proc.reset()
            outs = run_gpu(proc, ref, lens, mods)
            worst = max(worst, check_streams(outs, ref, lens, cfg, mods, exact, what="%s S %d" % (fam, S)))
            t0 = sum(lens[:first])
            for s in mine:
                got = np.concatenate([o[s] for o in outs])
                if payload:
                    worst = max(worst, check_signal(got[t0:t0 + n], ref_sig, exact, "%s S %d stream %d against the golden" % (fam, S, s)))
                    done = pr.completing_quantum(lens, n, first)
                    assert ref.completed[done][s] == 1 and (done == 0 or ref.completed[done - 1][s] == 0) and not ref.pending[done][s]
                else:
                    assert not bits(got).any() and ref.pending[-1][s] and ref.total[-1][s] == 0 and ref.completed[-1][s] == 0
        proc.close()
        eng.close()
    print("observed[golden %s %s] %d differing in one signal of %d" % (pname, mc["name"], worst, n))


# ---- b. sweep against the oracle ----------------------------------------------------------------------------------------------------------

SWEEP_SPBS, SWEEP_S, SWEEP_Q = (5, 10, 33, 40, 147), (1, 64, 65, 130), (128, 160, 37, 50)


def _sweep_cfgs(spb, framing, S):
    if S != 65:
        return config(spb, framing)
    cfgs = [config(spb, framing, tones=(1000 + 37 * s, 2000 + 41 * s)) for s in range(S)]       # per-stream tone pairs
    assert all(max(c["markFrequency"], c["spaceFrequency"]) < c["sampleRate"] / 2 for c in cfgs)
    return cfgs


def _sweep_plan(spb, framing, S, fi):
    """Two successive modulations per stream with a third refused while the second is pending, and reset() on two streams in the
    middle of their first modulation, which then take a new payload: (cfgs, lens, modulations, resets, the quantum length)."""
    cfgs = _sweep_cfgs(spb, framing, S)
    q = SWEEP_Q[(SWEEP_SPBS.index(spb) + SWEEP_S.index(S) + fi) % 4]
    seed = 100 * spb + 10 * S + fi
    first, second, third = (ragged_payloads(S, 7, seed + k) for k in (0, 1000, 2000))
    cfg_of = cfgs if isinstance(cfgs, list) else [cfgs] * S
    size = lambda s, p: oracle_signal(cfg_of[s], p).size if len(p) else 0
    longest = max(size(s, first[s]) for s in range(S))
    hit = sorted(sorted(range(S), key=lambda s: -len(first[s]))[:2])      # the two streams with the longest payloads are reset
    q_reset = (longest // 3) // q + 1
    end_new = (q_reset + 1) * q + size(hit[0], b"\x5a")
    q_second = (max(longest, end_new) - 1) // q + 2            # every modulation before it is over, one quantum ago
    again = {s: second[s] for s in range(S) if len(first[s])}      # (a stream with an empty first payload is pending for ever)
    longest2 = max(size(s, p) for s, p in again.items())
    n_quanta = q_second + (longest2 - 1) // q + 2
    busy = [s for s in again if len(second[s]) == 7][:3]             # still modulating one quantum later: their third call is refused
    mods = {0: dict(enumerate(first)), q_reset + 1: {s: b"\x5a" for s in hit}, q_second: again, q_second + 1: {s: third[s] for s in busy}}
    assert 0 < q_reset < q_reset + 1 < q_second and busy and min(size(s, second[s]) for s in busy) > q
    return cfgs, [q] * n_quanta, mods, {q_reset: hit}, q


@functools.lru_cache(maxsize=8)
def _sweep_oracle(spb, framing, S, fi):
    cfgs, lens, mods, resets, q = _sweep_plan(spb, framing, S, fi)
    return pr.run_oracle(cfgs, S, lens, mods, resets)


@pytest.mark.parametrize("pname,prec", PRECISIONS)
@pytest.mark.parametrize("S", SWEEP_S)
@pytest.mark.parametrize("spb", SWEEP_SPBS)
def test_process_sweep_matches_the_oracle(spb, S, pname, prec):
    worst = 0
    for fi, framing in enumerate(FRAMINGS):
        cfgs, lens, mods, resets, q = _sweep_plan(spb, framing, S, fi)
        ref = _sweep_oracle(spb, framing, S, fi)
        (q_reset, hit), = resets.items()
        # the plan does what it says: the reset streams were in the middle of a modulation, are silent from the next quantum on and
        # take their new payload; the third call is refused; streams with an empty payload stay pending
        assert all(ref.pending[q_reset - 1][s] and bits(ref.outs[q_reset - 1][s]).any() and not bits(ref.outs[q_reset][s]).any() for s in hit)
        assert all(ref.pending[q_reset + 1][s] or ref.completed[q_reset + 1][s] == 1 for s in hit) and len(ref.refused) == len(mods[max(mods)]) > 0
        assert S == 1 or np.stack(ref.pending).all(axis=0).any()
        eng = _engine(cfgs, prec, S)
        proc = _processor(eng)
        outs = run_gpu(proc, ref, lens, mods, resets)
        worst = max(worst, check_streams(outs, ref, lens, cfgs, mods, prec == 1, what="%s q %d" % (framing, q)))
        assert (ref.completed[-1] >= 1).sum() >= (S + 1) // 2
        proc.close()
        eng.close()
    print("observed[sweep %s spb %d S %d] %d differing in one signal" % (pname, spb, S, worst))


# ---- c. the store paths, through process_device on a caller's stream -------------------------------------------------------------------

STORE_N_OUT, STORE_S = (1, 3, 4, 31, 32, 33, 37, 50, 128), (1, 63, 65, 130)
STORE_CFG = config(10, "8n1")


def _store_plan(S):
    """Every n_out at every shift of the first element behind a 16-byte boundary and every pitch -- (lens, [(shift, pitch)], modulations):
    each stream takes its next payload in front of the quantum after the one in which its modulation completed, so that over the run
    modulations complete at many columns of a row."""
    lens, where = [], []
    for n_out in STORE_N_OUT:
        for shift in (0, 4, 8, 12):
            for pitch in sorted({n_out, n_out + 1, n_out + 3, (n_out + 3) // 4 * 4}):
                lens.append(n_out)
                where.append((shift, pitch))
    sets = [ragged_payloads(S, 7, 31 * S + k) if S > 1 else [bytes([17 * k + 1] * (k % 4 + 1))] for k in range(12)]      # (one stream: 1 to 4 bytes in turn)
    mods, ends, left, k_of = {}, {}, np.zeros(S, np.int64), np.zeros(S, np.int64)
    for q, n in enumerate(lens):
        for s in range(S):
            if left[s] <= 0 and k_of[s] >= 0:
                p = sets[k_of[s] % 12][s] or (b"\x33" if k_of[s] else b"")     # (an empty payload only as a stream's first: it ends the stream's turns)
                mods.setdefault(q, {})[s] = p
                left[s] = oracle_signal(STORE_CFG, p).size if p else 0
                k_of[s] = k_of[s] + 1 if p else -1
            if 0 < left[s] <= n:
                ends[(q, s)] = int(left[s])          # the column behind the modulation's last sample
        left -= n
    return lens, where, mods, ends


@functools.lru_cache(maxsize=4)
def _store_oracle(S):
    lens, where, mods, ends = _store_plan(S)
    return pr.run_oracle(STORE_CFG, S, lens, mods)


@pytest.mark.parametrize("pname,prec", PRECISIONS)
@pytest.mark.parametrize("S", STORE_S)
def test_process_device_store_paths_and_no_stray_writes(S, pname, prec):
    """store_tile's 16-byte stores (base on the 16-byte grid and a pitch of a multiple of four floats) and its single stores (every
    other base and pitch): columns < n_out of rows < S are the oracle's, every other word of the sentinel-framed buffer keeps its
    sentinel -- in the quanta in which modulations complete in the middle of a row too, where the rest of the row is 0x00000000."""
    lens, where, mods, ends = _store_plan(S)
    ref = _store_oracle(S)
    assert not ref.refused and (S == 1 or ref.pending[-1].any())
    vec = {(n, sh == 0 and p % 4 == 0) for n, (sh, p) in zip(lens, where)}
    assert vec == {(n, v) for n in STORE_N_OUT for v in (False, True)}, "both store paths at every n_out"
    mid_row = [(q, s) for (q, s), col in ends.items() if col < lens[q]]
    assert len(mid_row) >= 3 and all(ref.completed[q][s] == (ref.completed[q - 1][s] if q else 0) + 1 for q, s in ends)
    assert S == 1 or {where[q][0] == 0 and where[q][1] % 4 == 0 for q, s in mid_row} == {False, True}, "... on both store paths"
    eng = _engine(STORE_CFG, prec, S)
    proc = _processor(eng)
    c = Caller(eng)

    def process(q, x, k):
        shift, pitch = where[q]
        rows = RaggedRows(c, S, pitch, shift)
        proc.process_device(None, 0, 0, rows.ptr, k, pitch, stream=c.stream)
        body = rows.read()
        assert (body[:, k:] == SENTINEL).all(), ("quantum %d: written from column %d on" % (q, k), where[q])
        for s in range(S):
            if (q, s) in ends:
                assert not body[s, ends[(q, s)]:k].any(), ("quantum %d stream %d: 0x00000000 words behind the completed modulation" % (q, s))
        return np.ascontiguousarray(body[:, :k]).view(np.float32)

    outs = run_gpu(proc, ref, lens, mods, process=process)
    worst = check_streams(outs, ref, lens, STORE_CFG, mods, prec == 1, what="store S %d" % S)
    print("observed[store %s S %d] %d differing in one signal; %d completions mid-row" % (pname, S, worst, len(mid_row)))
    c.close()
    proc.close()
    eng.close()


# ---- d. the long carried phase -----------------------------------------------------------------------------------------------------------------

def _long_run(lc, prec, S):
    """the long case as the last of S streams (its neighbours: short payloads in front of quantum 0), in quanta of 4096 with twelve of
    37 across the recorded crossing -> its samples"""
    g = golden_modulate()
    payload = bytes(g.array(lc["payload"]))
    lens = pr.long_quanta(lc["n"], lc["cross"])
    eng = _engine(lc["config"], prec, S)
    proc = _processor(eng)
    proc.modulate([bytes([s, 0x55, 0xFF][:1 + s % 3]) for s in range(S - 1)] + [payload])
    parts = []
    for q, n in enumerate(lens):
        out = proc.process(None, n)
        parts.append(out[S - 1].copy())
        if S > 1 and q > 0:
            assert not bits(out[:S - 1]).any(), "the short neighbours are over"
    st = proc.tx_state()
    assert not st["pendingModulation"].any() and (st["completed"] == 1).all()
    proc.close()
    eng.close()
    return np.concatenate(parts)


@pytest.mark.parametrize("S", [1, 65])
@pytest.mark.parametrize("lc", golden_modulate().long, ids=lambda m: m["name"])
def test_process_long_signal_across_the_sine_limit(lc, S):
    """fp64 engines: tx_phase carried over hundreds of quanta, from sin_straight through ref_sin to the device library's sin() beyond
    2^20 * pi/2.  The digest of the samples before the crossing is the golden's; from the crossing on every sample is within one
    float32 spacing of the recorded one (identical where the limit is the "stated" 2^19 * pi/2, inside the restated range)."""
    tail = golden_modulate().array(lc["tail"])
    sig = _long_run(lc, 1, S)
    assert sha256(sig[:lc["cross"]]) == lc["prefix_sha256"]
    got = sig[lc["cross"]:lc["n"]]
    n_diff = differing(got, tail)
    print("observed[long %s S %d] %d of %d tail samples differ from the reference's" % (lc["name"], S, n_diff, tail.size))
    assert within_one_spacing(got, tail)
    if lc["limit"] == "stated":
        assert n_diff == 0
    assert not bits(sig[lc["n"]:]).any() and sig.size > lc["n"]


def test_process_long_signal_fp32():
    lc = golden_modulate().long[0]
    want = oracle_signal(lc["config"], bytes(golden_modulate().array(lc["payload"])))
    sig = _long_run(lc, 0, 1)
    n_diff = check_signal(sig[:lc["n"]], want, False, lc["name"])
    print("observed[long f32 %s] %d of %d samples differ from the oracle's" % (lc["name"], n_diff, want.size))
    assert not bits(sig[lc["n"]:]).any()


# ---- e. RX bookkeeping per quantum -----------------------------------------------------------------------------------------------------------------

RX_CFG = config(10, "8n1")                      # 100 samples per byte: a quantum of 1030 yields ten bytes
RX_QUANTA, RX_CAPS = (128, 160, 37, 1030), (1, 3, 16, 48, 1024)
RX_RUNS = [(cap, clear) for cap in RX_CAPS for clear in (True, False)]


def _rx_quantum(S, run):
    c, k = divmod(run, 2)
    return RX_QUANTA[(2 * c + k) % 4 if S == 65 else (2 * c + 3 - k) % 4]


def test_the_rx_rotation_covers_the_cross():
    met = {(_rx_quantum(S, run), cap, clear) for S in (65, 130) for run, (cap, clear) in enumerate(RX_RUNS)}
    assert {(q, cap) for q, cap, _ in met} == {(q, cap) for q in RX_QUANTA for cap in RX_CAPS}
    assert {(q, clear) for q, _, clear in met} == {(q, clear) for q in RX_QUANTA for clear in (True, False)}


@functools.lru_cache(maxsize=2)
def _rx_input(S):
    """clean frames of 20 to 60 bytes at 0.9 of full scale behind even and odd leads, no noise; read-only"""
    rng = np.random.default_rng(0xE0 + S)
    sigs = [oracle_signal(RX_CFG, bytes(rng.integers(0, 256, int(rng.integers(20, 61)), dtype=np.uint8))) for _ in range(S)]
    leads = [int(rng.integers(0, 200)) * 2 + s % 2 for s in range(S)]
    x = np.zeros((S, max(l + s.size for l, s in zip(leads, sigs)) + 200), np.float32)
    for s in range(S):
        x[s, leads[s]:leads[s] + sigs[s].size] = np.float32(0.9) * sigs[s]
    x.setflags(write=False)
    return x


def _rx_plan(S, run):
    q = _rx_quantum(S, run)
    x = _rx_input(S)
    lens = [q] * (x.shape[1] // q) + ([x.shape[1] % q] if x.shape[1] % q else [])
    tx = ragged_payloads(S, 12, 7 * S + run)                  # modulations that complete while bytes sit in the rings
    drains = {len(lens) // 4, len(lens) // 2, 3 * len(lens) // 4, len(lens) - 1}
    return q, x, lens, {0: dict(enumerate(tx))}, drains


@functools.lru_cache(maxsize=4)
def _rx_oracle(S, run):
    cap, clear = RX_RUNS[run]
    q, x, lens, mods, drains = _rx_plan(S, run)
    return pr.run_oracle(RX_CFG, S, lens, mods, inputs=x, drains=drains, rx_capacity=cap, clear_rx_on_tx_complete=clear)


@pytest.mark.parametrize("pname,prec", PRECISIONS)
@pytest.mark.parametrize("run", range(len(RX_RUNS)), ids=["cap%d-%s" % (c, "clear" if k else "keep") for c, k in RX_RUNS])
@pytest.mark.parametrize("S", [65, 130])
def test_rx_rings_follow_the_oracle_every_quantum(S, run, pname, prec):
    """after every quantum rx_lengths() equals the oracle rings' lengths; at three drains and at the end demodulate() gives the oracle's
    bytes in order, overwrite-the-oldest included; the TX samples are the oracle's all the while"""
    cap, clear = RX_RUNS[run]
    q, x, lens, mods, drains = _rx_plan(S, run)
    ref = _rx_oracle(S, run)
    # the stimulus: a modulation completed while its ring held bytes; small rings ran over
    done = [pr.completing_quantum(lens, oracle_signal(RX_CFG, p).size) for p in mods[0].values() if p]
    plain = sum(len(b) for d in ref.drained.values() for b in d)
    assert plain > 0 and (cap >= 48 or max(int(r.max()) for r in ref.ring_lens) == cap)
    assert any(ref.ring_lens[d - 1][s] > 0 for s, d in zip([s for s, p in mods[0].items() if p], done) if d)
    eng = _engine(RX_CFG, prec, S)
    proc = _processor(eng, rx_capacity=cap, clear_rx_on_tx_complete=clear)
    outs = run_gpu(proc, ref, lens, mods, inputs=x, drains=drains)
    worst = check_streams(outs, ref, lens, RX_CFG, mods, prec == 1, what="rx")
    print("observed[rx %s S %d cap %d q %d] %d differing in one signal, %d bytes drained" % (pname, S, cap, q, worst, plain))
    proc.close()
    eng.close()


@pytest.mark.parametrize("pname,prec", PRECISIONS)
def test_rx_input_from_a_pointer_off_the_16_byte_grid(pname, prec):
    """the input through process_device from a pointer 4, 8 and 12 bytes behind a 16-byte boundary, rows in_pitch = n_in + 1 or + 3
    floats apart (no multiple of four): the same rings"""
    S, run = 65, 4                                  # capacity 16, cleared on completion
    cap, clear = RX_RUNS[run]
    q, x, lens, mods, drains = _rx_plan(S, run)
    assert q % 4 == 0 and (cap, clear) == (16, True)
    ref = _rx_oracle(S, run)
    for shift in (4, 8, 12):
        pitch = q + (1 if shift != 8 else 3)
        assert pitch % 4
        eng = _engine(RX_CFG, prec, S)
        proc = _processor(eng, rx_capacity=cap, clear_rx_on_tx_complete=clear)
        c = Caller(eng)
        d_in = c.malloc(4 * (S * pitch + 8)) + shift
        d_out = c.malloc(4 * S * q)

        def process(i, xq, k):
            slab = np.zeros((S, pitch), np.float32)
            slab[:, :xq.shape[1]] = xq
            c.upload(d_in, slab)
            proc.process_device(d_in, xq.shape[1], pitch, d_out, k, q, stream=c.stream)
            c.sync()
            return c.download(d_out, np.empty((S, q), np.float32))[:, :k].copy()

        outs = run_gpu(proc, ref, lens, mods, inputs=x, drains=drains, process=process)
        check_streams(outs, ref, lens, RX_CFG, mods, prec == 1, what="rx shift %d" % shift)
        c.close()
        proc.close()
        eng.close()
