"""The reference side of tests/test_gpu_processor_float.py by itself, without a GPU: oracle.next_oracle.ProcessorOracle, cut into each
schedule family of tests/processor_ref.py, gives the real reference's signals (tests/golden/golden_modulate.npz) bit for bit, zeros
behind them, completes in the quantum that holds the last sample and clears its ring exactly there.  A mismatch of the GPU test is
then the kernel's and not the model's.

A payload of no bytes: FSKCore.modulateData(empty) is a signal where the framing has a preamble (the goldens with 0 payload bytes), but
ChunkedModulator.startModulation(empty) resets and returns (chunked-modulator.ts:31-35), so the processor's modulation stays pending
for ever and emits zeros.  Those goldens are held to that."""
import numpy as np
import pytest

import processor_ref as pr
from modulate_ref import bits, differing, golden_modulate, sha256, within_one_spacing


@pytest.mark.parametrize("mc", golden_modulate().short, ids=lambda m: m["name"])
def test_processor_oracle_in_every_schedule_family_gives_the_golden(mc):
    ref, payload, cfg = golden_modulate().array(mc["signal"]), bytes(mc["payload"]), mc["config"]
    n = ref.size
    assert pr.tones_end(cfg, n) == int(np.flatnonzero(bits(ref))[-1]) + 1        # the last tone sample is where the helper says
    for fam in pr.FAMILIES:
        lens = pr.quanta(n, fam, pr.tones_end(cfg, n))
        assert sum(lens[:-2]) < n <= sum(lens[:-1]), (fam, "one quantum past the one that holds the last sample")
        run = pr.run_oracle(cfg, 1, lens, {0: {0: payload}})
        sig = run.signal(0)
        if not payload:
            assert not bits(sig).any() and all(p[0] for p in run.pending) and run.completed[-1][0] == 0 and run.total[-1][0] == 0, fam
            continue
        assert np.array_equal(bits(sig[:n]), bits(ref)), fam
        assert not bits(sig[n:]).any() and sig.size > n, (fam, "zeros behind the signal")
        done = pr.completing_quantum(lens, n)
        assert done == len(lens) - 2
        assert [int(c[0]) for c in run.completed] == [0] * done + [1] * (len(lens) - done), fam
        assert [bool(p[0]) for p in run.pending] == [True] * done + [False] * (len(lens) - done), fam
        assert [int(t[0]) for t in run.total] == [n] * done + [0] * (len(lens) - done), fam


@pytest.mark.parametrize("clear", [True, False])
def test_processor_oracle_clears_its_ring_in_the_completing_quantum_only(clear):
    """bytes arrive while the modulation runs (a clean frame in the input); the ring is cleared in the quantum that holds the
    modulation's last sample and nowhere else"""
    from modulate_ref import config, oracle_signal
    cfg = config(40)
    heard = oracle_signal(cfg, bytes(range(30, 50)))
    tx = oracle_signal(cfg, b"\x55\xaa")
    lens = pr.quanta(tx.size, 128)
    x = np.zeros((1, sum(lens)), np.float32)
    x[0, :] = (np.float32(0.9) * heard)[:x.shape[1]]
    run = pr.run_oracle(cfg, 1, lens, {0: {0: b"\x55\xaa"}}, inputs=x, clear_rx_on_tx_complete=clear, rx_capacity=16)
    plain = pr.run_oracle(cfg, 1, lens, inputs=x, rx_capacity=16, n_out=0)       # the same input without a modulation
    done = pr.completing_quantum(lens, tx.size)
    held = [int(r[0]) for r in plain.ring_lens]
    assert held[done] >= 3, "bytes sit in the ring when the modulation completes"
    got = [int(r[0]) for r in run.ring_lens]
    assert got[:done] == held[:done]
    assert got[done] == (0 if clear else held[done])
    assert got[done + 1] == held[done + 1] - (held[done] if clear else 0)
    assert np.array_equal(bits(run.signal(0)[:tx.size]), bits(tx))


@pytest.mark.parametrize("lc", golden_modulate().long, ids=lambda m: m["name"])
def test_processor_oracle_long_signal_across_the_sine_limit(lc):
    """as tests/test_oracle_modulate_edges.py has it for modulate(): the digest before the crossing, the recorded samples from it on"""
    g = golden_modulate()
    tail = g.array(lc["tail"])
    lens = pr.long_quanta(lc["n"], lc["cross"])
    run = pr.run_oracle(lc["config"], 1, lens, {0: {0: bytes(g.array(lc["payload"]))}})
    sig = run.signal(0)
    assert sha256(sig[:lc["cross"]]) == lc["prefix_sha256"]
    got = sig[lc["cross"]:lc["n"]]
    n_diff = differing(got, tail)
    print("%s: %d of %d tail samples differ from the reference's" % (lc["name"], n_diff, tail.size))
    assert within_one_spacing(got, tail)
    if lc["limit"] == "stated":
        assert n_diff == 0
    assert not bits(sig[lc["n"]:]).any()
    done = pr.completing_quantum(lens, lc["n"])
    assert done == len(lens) - 2 and [int(c[0]) for c in run.completed][done - 1:] == [0, 1, 1]


def test_the_families_cut_where_they_should():
    assert pr.quanta(300, 128) == [128, 128, 128, 128] and pr.quanta(256, 128) == [128, 128, 128]
    assert pr.quanta(110, 37) == [37, 37, 37, 37] and pr.quanta(210, "single") == [215, 128]
    assert pr.quanta(110, "ones") == [1] * 70 + [128, 128] and pr.quanta(310, "tones", 255) == [255, 128, 128]
    lens = pr.long_quanta(542920, 524371)
    assert lens.count(37) == 12 and max(lens) == 4096 and sum(lens[:lens.index(37)]) < 524371 < sum(lens[:lens.index(37) + 12])
    assert sum(lens[:-2]) < 542920 <= sum(lens[:-1])
