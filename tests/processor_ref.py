"""What the FSKProcessor float-quantum tests share (tests/test_processor_ref_cpu.py on the CPU, tests/test_gpu_processor_float.py on
the GPU): the schedule families that cut a modulation into quanta, and a driver that takes one oracle.next_oracle.ProcessorOracle per
stream through such a schedule.  Nothing here calls the code under test."""
import numpy as np

from oracle import next_oracle as no
from oracle import pyoracle as po

# Schedule families for a modulation of n samples; each runs to one quantum past the one that holds the last sample.
#   128, 160      the real-time quantum, a 20 ms frame at 8 kHz
#   37            odd: ends inside a 32-sample tile and inside a four-sample block
#   3             shorter than a four-sample block
#   50            ends inside the 32-sample tile
#   "ones"        1 for the first 70 samples, then 128
#   "single"      one call of n + 5: the modulation starts and completes in the same quantum
#   "tones"       one quantum whose last sample is the frame's last tone sample, then 128
FAMILIES = (128, 160, 37, 3, 50, "ones", "single", "tones")


def bits_per_byte(cfg):
    return cfg.get("startBits", 1) + 8 + (1 if cfg.get("parity", "none") not in ("none", 0) else 0) + cfg.get("stopBits", 1)


def tones_end(cfg, n):
    """the number of samples of an n-sample frame up to its last tone sample: one byte's worth of silence follows (fsk.ts:389-424)"""
    return n - bits_per_byte(cfg) * (cfg.get("sampleRate", 48000) // cfg["baudRate"])


def quanta(total, pattern, tones=None):
    """Quantum lengths that carry a modulation of `total` samples, started in front of the first quantum, to its end and one quantum
    beyond.  pattern: one of FAMILIES; `tones` (for "tones"): tones_end() of the frame."""
    if pattern == "single":
        return [total + 5, 128]
    head = {"ones": [1] * 70, "tones": [tones]}.get(pattern, [])
    q = pattern if isinstance(pattern, int) else 128
    lens = list(head)
    while sum(lens) < total:
        lens.append(q)
    while sum(lens[:-1]) >= total:     # (a head that overshoots a short frame)
        lens.pop()
    return lens + [q]


def long_quanta(total, cross, q=4096, short=37, k=12):
    """quanta of q with a stretch of k quanta of `short` samples laid across sample `cross`, to the end of `total` and one beyond"""
    before = cross - short * k // 2
    lens = [q] * (before // q) + ([before % q] if before % q else []) + [short] * k
    assert sum(lens) - short * k < cross < sum(lens)
    while sum(lens) < total:
        lens.append(q)
    return lens + [q]


def completing_quantum(lens, total, start=0):
    """index of the quantum that holds the last sample of a modulation of `total` samples started in front of quantum `start`"""
    t = 0
    for q in range(start, len(lens)):
        t += lens[q]
        if t >= total:
            return q
    return None


class Run:
    """what run_oracle returns: per quantum q -- outs[q] float32 [S, lens[q]], ring_lens[q], pending[q], total[q], completed[q] (each
    of S entries, as they stand after the quantum) -- and drained {q: S byte strings} for the drains behind quantum q"""

    def __init__(self):
        self.outs, self.ring_lens, self.pending, self.total, self.completed, self.drained, self.refused = [], [], [], [], [], {}, []

    def signal(self, s):
        return np.concatenate([o[s] for o in self.outs])


def run_oracle(cfgs, S, lens, modulations=None, resets=None, inputs=None, drains=(), rx_capacity=1024, clear_rx_on_tx_complete=True, n_out=None):
    """One ProcessorOracle per stream (cfgs: one config for all S, or a list of S) through the quanta `lens`.
    modulations: {q: {stream: payload}} -- modulate() calls in front of quantum q; one on a stream whose modulation is pending is
    refused like the reference's ("Modulation already in progress"), noted in Run.refused as (q, stream) and otherwise without effect.
    resets: {q: [streams]} -- reset() (fsk-processor.ts:137-143: ring cleared, pending modulation dropped) in front of quantum q, before
    that quantum's modulate() calls.  inputs: float32 [S, sum(lens)] or None; drains: quanta behind which demodulate() empties every ring.
    n_out: output samples per quantum (default: lens; 0 for none)."""
    cfg_of = list(cfgs) if isinstance(cfgs, (list, tuple)) else [cfgs] * S
    assert len(cfg_of) == S and (inputs is None or inputs.shape == (S, sum(lens)))
    oracles = [no.ProcessorOracle(po.OracleCore(c), rx_capacity=rx_capacity, clear_rx_on_tx_complete=clear_rx_on_tx_complete) for c in cfg_of]
    run, t = Run(), 0
    for q, n in enumerate(lens):
        for s in (resets or {}).get(q, ()):
            oracles[s].ring.clear()
            oracles[s].pending = None
        for s, payload in sorted((modulations or {}).get(q, {}).items()):
            try:
                oracles[s].modulate(payload)
            except RuntimeError as e:
                assert str(e) == "Modulation already in progress"
                run.refused.append((q, s))
        k = n if n_out is None else n_out
        run.outs.append(np.stack([o.process(None if inputs is None else inputs[s, t:t + n], k) for s, o in enumerate(oracles)]))
        run.ring_lens.append(np.array([o.ring.length for o in oracles], np.uint32))
        run.pending.append(np.array([o.pending is not None for o in oracles]))
        run.total.append(np.array([0 if o.pending is None or o.pending.pending is None else len(o.pending.pending) for o in oracles], np.uint32))
        run.completed.append(np.array([o.completed for o in oracles], np.uint32))
        if q in drains:
            run.drained[q] = [o.demodulate() for o in oracles]
        t += n
    return run
