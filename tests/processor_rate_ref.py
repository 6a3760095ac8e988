"""The model of an 8 kHz link between two FSKProcessors (include/fskhip_next.h: fskhip_processor_process_rate_*): one side's pending
modulation decimated by 6 into mu-law quanta of 160 samples, the other side's interpolator and demodulator fed with them quantum by
quantum, both filters carrying their delay lines -- tests/resample_ref.py over oracle/pyoracle.py.  Not a test;
test_processor_rate_cpu.py holds it to the payload, and test_gpu_processor_rate.py two processors to its bytes."""
import numpy as np

import resample_ref as rr
from oracle import pyoracle as po

FACTOR, QUANTUM, FMT = 6, 160, "mulaw"
PAYLOAD = b"8 kHz trunk, 20 ms quanta"
# quanta of silence run behind the last one that holds signal.  The model needs none: a frame ends in bitsPerByte * samplesPerBit
# zeros of its own (fsk.ts:391-394), longer than the decimator's and the interpolator's delays (48 + 48 samples at 48 kHz) and the
# demodulator's, so the last byte is out before the signal's last quantum ends (test_processor_rate_cpu.py asserts it).  One is run
# all the same: the decimator rings into it, and it must add no byte.
TRAILING_QUANTA = 1


def signal_quanta(n_signal):
    """quanta that hold samples of a modulation of n_signal high rate samples"""
    return -(-n_signal // (FACTOR * QUANTUM))


def link(payload=PAYLOAD, trailing=TRAILING_QUANTA, cfg=None):
    """(the mu-law quanta on the wire, [n][160] uint8; the bytes the far side's demodulator returns, quantum by quantum)"""
    tx, rx = po.OracleCore(cfg), po.OracleCore(cfg)
    sig = np.asarray(tx.modulate(payload), np.float32)
    down = [po.FIR(list(rr.default_taps(FACTOR)))]
    up = [po.FIR(list(rr.default_taps(FACTOR, up=True)))]
    step = FACTOR * QUANTUM
    wire, got = [], []
    for q in range(signal_quanta(sig.size) + trailing):
        chunk = np.zeros(step, np.float32)
        part = sig[q * step:(q + 1) * step]          # modulateTo: zero fill, then what is left of the signal
        chunk[:part.size] = part
        low = rr.down(chunk, rr.default_taps(FACTOR), FACTOR, FMT, filters=down)
        high = rr.up(low, FMT, rr.default_taps(FACTOR, up=True), FACTOR, filters=up)
        data, _eod = rx.demodulate(high[0])
        wire.append(low[0])
        got.append(bytes(data))
    return np.stack(wire), got
