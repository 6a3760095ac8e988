"""FSKProcessorBatch(use_graph=True) against the plain launches, bit for bit, on every launch path.

A captured quantum (csrc/fsk_proc.h, run_quantum) holds every launch's arguments BY VALUE and is replayed while its key stays the
same; whatever the host advances from call to call -- the decimator parity, the amplitude ring's position, the fp64 NCO anchor --
has to be in that key (csrc/fsk_dispatch.hip, engine_launch_key), or a replay computes with the value of the capture.  Twin
processors over twin engines take the same samples, one with use_graph=False, one with use_graph=True:
  after every quantum   the output samples are byte-equal, and so are snapshot().processor and snapshot().engine (every state
                        word, the amplitude ring, the polyphase registers, the host's counters);
  at the end of a run   the drained RX bytes and the 'eod' counts are equal, and are the oracle's on the same samples; an fp64
                        engine's state is also that of a third engine that took the whole input in ONE demodulate_data call;
  replays happened      fskhip_processor_graph_stats per schedule entry is what run_quantum's key gives (KeyModel below), which for
                        every entry of a multiple of 32 samples at even parity is: all calls but the first are replays.
No tolerance anywhere."""
import re

import numpy as np
import pytest

import samples_ref as sr

pytestmark = pytest.mark.gpu

BELL = dict(baudRate=1200, markFrequency=1200, spaceFrequency=2200)       # 40 samples per bit
# Each length four times in a row, each there to move one quantity a capture holds by value: 128 the control; 160 a multiple of 32
# but not of 128; 100 and 48 no multiples of 32 (the fp64 NCO anchor moves); 37 and 1 odd (the decimator parity, and the fp32
# generic kernel's open pair, flip on every call); 20 moves the amplitude ring off its quad grid; 16 exactly one tile; then 128
# from whatever position that left, to the end of the input.
LENGTHS = (128, 160, 100, 48, 37, 1, 20, 16)
REPS = 4
GAP = 640                       # near-silence behind each frame: 'eod' resets inside replayed quanta

# name -> (precision, streams, options, how the streams' configurations are made, what last_kernel must name after a quantum of
# 128 or 160 samples)
PATHS = {
    "f32-auto": ("F32", 65, {}, "bell", r"demod_(blk6|blk|pipe|fused)_kernel"),
    "f32-seven-wave": ("F32", 65, {"kernel": "seven-wave", "blk_resets": 1}, "bell", r"demod_blk6_kernel<"),
    "f32-four-wave-resets0": ("F32", 65, {"kernel": "four-wave", "blk_resets": 0}, "bell", r"demod_blk_kernel<"),
    "f32-four-wave-resets1": ("F32", 65, {"kernel": "four-wave", "blk_resets": 1}, "bell", r"demod_blk_kernel_r<"),
    "f32-two-wave": ("F32", 65, {"kernel": "two-wave"}, "bell", r"demod_pipe_kernel"),
    "f32-one-wave": ("F32", 65, {"kernel": "one-wave"}, "bell", r"demod_fused_kernel"),
    # two streams on different tone pairs: the kernels' per-stream instantiations (as tests/test_gpu_parity.py's "-per-stream")
    "f32-seven-wave-per-stream": ("F32", 2, {"kernel": "seven-wave", "blk_resets": 1}, "two-tone-pairs", r"demod_blk6_kernel<\w+, \d+, false>"),
    "f32-four-wave-per-stream": ("F32", 2, {"kernel": "four-wave", "blk_resets": 1}, "two-tone-pairs", r"demod_blk_kernel_r\w*<\w+, false\b"),
    # 32 pattern bits (the golden set's d_preamble_AA_sfd_D5): wide registers, the fp32 generic kernel
    "f32-generic": ("F32", 65, {}, "wide-pattern", r"demod_kernel<float"),
    "f64-one-wave": ("F64", 65, {"exact_waves": 1}, "bell", r"demod_kernel<double"),
    "f64-two-waves": ("F64", 65, {"exact_waves": 2}, "bell", r"two waves"),
}
ENTRIES = ("float-device", "mulaw-frames")


@pytest.fixture(scope="module")
def wm():
    import __graft_entry__ as ge
    ge.build()
    import webaudio_modem_amd as wm
    return wm


def configs(kind, S):
    if kind == "two-tone-pairs":
        return [dict(BELL, markFrequency=BELL["markFrequency"] + 30 * s, spaceFrequency=BELL["spaceFrequency"] + 30 * s) for s in range(S)]
    if kind == "wide-pattern":
        return dict(preamblePattern=[0xAA, 0xAA, 0xAA], sfdPattern=[0xD5])      # (on the default tone pair, as the golden set has it)
    return dict(BELL)


def schedule(total):
    """[(length, calls)]: every length REPS times, then 128 to the end of `total` samples"""
    used = REPS * sum(LENGTHS)
    assert total > used and (total - used) % 128 == 0 and (total - used) // 128 >= REPS
    return [(n, REPS) for n in LENGTHS] + [(128, (total - used) // 128)]


_STIMULI = {}


def stimulus(kind, S):
    """(xq, xf, frame_len): mu-law samples [S, N] and the floats they decode to -- what both entry points take, so that one oracle
    run serves both.  Each stream: two frames of a 3-byte payload at 0.9 of full scale in light noise, the first behind
    the stream's own lead (anywhere in the first 1600 samples: during every schedule entry some streams are inside a frame and
    some in near-silence, taking 'eod' resets), each followed by GAP samples of near-silence.  Made once per kind and left unchanged."""
    if (kind, S) not in _STIMULI:
        from oracle import pyoracle as po
        cfgs = configs(kind, S)
        per_stream = isinstance(cfgs, list)
        rng = np.random.default_rng(0x6A9F + S)
        payloads = [b"abc", b"Hi!", b"xyz"]       # (text: the reference itself loses some frames whose first byte has its top bit set)
        sigs = [[np.asarray(po.OracleCore(c).modulate(p), np.float32) for p in payloads] for c in (cfgs if per_stream else [cfgs])]
        L = max(len(f) for row in sigs for f in row)
        need = 1600 + 2 * (L + GAP)
        used = REPS * sum(LENGTHS)
        N = used + 128 * max(REPS, -(-(need - used) // 128))
        x = (rng.standard_normal((S, N)) * 0.004).astype(np.float32)
        for s in range(S):
            row = sigs[s if per_stream else 0]
            at = (s * 37) % 1600
            for k in range(2):
                f = row[(s + k) % 3]
                x[s, at:at + len(f)] += np.float32(0.9) * f
                at += len(f) + GAP
        xq = sr.quantise(x, "mulaw")
        xf = sr.decode(xq, "mulaw")
        xq.setflags(write=False)
        xf.setflags(write=False)
        _STIMULI[kind, S] = (xq, xf, L)
    return _STIMULI[kind, S]


def tx_payloads(S):
    """one byte per stream: the modulation completes, and clears the RX ring, early in the run"""
    return [bytes([(0x5A + s) & 0xFF]) for s in range(S)]


_ORACLE = {}


def oracle(kind, S, tx):
    """(drained bytes per stream, 'eod' count per stream) of S reference processors on the stimulus, cut as schedule() cuts it;
    tx: a modulation is pending from the start, and its completion clears the RX ring (fsk-processor.ts:228-235).  Once per
    (kind, S, tx)."""
    if (kind, S, tx) not in _ORACLE:
        from oracle import next_oracle as no
        from oracle import pyoracle as po
        _, xf, _ = stimulus(kind, S)
        cfgs = configs(kind, S)
        rows, eods = [], []
        for s in range(S):
            cfg = cfgs[s] if isinstance(cfgs, list) else cfgs
            got, eod = po.OracleCore(cfg).demodulate(xf[s].copy())
            eods.append(int(eod))
            if tx:
                o = no.ProcessorOracle(po.OracleCore(cfg), rx_capacity=1024)
                o.modulate(tx_payloads(S)[s])
                t = 0
                for n, calls in schedule(xf.shape[1]):
                    for _ in range(calls):
                        o.process(xf[s, t:t + n], n)
                        t += n
                assert o.pending is None and o.completed == 1
                got = o.demodulate()
            rows.append(bytes(got))
        _ORACLE[kind, S, tx] = (rows, eods)
    return _ORACLE[kind, S, tx]


class KeyModel:
    """What of run_quantum's key the host advances from call to call (engine_launch_key: the decimator parity, the amplitude
    ring's position mod 4, the fp32 generic kernel's open pair, an fp64 engine's sample count mod 32; note_call) for a lock-step
    engine.  A call replays when its key is the key of the call before it."""

    def __init__(self, f64, generic):
        self.f64, self.generic = f64, generic
        self.parity = self.pushes = self.total = 0
        self.gen_odd = False
        self.last = None

    def call(self, n):
        key = (n, self.parity, self.pushes & 3, self.gen_odd, self.total & 31 if self.f64 else 0)
        replay = key == self.last
        self.last = key
        self.pushes += (self.parity + n) >> 1
        self.parity = (self.parity + n) & 1
        self.total += n
        if self.generic and not self.f64:
            self.gen_odd = self.parity != 0
        return replay


def twins(wm, path, rx_capacity=1024):
    precision, S, options, kind, _ = PATHS[path]
    cfgs = configs(kind, S)
    engs = [wm.FSKEngine(S, cfgs, precision=getattr(wm, "PRECISION_" + precision), options=options) for _ in range(2)]
    procs = [wm.FSKProcessorBatch(e, rx_capacity=rx_capacity, use_graph=g) for e, g in zip(engs, (False, True))]
    return engs, procs


def same_state(procs):
    a, b = (p.snapshot() for p in procs)
    return a.processor == b.processor and a.engine == b.engine


class FloatDevice:
    """the float form on device buffers and a HIP stream of the caller's: fskhip_processor_process_device"""

    PITCH = 160

    def __init__(self, eng, proc):
        from hip_caller import Caller
        self.c, self.proc, self.S = Caller(eng), proc, eng.n_streams
        self.d_in, self.d_out = self.c.malloc(self.S * self.PITCH * 4), self.c.malloc(self.S * self.PITCH * 4)
        self.h = np.zeros((self.S, self.PITCH), np.float32)

    def quantum(self, xq, xf, n_out):
        n = xf.shape[1]
        self.h[:, :n] = xf
        self.c.upload(self.d_in, self.h)
        self.proc.process_device(self.d_in, n, self.PITCH, self.d_out if n_out else None, n_out, self.PITCH, stream=self.c.stream)
        self.c.sync()
        if not n_out:
            return b""
        out = self.c.download(self.d_out, np.empty((self.S, self.PITCH), np.float32))
        return out[:, :n_out].tobytes()

    def close(self):
        self.c.close()


class MulawFrames:
    """mu-law interleaved frames in and out through the host form: fskhip_processor_process_fmt_host"""

    def __init__(self, eng, proc):
        self.proc = proc

    def quantum(self, xq, xf, n_out):
        out = self.proc.process_samples(np.ascontiguousarray(xq.T), "mulaw", "sample", n_out, "mulaw", "sample")
        return b"" if out is None else out.tobytes()

    def close(self):
        pass


def family(name):
    """a kernel name without its template arguments, the four-wave kernel's two forms taken as one"""
    return name.split("<")[0].replace("demod_blk_kernel_r", "demod_blk_kernel")


CASES = [(p, e, tx) for p in PATHS for e in ENTRIES for tx in (False, True)]


@pytest.mark.parametrize("path,entry,tx", CASES, ids=["%s-%s-%s" % (p, e, "tx" if tx else "rx") for p, e, tx in CASES])
def test_replayed_quanta_are_the_plain_launches(wm, path, entry, tx):
    """Without the fp64 anchor in the launch key (measured on an MI355X) every f64-* case fails at the second call of the 48-sample
    entry, its first replay behind a capture that held another anchor: the states differ, the bytes do not.  The entries of 100,
    37, 1 and 20 samples capture afresh on every call with or without it (the ring's position or the parity moves), so they pass
    either way; 16 moves the anchor like 48."""
    precision, S, options, kind, kernel = PATHS[path]
    xq, xf, frame_len = stimulus(kind, S)
    want_rows, want_eod = oracle(kind, S, tx)
    # (the stimulus: every stream decodes a frame and takes 'eod' resets; on the Bell-202 pair both frames arrive)
    assert min(want_eod) >= 2 and all(len(r) >= (1 if tx else 3 if kind == "wide-pattern" else 6) for r in want_rows), (want_eod[:8], want_rows[:4])
    engs, procs = twins(wm, path)
    sides = [(FloatDevice if entry == "float-device" else MulawFrames)(e, p) for e, p in zip(engs, procs)]
    if tx:
        for p in procs:
            p.modulate(tx_payloads(S))
        assert int(max(procs[0].tx_state()["totalSamples"])) < xf.shape[1] - 4 * 128    # it completes well inside the run
    model = KeyModel(precision == "F64", kind == "wide-pattern")
    t = 0
    for n, calls in schedule(xf.shape[1]):
        before = procs[1].graph_stats()
        want_replays = 0
        for k in range(calls):
            outs = [side.quantum(xq[:, t:t + n], xf[:, t:t + n], n if tx else 0) for side in sides]
            assert outs[0] == outs[1], (n, k, t)
            assert same_state(procs), (n, k, t)
            want_replays += model.call(n)
            t += n
            if n >= 128:
                names = [e.last_kernel() for e in engs]
                assert re.search(kernel, names[1]), (n, k, names)
                assert family(names[0]) == family(names[1]) and (path == "f32-auto" or names[0] == names[1]), (n, k, names)
        captures, replays = (a - b for a, b in zip(procs[1].graph_stats(), before))
        assert captures + replays == calls, (n, captures, replays)
        if n % 32 == 0:
            assert want_replays == calls - 1, (n, want_replays)                # the matrix itself: such an entry is carried by replays
        if path == "f32-auto":
            # ("blk_resets" = auto looks at the tile statistics between calls and may change kernels, which captures afresh)
            assert replays <= want_replays and (want_replays == 0 or replays >= 1), (n, replays, want_replays)
        else:
            assert replays == want_replays, (n, replays, want_replays)
    assert t == xf.shape[1]
    assert procs[0].graph_stats() == (0, 0)
    if tx:
        st = [p.tx_state() for p in procs]
        assert not st[1]["pendingModulation"].any() and list(st[0]["completed"]) == list(st[1]["completed"]) == [1] * S
    eods = [[e.get_status(s)["eodCount"] for s in range(S)] for e in engs]
    assert eods[0] == eods[1] == want_eod
    rows = [p.demodulate() for p in procs]
    assert rows[0] == rows[1] == want_rows
    if precision == "F64":
        # the reference's sample-serial order: one call over the whole input leaves every state word as the replayed quanta did
        one = wm.FSKEngine(S, configs(kind, S), precision=wm.PRECISION_F64)
        one_rows, one_eod = one.demodulate_data(np.array(xf))
        assert [int(v) for v in one_eod] == want_eod and (tx or [bytes(r) for r in one_rows] == want_rows)
        for s in range(S):
            (ra, ia), (rb, ib) = engs[1].debug_state(s), one.debug_state(s)
            assert np.array_equal(np.asarray(ra).view(np.uint64), np.asarray(rb).view(np.uint64)) and ia == ib, s
        one.close()
    for x in sides + procs + engs:
        x.close()


@pytest.mark.parametrize("precision,name,value", (("F64", "exact_waves", 2), ("F32", "kernel", "one-wave")))
def test_an_option_cannot_change_under_a_capture(wm, precision, name, value):
    """What chooses a launch besides the key's state -- "exact_waves" on fp64 (plan_launches, split2), "kernel" on fp32 -- cannot
    move under a captured quantum: fskhip_set_option refuses an engine that has demodulated, and a replayed call counts
    (note_call).  Tried on both twins after the second replay: both refuse, last_kernel and the state stay equal, and the replays
    go on."""
    S = 65
    xq, xf, _ = stimulus("bell", S)
    engs = [wm.FSKEngine(S, dict(BELL), precision=getattr(wm, "PRECISION_" + precision)) for _ in range(2)]
    procs = [wm.FSKProcessorBatch(e, use_graph=g) for e, g in zip(engs, (False, True))]
    for k in range(6):
        for p in procs:
            p.process(xf[:, 128 * k:128 * (k + 1)])
        assert same_state(procs), k
        if k == 2:
            assert procs[1].graph_stats() == (1, 2)
            for e in engs:
                with pytest.raises(wm.FskHipError) as ei:
                    e.set_option(name, value)
                assert ei.value.code == -1 and "has demodulated already" in str(ei.value)
            assert same_state(procs)
        assert engs[0].last_kernel() == engs[1].last_kernel() != "", k
    assert procs[1].graph_stats() == (1, 5)
    assert procs[0].demodulate() == procs[1].demodulate()
    for x in procs + engs:
        x.close()


def test_rate_quanta_run_plainly_whatever_the_flag_says(wm):
    """process_samples_at launches plainly (the resamplers' history buffers change places from call to call): with use_graph nothing
    is captured and nothing replayed"""
    S = 65
    engs, procs = twins(wm, "f32-auto")
    ups, dns = [wm.Upsampler(6, S) for _ in range(2)], [wm.Downsampler(6, S) for _ in range(2)]
    for p in procs:
        p.modulate(tx_payloads(S))
    rng = np.random.default_rng(5)
    for k in range(4):
        x = rng.integers(0, 256, (32, S)).astype(np.uint8)
        outs = [p.process_samples_at(x, upsampler=u, n_out=32, downsampler=d) for p, u, d in zip(procs, ups, dns)]
        assert outs[0].tobytes() == outs[1].tobytes(), k
        assert same_state(procs), k
    assert procs[1].graph_stats() == (0, 0)
    for x in ups + dns + procs + engs:
        x.close()
