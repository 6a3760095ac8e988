"""A rate converter through remap, snapshot and restore on the device (include/fskhip_next.h: fskhip_ratecvt_remap, _snapshot,
_restore; the rows move by csrc/fsk_resample_remap.hip's gather).  Every comparison is bit for bit, on uint32 views, so that NaN
payloads and -0.0 count.  The model is numpy's: rows of state() taken through the map, zero rows for -1; the position, one word for
all streams, is the source's.  Histories are planted by process_any over a length that leaves the handle between two period
boundaries, and once by whole periods, from position 0."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CAPTURE, PLAYBACK = 0, 1
TAPS13 = [0.013, -0.021, 0.034, 0.055, -0.089, 0.144, 0.733, 0.144, -0.089, 0.055, 0.034, -0.021, 0.013]
# name: (in_rate, out_rate, taps) -> up / down = out / in over their gcd; H = ceil((n_taps - 1) / up): 0; 3 and 4, rows off the 16-byte
# grid; 16 and 18, the two real designs (2 561 taps)
DESIGNS = {"1:1-1tap": (1, 1, [0.75]), "2:3-6taps": (3, 2, [0.11, -0.23, 0.52, 0.47, -0.19, 0.07]), "3:2-13taps": (2, 3, TAPS13),
           "44100-48000": (44100, 48000, None), "48000-44100": (48000, 44100, None)}
RATIO = {"1:1-1tap": (1, 1), "2:3-6taps": (2, 3), "3:2-13taps": (3, 2), "44100-48000": (160, 147), "48000-44100": (147, 160)}
HISTORY = {"1:1-1tap": 0, "2:3-6taps": 3, "3:2-13taps": 4, "44100-48000": 16, "48000-44100": 18}
NAN_WORD, NEG_ZERO = 0x7FC12345, 0x80000000
PLANT = 131           # inputs per stream that plant a history: a prime, so the handle stops between two period boundaries for every down > 1


@pytest.fixture(scope="module")
def wm():
    import __graft_entry__ as ge
    ge.build()
    import webaudio_modem_amd as wm
    return wm


def make(wm, direction, name, S, precision):
    in_rate, out_rate, taps = DESIGNS[name]
    h = (wm.CaptureConverter, wm.PlaybackConverter)[direction](in_rate, out_rate, S, taps=taps, precision=getattr(wm, "PRECISION_" + precision))
    assert h.history == HISTORY[name] and (h.up, h.down) == RATIO[name]
    return h


def run_any(h, direction, rng, n):
    """n inputs per stream through h.process_any: (the input, the output)"""
    x = rng.uniform(-1, 1, (h.n_streams, n)).astype(np.float32)
    return x, h.process_any(x, "f32")


def feed(h, x):
    return h.process_any(x, "f32")


def words(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def close(*things):
    for x in things:
        x.close()


def plant(*handles):
    """a NaN with a payload and a -0.0 through set_state, in the first and the last row"""
    st = words(handles[0].state()).copy()
    if st.size:
        st[0, 0] = NAN_WORD
        st[-1, -1] = NEG_ZERO if st.size > 1 else NAN_WORD
        for h in handles:
            h.set_state(st.view(np.float32))
    return st


def maps(S, rng):
    grow = np.full(2 * S + 3, -1, np.int64)
    grow[0:2 * S:2] = rng.permutation(S)
    return {"identity": np.arange(S), "reversed": np.arange(S)[::-1].copy(), "permutation": rng.permutation(S), "shrink": np.array([S // 2]), "grow": grow,
            "twice": np.array([S - 1, 0, S - 1, S // 3])}


def model_rows(src_words, m):
    out = np.zeros((len(m), src_words.shape[1]), np.uint32)
    out[np.asarray(m) >= 0] = src_words[np.asarray(m)[np.asarray(m) >= 0]]
    return out


def by_hand(wm, direction, name, precision, rows, position):
    """the carry without the library: a new handle, set_state, position"""
    h = make(wm, direction, name, len(rows), precision)
    h.set_state(rows.view(np.float32))
    h.position = position
    return h


def same_design(a, b):
    return (type(a) is type(b) and a.taps == b.taps and a.history == b.history and (a.up, a.down) == (b.up, b.down) and a.precision == b.precision
            and (a.in_rate, a.out_rate) == (b.in_rate, b.out_rate))


def continue_alike(r, hand, rng, where):
    """two further calls of 1 and 129 inputs: output, history and position bit for bit"""
    for n in (1, 129):
        x = rng.uniform(-1, 1, (r.n_streams, n)).astype(np.float32)
        assert np.array_equal(words(feed(hand, x)), words(feed(r, x))), (where, n)
        assert np.array_equal(words(hand.state()), words(r.state())) and hand.position == r.position, (where, n)


def check_remap(wm, direction, name, S, precision, seed):
    rng = np.random.default_rng(seed)
    up, down = RATIO[name]
    # 131 inputs once, 131 and 132: either ping-pong buffer is the current one, at two positions; then whole periods from position 0
    for label, lengths in (("one-call", (PLANT,)), ("two-calls", (PLANT, PLANT + 1)), ("whole-periods", (3 * down,))):
        h, twin = make(wm, direction, name, S, precision), make(wm, direction, name, S, precision)
        for n in lengths:
            x = rng.uniform(-1, 1, (S, n)).astype(np.float32)
            assert np.array_equal(words(feed(twin, x)), words(feed(h, x)))
        pos = sum(lengths) % down
        assert h.position == pos and (pos != 0 or label == "whole-periods" or down == 1)
        src = plant(h, twin)
        assert np.array_equal(words(h.state()), src)
        for mlabel, m in maps(S, rng).items():
            where = (label, mlabel)
            r = h.remapped(m)
            want = model_rows(src, m)
            assert same_design(r, h) and r.n_streams == len(m) and r.position == pos, where
            assert np.array_equal(words(r.state()), want), where
            assert np.array_equal(words(h.state()), src) and h.position == pos, where           # the source is not changed
            hand = by_hand(wm, direction, name, precision, want, pos)
            continue_alike(r, hand, rng, where)
            close(r, hand)
        x = rng.uniform(-1, 1, (S, 37)).astype(np.float32)                                      # the source, continued, is its untouched twin
        assert np.array_equal(words(feed(twin, x)), words(feed(h, x)))
        assert np.array_equal(words(twin.state()), words(h.state())) and twin.position == h.position
        close(h, twin)


# every design goes both ways: the direction names the side that carries the capture format, not up or down
GRID = [(S, name, precision, direction) for name in DESIGNS for S in (1, 63, 65, 130) for precision in ("F32", "F64") for direction in (CAPTURE, PLAYBACK)]


@pytest.mark.parametrize("S,name,precision,direction", GRID, ids=["%d-%s-%s-%s" % (c[0], c[1], c[2], ("capture", "playback")[c[3]]) for c in GRID])
def test_remapped_state_is_the_models_and_continues_as_a_hand_made_handle(wm, S, name, precision, direction):
    check_remap(wm, direction, name, S, precision, seed=1000 * S + 7 * direction + len(name))


def snapshot_raw(wm, h, sel, cap_less=0):
    """fskhip_ratecvt_snapshot through ctypes: (rc, written, the buffer) with a buffer `cap_less` bytes too small, prefilled 0x5A"""
    from webaudio_modem_amd import _lib
    L = _lib.lib()
    sel = None if sel is None else np.ascontiguousarray(sel, np.int64)
    n = h.n_streams if sel is None else len(sel)
    need = C.c_size_t(0)
    assert L.fskhip_ratecvt_snapshot_bytes(h._h, n, C.byref(need)) == 0
    buf = np.full(need.value, 0x5A, np.uint8)
    w = C.c_size_t(0)
    rc = L.fskhip_ratecvt_snapshot(h._h, None if sel is None else sel.ctypes.data, n, buf.ctypes.data, need.value - cap_less, C.byref(w))
    return rc, w.value, buf


@pytest.mark.parametrize("precision", ("F32", "F64"))
@pytest.mark.parametrize("direction", (CAPTURE, PLAYBACK), ids=("capture", "playback"))
@pytest.mark.parametrize("name", tuple(DESIGNS))
def test_snapshot_is_canonical_and_restore_is_the_remap(wm, name, direction, precision):
    S = 65
    rng = np.random.default_rng(77 + direction)
    up, down = RATIO[name]
    a, b = make(wm, direction, name, S, precision), make(wm, direction, name, S, precision)
    run_any(a, direction, rng, PLANT)               # different call histories: one call, two calls ...
    run_any(b, direction, rng, PLANT - 5)
    run_any(b, direction, rng, 5)
    src = plant(a, b)                               # ... and the same observable state
    pos = PLANT % down
    assert a.position == b.position == pos
    before = a.snapshot()
    assert before == b.snapshot()
    # a call flips which of the two buffers is current; set_state and position undo what can be observed of it
    run_any(a, direction, rng, 3)
    a.set_state(src.view(np.float32))
    a.position = pos
    assert a.snapshot() == before == b.snapshot()
    sel = np.array([64, 3, 3, 17, 0, 40, 64])
    assert a.snapshot(sel) == b.snapshot(sel)
    snap = a.snapshot(sel)
    info = wm.ratecvt_snapshot_info(snap)
    assert info == dict(n_streams=len(sel), direction=direction, up=up, down=down, n_taps=len(a.taps), precision=a.precision, history=a.history, position=pos)
    assert len(snap) == (64 + 8 * len(a.taps) + 4 * len(sel) * a.history + 15) // 16 * 16
    assert np.array_equal(np.frombuffer(snap, "<f8", len(a.taps), 64), np.asarray(a.taps))
    assert np.array_equal(np.frombuffer(snap, "<u4", len(sel) * a.history, 64 + 8 * len(a.taps)).reshape(len(sel), a.history), src[sel])
    in_rate, out_rate, _ = DESIGNS[name]
    from webaudio_modem_amd.filters import _RateConverter
    for m in (None, np.array([6, -1, 2, 2, 0, -1, 5, 1, 3, 4]), np.array([-1, -1]), np.array([1])):
        r = type(a).from_snapshot(snap, m, in_rate=in_rate, out_rate=out_rate)
        mm = np.arange(len(sel)) if m is None else m
        via = a.remapped(np.where(mm >= 0, sel[np.maximum(mm, 0)], -1))
        assert same_design(r, a) and r.n_streams == len(mm) and r.position == via.position == pos
        assert np.array_equal(words(r.state()), words(via.state()))
        assert np.array_equal(words(r.state()), model_rows(src[sel], mm))
        continue_alike(r, via, rng, m)
        close(r, via)
    # without rates the image's ratio stands in for them, and the base class picks the class from the image
    r = _RateConverter.from_snapshot(snap)
    assert type(r) is type(a) and (r.in_rate, r.out_rate, r.up, r.down) == (down, up, up, down) and r.taps == a.taps and r.position == pos
    assert np.array_equal(words(r.state()), src[sel])
    r.close()
    assert np.array_equal(words(a.state()), src) and a.position == pos
    # the other class refuses the image
    with pytest.raises(ValueError, match="not (capture|playback)"):
        (wm.PlaybackConverter, wm.CaptureConverter)[direction].from_snapshot(snap)
    close(a, b)


def test_a_cap_that_is_too_small_returns_the_size_and_writes_nothing(wm):
    from webaudio_modem_amd import _lib
    h = make(wm, PLAYBACK, "2:3-6taps", 7, "F32")
    run_any(h, PLAYBACK, np.random.default_rng(5), 10)
    rc, w, buf = snapshot_raw(wm, h, None, cap_less=1)
    assert rc == _lib.E_OVERFLOW and w == len(buf) == (64 + 48 + 4 * 7 * 3 + 15) // 16 * 16 and (buf == 0x5A).all()
    rc, w, buf = snapshot_raw(wm, h, [2, 2], cap_less=16)
    assert rc == _lib.E_OVERFLOW and w == len(buf) and (buf == 0x5A).all()
    rc, w, buf = snapshot_raw(wm, h, None)
    assert rc == 0 and w == len(buf) and buf.tobytes() == h.snapshot()
    # a selection out of range is refused before anything is written
    rc, w, buf = snapshot_raw(wm, h, [0, 7])
    assert rc == _lib.E_INVALID and "sel[1] = 7, the rate converter has 7 streams" in _lib.lib().fskhip_last_error().decode() and (buf == 0x5A).all()
    h.close()


def test_a_corrupted_image_and_a_bad_map_are_refused_and_leave_no_handle(wm):
    from webaudio_modem_amd import _lib
    L = _lib.lib()
    h = make(wm, CAPTURE, "44100-48000", 5, "F32")
    run_any(h, CAPTURE, np.random.default_rng(6), PLANT)
    before, pos = words(h.state()).copy(), h.position
    good = h.snapshot()
    snap = bytearray(good)
    snap[64 + 8 * 2561 + 13] ^= 0x10
    with pytest.raises(wm.FskHipError, match="checksum"):
        wm.CaptureConverter.from_snapshot(bytes(snap))
    out = C.c_void_p()
    arr = np.frombuffer(bytes(snap), np.uint8)
    assert L.fskhip_ratecvt_restore(0, arr.ctypes.data, arr.nbytes, None, 0, C.byref(out)) == _lib.E_INVALID and out.value is None
    for bad, text in (([0, 5], "map[1] = 5, the snapshot has 5 records"), ([-2], "map[0] = -2"), ([], "n_map is 0")):
        with pytest.raises(wm.FskHipError, match=text.replace("[", r"\[").replace("]", r"\]")) as ei:
            wm.CaptureConverter.from_snapshot(good, np.array(bad, np.int64))
        assert ei.value.code == _lib.E_INVALID
    arr = np.frombuffer(good, np.uint8)
    m = np.array([0, 5], np.int64)
    assert L.fskhip_ratecvt_restore(0, arr.ctypes.data, arr.nbytes, m.ctypes.data, 2, C.byref(out)) == _lib.E_INVALID and out.value is None
    assert L.fskhip_ratecvt_restore(0, arr.ctypes.data, arr.nbytes, m.ctypes.data, 0, C.byref(out)) == _lib.E_INVALID and out.value is None
    for bad, text in (([0, 5], "map[1] = 5, the source has 5 streams"), ([-2], "map[0] = -2"), ([], "n_map is 0")):
        with pytest.raises(wm.FskHipError, match=text.replace("[", r"\[").replace("]", r"\]")) as ei:
            h.remapped(np.array(bad, np.int64))
        assert ei.value.code == _lib.E_INVALID
    m = np.array([0, 1], np.int64)
    assert L.fskhip_ratecvt_remap(h._h, m.ctypes.data, 2, None) == _lib.E_INVALID and "null out" in L.fskhip_last_error().decode()
    assert L.fskhip_ratecvt_remap(h._h, None, 2, C.byref(out)) == _lib.E_INVALID and "null map" in L.fskhip_last_error().decode() and out.value is None
    assert L.fskhip_ratecvt_remap(h._h, m.ctypes.data, 0, C.byref(out)) == _lib.E_INVALID and "n_map is 0" in L.fskhip_last_error().decode() and out.value is None
    assert np.array_equal(words(h.state()), before) and h.position == pos
    h.close()


@pytest.mark.parametrize("S,name", ((3000, "44100-48000"), (8300, "2:3-6taps")), ids=("3000-default", "8300-two-slabs"))
@pytest.mark.parametrize("direction", (CAPTURE, PLAYBACK), ids=("capture", "playback"))
def test_batches_beyond_one_round_of_workgroups_and_one_staging_slab(wm, S, name, direction):
    """3 000 streams of the default design: more workgroups than one per CU; 8 300 records of 3 floats: an image that crosses in two
    staging slabs, with 16-byte quads of the destination that the two slabs share"""
    rng = np.random.default_rng(S + direction)
    h = make(wm, direction, name, S, "F32")
    run_any(h, direction, rng, 25)
    pos = 25 % h.down
    src = plant(h)
    m = np.concatenate([rng.permutation(S), [-1, 5, -1, S - 1, 5]])
    m[rng.integers(0, S, 40)] = -1
    r = h.remapped(m)
    assert np.array_equal(words(r.state()), model_rows(src, m)) and r.position == pos != 0
    snap = h.snapshot()
    at = 64 + 8 * len(h.taps)
    assert np.array_equal(np.frombuffer(snap, "<u4", S * h.history, at).reshape(S, h.history), src)
    sel = rng.permutation(S)[:S - 7]
    assert h.snapshot(sel)[at:at + 4 * len(sel) * h.history] == src[sel].tobytes()
    back = type(h).from_snapshot(snap, m)
    assert np.array_equal(words(back.state()), model_rows(src, m)) and back.position == pos
    continue_alike(back, r, rng, S)
    close(h, r, back)


# ---- end to end at 44.1 kHz: a frame loops back through one FSKProcessor batch in 128-frame quanta, carried mid-frame ----
E2E_S, E2E_Q, E2E_NEW = 67, 128, 5


class Loop:
    """an FSKProcessor batch whose 44.1 kHz output (s16 frames) is its next quantum's input, through a CaptureConverter and a
    PlaybackConverter: process_samples_at_any in quanta of 128 frames"""

    def __init__(self, wm, proc, cap, play, wire):
        self.wm, self.proc, self.cap, self.play, self.wire = wm, proc, cap, play, wire
        self.wires, self.modulating = [], []

    @classmethod
    def start(cls, wm, payloads):
        S = len(payloads)
        proc = wm.FSKProcessorBatch(wm.FSKEngine(S, {}, precision=wm.PRECISION_F32), rx_capacity=1024, clear_rx_on_tx_complete=False)
        proc.modulate(payloads)
        return cls(wm, proc, wm.CaptureConverter(44100, 48000, S), wm.PlaybackConverter(48000, 44100, S), np.zeros((E2E_Q, S), np.int16))

    def run(self, n):
        for _ in range(n):
            self.wire = self.proc.process_samples_at_any(self.wire, "s16", "sample", self.cap, E2E_Q, "s16", "sample", self.play)
            self.wires.append(self.wire.copy())
            self.modulating.append(int(np.count_nonzero(self.proc.tx_state()["isModulating"])))   # streams still sending

    def carried(self, how, m):
        """the whole loop under the map m: every piece through remapped ('remapped'), through snapshot / from_snapshot ('snapshot'),
        or as 'remapped' but with the two converters left fresh ('fresh')"""
        wm = self.wm
        if how == "snapshot":
            proc = wm.FSKProcessorBatch.from_snapshot(self.proc.snapshot(), m, clear_rx_on_tx_complete=False)
            cap = wm.CaptureConverter.from_snapshot(self.cap.snapshot(), m, in_rate=44100, out_rate=48000)
            play = wm.PlaybackConverter.from_snapshot(self.play.snapshot(), m, in_rate=48000, out_rate=44100)
        else:
            proc = self.proc.remapped(m)
            cap, play = (h.remapped(m if how == "remapped" else np.full(len(m), -1)) for h in (self.cap, self.play))
        wire = np.zeros((E2E_Q, len(m)), np.int16)      # the frames in flight follow their streams; a new stream's line is silent
        wire[:, m >= 0] = self.wire[:, m[m >= 0]]
        return Loop(wm, proc, cap, play, wire)

    def close(self):
        close(self.cap, self.play, self.proc, self.proc.engine)


@pytest.fixture(scope="module")
def e2e_control(wm):
    """the loop that is not carried at all: run until every frame has left and 40 quanta longer, for the converters' and the
    demodulator's delay behind the last sample"""
    rng = np.random.default_rng(0x441)
    payloads = [bytes(rng.integers(0, 256, 1 + s % 3, dtype=np.uint8)) for s in range(E2E_S)]
    control = Loop.start(wm, payloads)
    tail = 0
    while tail < 40:
        assert len(control.wires) < 600, "the frames did not end"
        control.run(1)
        tail += control.modulating[-1] == 0
    back = control.proc.demodulate()
    assert back == payloads                             # the frame sent came back across 44.1 kHz
    yield control, payloads
    control.close()


@pytest.mark.parametrize("how", ("remapped", "snapshot", "fresh"))
def test_a_frame_stopped_mid_way_continues_under_a_map_that_grows_the_batch(wm, e2e_control, how):
    control, payloads = e2e_control
    n_quanta = len(control.wires)
    cut = next(i for i, n in enumerate(control.modulating) if n < E2E_S) // 2 + 1   # mid-way through the shortest frame
    rng = np.random.default_rng(0xCA77)
    m = np.full(E2E_S + E2E_NEW, -1, np.int64)
    at = np.sort(rng.permutation(E2E_S + E2E_NEW)[:E2E_S])
    m[at] = rng.permutation(E2E_S)                      # a permutation, with five new streams between
    old = m >= 0
    first = Loop.start(wm, payloads)
    first.run(cut)
    while first.cap.position == 0 or first.play.position == 0:    # (128 frames a quantum: the handles meet a boundary once in 147 and 160)
        first.run(1)
        cut += 1
    assert first.proc.tx_state()["isModulating"].all()  # stopped mid-frame, every stream ...
    assert first.cap.position == cut * E2E_Q % 147 != 0 and first.play.position != 0   # ... and between two period boundaries, both ways
    assert all(np.array_equal(a, c) for a, c in zip(first.wires, control.wires))
    dut = first.carried(how, m)
    assert dut.cap.position == first.cap.position and dut.play.position == first.play.position
    first.close()
    dut.run(n_quanta - cut)
    same = [np.array_equal(a[:, old], c[:, m[old]]) for a, c in zip(dut.wires, control.wires[cut:])]
    got = dut.proc.demodulate()
    if how == "fresh":
        # fresh converters restart every stream's filters from zero: the line differs behind the seam, and this test sees it
        assert not all(same)
    else:
        assert all(same), [cut + i for i, ok in enumerate(same) if not ok][:8]
        assert [got[i] for i in np.flatnonzero(old)] == [payloads[j] for j in m[old]]
        assert np.array_equal(words(dut.cap.state())[old], words(control.cap.state())[m[old]]) and dut.cap.position == control.cap.position
        assert np.array_equal(words(dut.play.state())[old], words(control.play.state())[m[old]]) and dut.play.position == control.play.position
        # the new streams are idle receivers: a silent line, nothing sent, nothing decoded
        assert all(not w[:, ~old].any() for w in dut.wires)
        assert all(len(got[i]) == 0 for i in np.flatnonzero(~old))
        assert not dut.proc.tx_state()["isModulating"][~old].any()
    dut.close()
