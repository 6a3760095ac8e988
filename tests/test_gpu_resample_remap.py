"""A resampler through remap, snapshot and restore on the device (include/fskhip_next.h: fskhip_resampler_remap, _snapshot,
_restore; csrc/fsk_resample_remap.hip).  Every comparison is bit for bit, on uint32 views, so that NaN payloads and -0.0 count.  The
model is numpy's: rows of state() taken through the map, zero rows for -1."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

UP, DOWN = 0, 1
TAPS13 = [0.013, -0.021, 0.034, 0.055, -0.089, 0.144, 0.733, 0.144, -0.089, 0.055, 0.034, -0.021, 0.013]
# (factor, taps): H = 0 in both directions; 3 up, 5 down; 4 up, 12 down; the default 8 kHz <-> 48 kHz design, 16 up, 96 down
DESIGNS = {"L1-1tap": (1, [0.75]), "L2-6taps": (2, [0.11, -0.23, 0.52, 0.47, -0.19, 0.07]), "L3-13taps": (3, TAPS13), "L6-default": (6, None)}
HISTORY = {("L1-1tap", UP): 0, ("L1-1tap", DOWN): 0, ("L2-6taps", UP): 3, ("L2-6taps", DOWN): 5, ("L3-13taps", UP): 4, ("L3-13taps", DOWN): 12,
           ("L6-default", UP): 16, ("L6-default", DOWN): 96, ("L1-4096taps", UP): 4095, ("L1-4096taps", DOWN): 4095}
NAN_WORD, NEG_ZERO = 0x7FC12345, 0x80000000


@pytest.fixture(scope="module")
def wm():
    import __graft_entry__ as ge
    ge.build()
    import webaudio_modem_amd as wm
    return wm


def design(name):
    if name == "L1-4096taps":
        return 1, list(np.random.default_rng(4096).uniform(-0.01, 0.01, 4096))
    return DESIGNS[name]


def make(wm, direction, name, S, precision):
    factor, taps = design(name)
    h = (wm.Upsampler, wm.Downsampler)[direction](factor, S, taps=taps, precision=getattr(wm, "PRECISION_" + precision))
    assert h.history == HISTORY[(name, direction)]
    return h


def run(h, direction, rng, n):
    """n low rate samples per stream through h: (the input, the output)"""
    x = rng.uniform(-1, 1, (h.n_streams, n if direction == UP else n * h.factor)).astype(np.float32)
    return x, h.process(x, "f32")


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
            "thrice": np.array([S - 1, 0, S - 1, S // 3, S - 1]), "fresh": np.full(S + 1, -1)}


def model_rows(src_words, m):
    out = np.zeros((len(m), src_words.shape[1]), np.uint32)
    out[np.asarray(m) >= 0] = src_words[np.asarray(m)[np.asarray(m) >= 0]]
    return out


def check_remap(wm, direction, name, S, precision, seed):
    rng = np.random.default_rng(seed)
    for calls in (1, 2):       # an odd and an even number of process calls before: either ping-pong buffer is the current one
        h, twin = make(wm, direction, name, S, precision), make(wm, direction, name, S, precision)
        for _ in range(calls):
            x, y = run(h, direction, rng, 41)
            assert np.array_equal(words(twin.process(x, "f32")), words(y))
        src = plant(h, twin)
        assert np.array_equal(words(h.state()), src)
        for label, m in maps(S, rng).items():
            r = h.remapped(m)
            want = model_rows(src, m)
            assert type(r) is type(h) and r.n_streams == len(m) and r.history == h.history and r.taps == h.taps and r.factor == h.factor
            assert np.array_equal(words(r.state()), want), (label, calls)
            assert np.array_equal(words(h.state()), src), (label, calls)          # the source is not changed
            by_hand = make(wm, direction, name, len(m), precision)
            by_hand.set_state(want.view(np.float32))
            x, y = run(r, direction, rng, 37)
            assert np.array_equal(words(by_hand.process(x, "f32")), words(y)), (label, calls)
            assert np.array_equal(words(by_hand.state()), words(r.state())), (label, calls)
            close(r, by_hand)
        x, y = run(h, direction, rng, 37)                                          # the source, continued, is its untouched twin
        assert np.array_equal(words(twin.process(x, "f32")), words(y))
        assert np.array_equal(words(twin.state()), words(h.state()))
        close(h, twin)


GRID = [(S, name, precision, direction) for name in DESIGNS for S in (1, 63, 65, 130) for precision in ("F32", "F64") for direction in (UP, DOWN)]
GRID += [(3, "L1-4096taps", precision, direction) for precision in ("F32", "F64") for direction in (UP, DOWN)]


@pytest.mark.parametrize("S,name,precision,direction", GRID, ids=["%d-%s-%s-%s" % (c[0], c[1], c[2], ("up", "down")[c[3]]) for c in GRID])
def test_remapped_state_is_the_models_and_continues_as_a_hand_made_handle(wm, S, name, precision, direction):
    check_remap(wm, direction, name, S, precision, seed=1000 * S + 7 * direction + len(name))


def snapshot_raw(wm, h, sel, cap_less=0):
    """fskhip_resampler_snapshot through ctypes: (rc, written, the buffer) with a buffer `cap_less` bytes too small, prefilled 0x5A"""
    from webaudio_modem_amd import _lib
    L = _lib.lib()
    sel = None if sel is None else np.ascontiguousarray(sel, np.int64)
    n = h.n_streams if sel is None else len(sel)
    need = C.c_size_t(0)
    assert L.fskhip_resampler_snapshot_bytes(h._h, n, C.byref(need)) == 0
    buf = np.full(need.value, 0x5A, np.uint8)
    w = C.c_size_t(0)
    rc = L.fskhip_resampler_snapshot(h._h, None if sel is None else sel.ctypes.data, n, buf.ctypes.data, need.value - cap_less, C.byref(w))
    return rc, w.value, buf


@pytest.mark.parametrize("direction", (UP, DOWN), ids=("up", "down"))
@pytest.mark.parametrize("name", ("L2-6taps", "L6-default", "L1-1tap"))
def test_snapshot_is_canonical_and_restore_is_the_remap(wm, name, direction):
    S = 65
    rng = np.random.default_rng(77 + direction)
    a, b = make(wm, direction, name, S, "F32"), make(wm, direction, name, S, "F32")
    run(a, direction, rng, 41)                      # different call histories: one call, two calls
    run(b, direction, rng, 11)
    run(b, direction, rng, 5)
    src = plant(a, b)                               # ... and the same observable state
    assert a.snapshot() == b.snapshot()
    sel = np.array([64, 3, 3, 17, 0, 40, 64])
    assert a.snapshot(sel) == b.snapshot(sel)
    snap = a.snapshot(sel)
    info = wm.resampler_snapshot_info(snap)
    factor, taps = design(name)
    assert info == dict(n_streams=len(sel), direction=direction, factor=factor, n_taps=len(a.taps), precision=wm.PRECISION_F32, history=a.history)
    assert len(snap) == (48 + 8 * len(a.taps) + 4 * len(sel) * a.history + 15) // 16 * 16
    assert np.array_equal(np.frombuffer(snap, "<f8", len(a.taps), 48), np.asarray(a.taps))
    assert np.array_equal(np.frombuffer(snap, "<u4", len(sel) * a.history, 48 + 8 * len(a.taps)).reshape(len(sel), a.history), src[sel])
    for m in (None, np.array([6, -1, 2, 2, 0, -1, 5, 1, 3, 4]), np.array([-1, -1]), np.array([1])):
        r = type(a).from_snapshot(snap, m)
        mm = np.arange(len(sel)) if m is None else m
        via = a.remapped(np.where(mm >= 0, sel[np.maximum(mm, 0)], -1))
        assert type(r) is type(a) and r.n_streams == len(mm) and r.taps == a.taps and r.factor == a.factor and r.precision == a.precision
        assert np.array_equal(words(r.state()), words(via.state()))
        assert np.array_equal(words(r.state()), model_rows(src[sel], mm))
        x, y = run(r, direction, rng, 37)
        assert np.array_equal(words(via.process(x, "f32")), words(y))
        assert np.array_equal(words(via.state()), words(r.state()))
        close(r, via)
    assert np.array_equal(words(a.state()), src)
    # the other class refuses the image
    with pytest.raises(ValueError, match="goes"):
        (wm.Downsampler, wm.Upsampler)[direction].from_snapshot(snap)
    close(a, b)


def test_a_cap_that_is_too_small_returns_the_size_and_writes_nothing(wm):
    from webaudio_modem_amd import _lib
    h = make(wm, DOWN, "L2-6taps", 7, "F32")
    run(h, DOWN, np.random.default_rng(5), 9)
    rc, w, buf = snapshot_raw(wm, h, None, cap_less=1)
    assert rc == _lib.E_OVERFLOW and w == len(buf) == (48 + 48 + 4 * 7 * 5 + 15) // 16 * 16 and (buf == 0x5A).all()
    rc, w, buf = snapshot_raw(wm, h, [2, 2], cap_less=16)
    assert rc == _lib.E_OVERFLOW and w == len(buf) and (buf == 0x5A).all()
    rc, w, buf = snapshot_raw(wm, h, None)
    assert rc == 0 and w == len(buf) and buf.tobytes() == h.snapshot()
    # a selection out of range is refused before anything is written
    rc, w, buf = snapshot_raw(wm, h, [0, 7])
    assert rc == _lib.E_INVALID and "sel[1] = 7" in _lib.lib().fskhip_last_error().decode() and (buf == 0x5A).all()
    h.close()


def test_a_corrupted_image_and_a_bad_map_are_refused_and_leave_no_handle(wm):
    from webaudio_modem_amd import _lib
    L = _lib.lib()
    h = make(wm, UP, "L6-default", 5, "F32")
    run(h, UP, np.random.default_rng(6), 50)
    before = words(h.state()).copy()
    snap = bytearray(h.snapshot())
    snap[48 + 8 * 97 + 13] ^= 0x10
    with pytest.raises(wm.FskHipError, match="checksum"):
        wm.Upsampler.from_snapshot(bytes(snap))
    out = C.c_void_p()
    arr = np.frombuffer(bytes(snap), np.uint8)
    assert L.fskhip_resampler_restore(0, arr.ctypes.data, arr.nbytes, None, 0, C.byref(out)) == _lib.E_INVALID and out.value is None
    for bad, text in (([0, 5], "map[1] = 5, the source has 5 streams"), ([-2], "map[0] = -2"), ([], "n_map is 0")):
        with pytest.raises(wm.FskHipError, match=text.replace("[", r"\[").replace("]", r"\]")) as ei:
            h.remapped(np.array(bad, np.int64))
        assert ei.value.code == _lib.E_INVALID
    m = np.array([0, 1], np.int64)
    assert L.fskhip_resampler_remap(h._h, m.ctypes.data, 2, None) == _lib.E_INVALID and "null out" in L.fskhip_last_error().decode()
    assert L.fskhip_resampler_remap(h._h, None, 2, C.byref(out)) == _lib.E_INVALID and "null map" in L.fskhip_last_error().decode() and out.value is None
    assert np.array_equal(words(h.state()), before)
    h.close()


@pytest.mark.parametrize("S,name", ((3000, "L6-default"), (8300, "L2-6taps")), ids=("3000-default", "8300-two-slabs"))
@pytest.mark.parametrize("direction", (UP, DOWN), ids=("up", "down"))
def test_batches_beyond_one_round_of_workgroups_and_one_staging_slab(wm, S, name, direction):
    """3 000 streams of the default design: more workgroups than one per CU; 8 300 records of 3 or 5 floats: an image that crosses in
    two staging slabs, with 16-byte quads of the destination that the two slabs share"""
    rng = np.random.default_rng(S + direction)
    h = make(wm, direction, name, S, "F32")
    run(h, direction, rng, 24)
    src = plant(h)
    m = np.concatenate([rng.permutation(S), [-1, 5, -1, S - 1, 5]])
    m[rng.integers(0, S, 40)] = -1
    r = h.remapped(m)
    assert np.array_equal(words(r.state()), model_rows(src, m))
    snap = h.snapshot()
    assert np.array_equal(np.frombuffer(snap, "<u4", S * h.history, 48 + 8 * len(h.taps)).reshape(S, h.history), src)
    sel = rng.permutation(S)[:S - 7]
    at = 48 + 8 * len(h.taps)
    assert h.snapshot(sel)[at:at + 4 * len(sel) * h.history] == src[sel].tobytes()
    back = type(h).from_snapshot(snap, m)
    assert np.array_equal(words(back.state()), model_rows(src, m))
    x, y = run(r, direction, rng, 37)
    assert np.array_equal(words(back.process(x, "f32")), words(y))
    assert np.array_equal(words(back.state()), words(r.state()))
    close(h, r, back)


# ---- end to end at the trunk's rate: the 8 kHz mu-law link of test_gpu_processor_rate.py's XModem transfer, carried mid-way ----
E2E_S, E2E_Q, E2E_NEW = 65, 160, 5


class Link:
    """two FSKProcessor batches A and B joined by mu-law frames at 8 kHz, an XModemSenderBatch on A and an XModemFileReceiverBatch on B;
    every frame between them is what one process_samples_at produced and the other consumes, one quantum later"""

    def __init__(self, wm, procs, resamplers, tx, rx, a_out, b_out):
        self.wm, (self.A, self.B), self.hs, self.tx, self.rx, self.a_out, self.b_out = wm, procs, resamplers, tx, rx, a_out, b_out
        self.frames = []

    @classmethod
    def start(cls, wm, files):
        import samples_ref as sr
        S = len(files)
        engs = [wm.FSKEngine(S, {}, precision=wm.PRECISION_F32) for _ in range(2)]
        A, B = (wm.FSKProcessorBatch(e, rx_capacity=1024, clear_rx_on_tx_complete=True) for e in engs)
        hs = [wm.Upsampler(6, S), wm.Downsampler(6, S), wm.Upsampler(6, S), wm.Downsampler(6, S)]
        tx, rx = wm.XModemSenderBatch(A, 16), wm.XModemFileReceiverBatch(B, 64)
        tx.send(files)
        rx.start()
        quiet = np.full((E2E_Q, S), sr.silence("mulaw"), np.uint8)
        return cls(wm, (A, B), hs, tx, rx, quiet, quiet.copy())

    def run(self, first, last):
        a_up, a_dn, b_up, b_dn = self.hs
        for quantum in range(first, last):
            a_next = self.A.process_samples_at(self.b_out, upsampler=a_up, n_out=E2E_Q, downsampler=a_dn)
            b_next = self.B.process_samples_at(self.a_out, upsampler=b_up, n_out=E2E_Q, downsampler=b_dn)
            self.a_out, self.b_out = a_next, b_next
            self.frames.append((a_next.copy(), b_next.copy()))
            if quantum % 4 == 3:
                self.tx.poll_active()
                self.rx.poll_active()

    def carried(self, how, m):
        """the whole link under the map m: every piece through remapped ('remapped'), through snapshot / from_snapshot ('snapshot'), or
        as 'remapped' but with the four resamplers left fresh ('control')"""
        import samples_ref as sr
        wm = self.wm
        if how == "snapshot":
            A, B = (wm.FSKProcessorBatch.from_snapshot(p.snapshot(), m, clear_rx_on_tx_complete=True) for p in (self.A, self.B))
            tx, rx = wm.XModemSenderBatch.from_snapshot(A, self.tx.snapshot(), m), wm.XModemFileReceiverBatch.from_snapshot(B, self.rx.snapshot(), m)
            hs = [type(h).from_snapshot(h.snapshot(), m) for h in self.hs]
        else:
            A, B = self.A.remapped(m), self.B.remapped(m)
            tx, rx = self.tx.remapped(A, m), self.rx.remapped(B, m)
            hs = [h.remapped(m if how == "remapped" else np.full(len(m), -1)) for h in self.hs]
        frames = []
        for f in (self.a_out, self.b_out):       # the frames in flight follow their streams; a new stream's line is silent
            g = np.full((E2E_Q, len(m)), sr.silence("mulaw"), np.uint8)
            g[:, m >= 0] = f[:, m[m >= 0]]
            frames.append(g)
        return Link(wm, (A, B), hs, tx, rx, *frames)

    def close(self):
        engines = [self.A.engine, self.B.engine]
        close(self.tx, self.rx, *self.hs, self.A, self.B, *engines)


@pytest.fixture(scope="module")
def e2e_twin(wm):
    """the uninterrupted link: files of one to three packets, run until every file has arrived and a little longer"""
    rng = np.random.default_rng(0xE2E)
    files = [bytes(rng.integers(0, 256, 1 + (7 * s) % 40, dtype=np.uint8)) for s in range(E2E_S)]
    twin = Link.start(wm, files)
    done_at = None
    for q in range(0, 1200, 4):
        twin.run(q, q + 4)
        if done_at is None and twin.rx.files() == files:
            done_at = q + 4
        if done_at is not None and q + 4 >= done_at + 8:
            break
    assert done_at is not None, "the files did not arrive"
    yield twin, files, done_at
    twin.close()


@pytest.mark.parametrize("how", ("remapped", "snapshot", "control"))
def test_a_transfer_stopped_mid_way_continues_under_a_map_that_grows_the_batch(wm, e2e_twin, how):
    twin, files, done_at = e2e_twin
    n_quanta = len(twin.frames)
    cut = done_at // 2 // 4 * 4 + 1                     # mid-way, and not on a poll's quantum
    rng = np.random.default_rng(0xCA77)
    m = np.full(E2E_S + E2E_NEW, -1, np.int64)
    at = np.sort(rng.permutation(E2E_S + E2E_NEW)[:E2E_S])
    m[at] = rng.permutation(E2E_S)                      # a permutation, with five new streams between
    old = m >= 0
    first = Link.start(wm, files)
    first.run(0, cut)
    assert first.rx.files() != files                    # stopped mid-way
    assert all(np.array_equal(a, c) and np.array_equal(b, d) for (a, b), (c, d) in zip(first.frames, twin.frames))
    dut = first.carried(how, m)
    first.close()
    dut.run(cut, n_quanta)
    same = [np.array_equal(a[:, old], c[:, m[old]]) and np.array_equal(b[:, old], d[:, m[old]]) for (a, b), (c, d) in zip(dut.frames, twin.frames[cut:])]
    histories = [np.array_equal(words(h.state())[old], words(t.state())[m[old]]) for h, t in zip(dut.hs, twin.hs)]
    got = dut.rx.files()
    if how == "control":
        # fresh resamplers restart every moved stream's filters from zero: the line differs behind the seam, and this test sees it
        assert not all(same)
    else:
        assert all(same), [cut + i for i, ok in enumerate(same) if not ok][:8]
        assert [got[i] for i in np.flatnonzero(old)] == [files[j] for j in m[old]]
        assert all(histories), histories
        assert all(len(got[i]) == 0 for i in np.flatnonzero(~old))
    dut.close()
