"""Stream snapshots on the GPU (fskhip_snapshot_streams / fskhip_restore_streams, include/fskhip.h): a host-side image of a set
of streams that a fresh engine continues from under the remap's contract.

The bar is the remap tests' own (tests/test_gpu_remap.py, whose construction this file reuses): against a CONTROL engine that
demodulates the whole input uninterrupted, every continued stream is the control's stream bit for bit after every later call --
bytes, per-call 'eod', status, every carried state word -- and a lock-step fp32 engine stays on its whole-tile kernels.  What
new streams, odd cuts and fractional ring capacities do is pinned by "restore == remap": a destination restored from
src.snapshot() and one made by src.remapped() with the same map are indistinguishable, word for word and call for call."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_remap as R
from conftest import golden_hostile

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]

VARIANTS, S_SRC, N = R.VARIANTS, R.S_SRC, R.N


def _wm():
    import webaudio_modem_amd as wm
    return wm


def _prec(prec):
    wm = _wm()
    return wm.PRECISION_F64 if prec else wm.PRECISION_F32


def _all_states(eng):
    return [R._state(eng, s) for s in range(eng.n_streams)]


def _same_engines(a, b):
    """every stream's state words and status, a against b"""
    assert a.n_streams == b.n_streams
    for s in range(a.n_streams):
        assert R._same_state(R._state(a, s), R._state(b, s)), s
        assert a.get_status(s) == b.get_status(s), s


# ---- 1. round trip through bytes ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cut_name", ["even", "postreset"])
@pytest.mark.parametrize("kind", ["uniform", "per-stream"])
@pytest.mark.parametrize("vname,prec,opts", VARIANTS)
def test_snapshot_round_trip_through_bytes(vname, prec, opts, kind, cut_name):
    wm = _wm()
    precision = _prec(prec)
    x = R._signals(R._cfgs(kind, S_SRC), S_SRC, N, seed=11)
    cut = 4096 if cut_name == "even" else R._post_reset_cut(kind, x)

    def upto_cut():
        e = wm.FSKEngine(S_SRC, R._cfgs(kind, S_SRC), precision=precision, options=opts or None)
        for a, b in ((0, 1000), (1000, cut)):
            e.demodulate_data(x[:, a:b])
        return e

    src = upto_cut()
    blob = bytes(src.snapshot())              # nothing but bytes survives the source
    src.close()
    del src
    info = wm.snapshot_info(blob)
    assert info["n_streams"] == S_SRC and info["precision"] == precision and info["per_stream_configs"] == (kind != "uniform")
    rest = N - cut
    m = np.arange(S_SRC, dtype=np.int64)
    for chunks in ([rest], [rest // 3 + (rest // 3) % 2, rest - (rest // 3 + (rest // 3) % 2)], [64, 1000, 2, rest - 1066]):
        ctrl = upto_cut()
        if cut_name == "postreset" and vname == "f32-four-wave":
            zr = [R._state(ctrl, s)[1][R.wm_int_index("zr_dph")] for s in range(S_SRC)]
            assert min(zr) < R.K_HAND_PAIRS    # some stream is inside the span after its reset
        dst = wm.FSKEngine.from_snapshot(blob, options=opts or None)
        assert dst.n_streams == S_SRC and dst.precision == precision
        _same_engines(dst, ctrl)
        kern = R._check_calls(ctrl, dst, None, m, np.zeros(0, np.int64), x[:, cut:], None, chunks, 0)
        if not prec and vname != "f32-generic":
            c_name, d_name = max(zip(chunks, kern))[1]           # the longest call after the cut
            assert "demod_kernel<" not in d_name and "tail" not in d_name, d_name
            assert R._family(c_name) == R._family(d_name), (c_name, d_name)
        dst.close()
        ctrl.close()


# ---- 2. restore == remap ------------------------------------------------------------------------------------------------
GEOMETRIES = {
    "default": {},
    "fractional-ring": {"sampleRate": 44100},                          # capacity 1227.6: poly_u
    "wide-pattern": {"preamblePattern": [0x55, 0x55, 0x55]},           # 40 pattern bits: 64-bit polyphase registers
}


def _restore_equals_remap(precision, opts, kind, cut, base):
    wm = _wm()

    def cfgs(n, key=lambda s: s):
        if kind == "uniform":
            return dict(base)
        return [dict(base, **R._cfg(kind, key(s))) for s in range(n)]

    x = R._signals(cfgs(S_SRC), S_SRC, N, seed=13)
    src = wm.FSKEngine(S_SRC, cfgs(S_SRC), precision=precision, options=opts or None)
    for a, b in ((0, 1000), (1000, cut)):
        src.demodulate_data(x[:, a:b])
    blob = src.snapshot()
    rest = N - cut
    for n_dst, seed in ((97, 5), (200, 6)):
        m = R._maps(n_dst, seed + cut)
        fidx = np.nonzero(m < 0)[0]
        dcfg = cfgs(n_dst, key=lambda i: int(m[i]) if m[i] >= 0 else i)
        a = src.remapped(m, configs=dcfg if kind != "uniform" else None, options=opts or None)
        b = wm.FSKEngine.from_snapshot(blob, m, configs=dcfg if kind != "uniform" else None, options=opts or None)
        _same_engines(a, b)
        y = R._signals(cfgs(len(fidx), key=lambda j: int(fidx[j])), len(fidx), rest, seed=100 + seed)
        off = 0
        for c in (rest // 3 + (rest // 3) % 2 + 1, rest - 1 - (rest // 3 + (rest // 3) % 2)):
            din = np.where((m >= 0)[:, None], x[np.maximum(m, 0), cut + off:cut + off + c], 0).astype(np.float32)
            din[fidx] = y[:, off:off + c]
            ab, ae = a.demodulate_data(din)
            bb, be = b.demodulate_data(din)
            assert ab == bb and np.array_equal(ae, be)
            assert a.last_kernel() == b.last_kernel()
            _same_engines(a, b)
            off += c
        a.close()
        b.close()
    src.close()


@pytest.mark.parametrize("kind", ["uniform", "per-stream"])
@pytest.mark.parametrize("vname,prec,opts", VARIANTS)
def test_restore_is_indistinguishable_from_remap(vname, prec, opts, kind):
    _restore_equals_remap(_prec(prec), opts, kind, 4096, {})


@pytest.mark.parametrize("cut", [4097, 2050])
@pytest.mark.parametrize("kind", ["uniform", "per-stream"])
@pytest.mark.parametrize("vname,prec,opts", [VARIANTS[0], VARIANTS[1], VARIANTS[3], VARIANTS[7]])
def test_restore_is_indistinguishable_from_remap_off_the_grid(vname, prec, opts, kind, cut):
    """an odd cut (new streams take an fp32 destination out of lock step) and a cut inside a frame"""
    _restore_equals_remap(_prec(prec), opts, kind, cut, {})


@pytest.mark.parametrize("cut", [4096, 4097])
@pytest.mark.parametrize("geometry", ["fractional-ring", "wide-pattern"])
@pytest.mark.parametrize("prec", [0, 1])
def test_restore_equals_remap_on_wide_and_fractional_rings(prec, geometry, cut):
    _restore_equals_remap(_prec(prec), {}, "uniform", cut, GEOMETRIES[geometry])


@pytest.mark.parametrize("geometry", ["fractional-ring", "wide-pattern"])
@pytest.mark.parametrize("prec", [0, 1])
def test_round_trip_on_wide_and_fractional_rings(prec, geometry):
    """the 64-bit polyphase registers and their `undefined` masks travel: a restored engine against the uninterrupted control"""
    wm = _wm()
    cfg = GEOMETRIES[geometry]
    x = R._signals(cfg, S_SRC, N, seed=17)
    cut = 4096
    ctrl = wm.FSKEngine(S_SRC, cfg, precision=_prec(prec))
    src = wm.FSKEngine(S_SRC, cfg, precision=_prec(prec))
    for e in (ctrl, src):
        e.demodulate_data(x[:, :cut])
    blob = bytes(src.snapshot())
    src.close()
    sel = np.random.default_rng(3).permutation(S_SRC).astype(np.int64)[:100]
    dst = wm.FSKEngine.from_snapshot(blob, sel)
    R._check_calls(ctrl, dst, None, sel, np.zeros(0, np.int64), x[:, cut:], None, [2000, N - cut - 2000], 0)
    assert sum(ctrl.get_status(s)["syncDetections"] for s in range(S_SRC)) > S_SRC // 2
    dst.close()
    ctrl.close()


# ---- 3. selection and determinism ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["uniform", "per-stream"])
@pytest.mark.parametrize("prec", [0, 1])
def test_selection_determinism_and_what_the_image_says(prec, kind):
    wm = _wm()
    from webaudio_modem_amd import _lib
    x = R._signals(R._cfgs(kind, S_SRC), S_SRC, 4096, seed=19)
    src = wm.FSKEngine(S_SRC, R._cfgs(kind, S_SRC), precision=_prec(prec))
    src.demodulate_data(x[:, :1000])
    src.demodulate_data(x[:, 1000:])
    full = src.snapshot()
    again = src.snapshot(out=wm.pinned_empty(len(full), np.uint8))      # page-locked memory: same bytes
    assert bytes(full) == bytes(again)
    info = wm.snapshot_info(full)
    st = src.get_status(0)
    assert (info["n_streams"], info["precision"]) == (S_SRC, _prec(prec))
    assert (info["demodulationCalls"], info["totalSamplesProcessed"]) == (st["demodulationCalls"], st["totalSamplesProcessed"]) == (2, 4096)
    assert len(full) == 352 + S_SRC * info["record_bytes"] and info["record_bytes"] % 16 == 0
    for s in (0, 1, 63, 64, 129):
        want = wm.make_config(R._cfg(kind, s))[1]
        got = wm.snapshot_stream_config(full, s)
        assert got == dict(want, sampleRate=48000.0, baudRate=1200.0, markFrequency=float(want["markFrequency"]),
                           spaceFrequency=float(want["spaceFrequency"]), preFilterBandwidth=800.0), (s, got)
    sel = np.array([129, 0, 64, 64, 5, 127, 63, 1], np.int64)
    part = src.snapshot(sel)
    assert wm.snapshot_info(part)["n_streams"] == len(sel)
    cfg_sel = None if kind == "uniform" else [R._cfg(kind, int(s)) for s in sel]
    a = wm.FSKEngine.from_snapshot(part, configs=cfg_sel)                # identity over the selected records
    b = wm.FSKEngine.from_snapshot(full, sel, configs=cfg_sel)           # the selection as the map
    _same_engines(a, b)
    for i, s in enumerate(sel):
        assert R._same_state(R._state(a, i), R._state(src, int(s))), (i, s)
        assert a.get_status(i) == src.get_status(int(s))
    # the records of a selection are the full image's records: a host may move them with memcpy
    rb = info["record_bytes"]
    for i, s in enumerate(sel):
        assert bytes(part[352 + i * rb:352 + (i + 1) * rb]) == bytes(full[352 + int(s) * rb:352 + (int(s) + 1) * rb]), (i, s)
    # too small a buffer: FSKHIP_E_OVERFLOW with the size needed; out-of-range selections are named
    w = C.c_size_t(0)
    small = np.zeros(1000, np.uint8)
    rc = src._L.fskhip_snapshot_streams(src._h, None, 0, small.ctypes.data, small.nbytes, C.byref(w))
    assert rc == _lib.E_OVERFLOW and w.value == len(full) == src._L.fskhip_snapshot_bytes(src._h, S_SRC)
    bad = np.array([0, 130], np.int64)
    rc = src._L.fskhip_snapshot_streams(src._h, bad.ctypes.data, 2, full.ctypes.data, full.nbytes, C.byref(w))
    assert rc == _lib.E_INVALID and "sel[1] = 130" in src._L.fskhip_last_error().decode()
    for e in (a, b, src):
        e.close()


# ---- 4. across engines --------------------------------------------------------------------------------------------------
def _sharded_map(n_src, seed):
    rng = np.random.default_rng(seed)
    m = np.concatenate([rng.permutation(n_src)[:n_src - 30], rng.integers(0, n_src, 25), -np.ones(9, np.int64)])
    return rng.permutation(m).astype(np.int64)


def _check_sharded(devices_src, devices_dst_list, prec, opts_kind):
    wm = _wm()
    precision = _prec(prec)
    kind = opts_kind
    x = R._signals(R._cfgs(kind, S_SRC), S_SRC, N, seed=23)
    cut = 4096
    src = wm.FSKEngineSharded(S_SRC, R._cfgs(kind, S_SRC), devices=devices_src, precision=precision)
    for a, b in ((0, 1000), (1000, cut)):
        src.demodulate_data(x[:, a:b])
    rest = N - cut
    for k, devices in enumerate(devices_dst_list):
        m = _sharded_map(S_SRC, 31 + k)
        fidx = np.nonzero(m < 0)[0]
        dcfg = None if kind == "uniform" else R._cfgs(kind, len(m), key=lambda i: int(m[i]) if m[i] >= 0 else i)
        dst = src.remapped(m, configs=dcfg, devices=devices)
        assert [e.device for e in dst.engines] == list(devices) and dst.n_streams == len(m)
        ctrl = wm.FSKEngine(S_SRC, R._cfgs(kind, S_SRC), precision=precision)
        for a, b in ((0, 1000), (1000, cut)):
            ctrl.demodulate_data(x[:, a:b])
        fcfg = R._cfgs(kind, len(fidx), key=lambda j: int(fidx[j]))
        fresh = wm.FSKEngine(len(fidx), fcfg, precision=precision)
        y = R._signals(fcfg, len(fidx), rest, seed=200 + k)
        off = 0
        for c in (rest // 2, rest - rest // 2):
            din = np.where((m >= 0)[:, None], x[np.maximum(m, 0), cut + off:cut + off + c], 0).astype(np.float32)
            din[fidx] = y[:, off:off + c]
            cb, ce = ctrl.demodulate_data(x[:, cut + off:cut + off + c])
            db, de = dst.demodulate_data(din)
            fb, fe = fresh.demodulate_data(y[:, off:off + c])
            for i, s in enumerate(m):
                if s >= 0:
                    assert db[i] == cb[s] and de[i] == ce[s], (i, s)
                    assert dst.get_status(i) == ctrl.get_status(int(s)), (i, s)
                    sh, local = dst.locate(i)
                    assert R._same_state(R._state(dst.engines[sh], local), R._state(ctrl, int(s))), (i, s)
            for j, i in enumerate(fidx):
                assert db[i] == fb[j] and de[i] == fe[j], i
                a_, b_ = dst.get_status(int(i)), fresh.get_status(j)
                for key in ("silenceThreshold", "agcGain"):
                    assert a_.pop(key) == pytest.approx(b_.pop(key), rel=1e-12 if prec else 1e-5), (i, key)
                assert a_ == b_, i
            off += c
        if not prec:
            for e in dst.engines:
                assert "demod_kernel<" not in e.last_kernel(), e.last_kernel()
        for e in (dst, ctrl, fresh):
            e.close()
    # the sharded source is untouched: a snapshot of it restores into ONE engine that equals a control, too
    blob = src.snapshot()
    one = wm.FSKEngine.from_snapshot(blob, configs=None if kind == "uniform" else R._cfgs(kind, S_SRC))
    ctrl = wm.FSKEngine(S_SRC, R._cfgs(kind, S_SRC), precision=precision)
    for a, b in ((0, 1000), (1000, cut)):
        ctrl.demodulate_data(x[:, a:b])
    _same_engines(one, ctrl)
    for e in (one, ctrl, src):
        e.close()


@pytest.mark.parametrize("kind", ["uniform", "per-stream"])
@pytest.mark.parametrize("prec", [0, 1])
def test_sharded_batch_remaps_across_engines_on_one_device(prec, kind):
    _check_sharded([0, 0], ([0, 0, 0], [0]), prec, kind)


def test_sharded_batch_remaps_across_two_devices():
    from webaudio_modem_amd import _lib
    if _lib.lib().fskhip_device_count() < 2:
        pytest.skip("needs two HIP devices: this box has one (the same path runs on devices [0, 0] above)")
    _check_sharded([0, 1], ([1, 0, 1], [1]), 0, "uniform")


def test_concat_refuses_engines_with_different_histories():
    wm = _wm()
    x = R._signals({}, 8, 1088, seed=29)
    a = wm.FSKEngine(8, {}, precision=wm.PRECISION_F32)
    b = wm.FSKEngine(8, {}, precision=wm.PRECISION_F32)
    a.demodulate_data(x[:, :1024])
    b.demodulate_data(x[:, :1088])             # 64 samples more
    with pytest.raises(wm.FskHipError, match="differ in total_samples"):
        wm.snapshot_concat([a.snapshot(), b.snapshot()])
    a.demodulate_data(x[:, 1024:])             # the same samples, but in one call more
    with pytest.raises(wm.FskHipError, match="differ in calls"):
        wm.snapshot_concat([a.snapshot(), b.snapshot()])
    c = wm.FSKEngine(8, {}, precision=wm.PRECISION_F32)
    c.demodulate_data(x[:, :1088])
    both = wm.snapshot_concat([b.snapshot(), c.snapshot()])
    assert wm.snapshot_info(both)["n_streams"] == 16
    for e in (a, b, c):
        e.close()


# ---- 5. the fault flag and the signal-quality estimates travel ------------------------------------------------------------
@pytest.mark.parametrize("vname,prec,opts", [VARIANTS[0], VARIANTS[1], VARIANTS[3], VARIANTS[7]])
def test_faults_travel_with_the_stream(vname, prec, opts):
    wm = _wm()
    gh = golden_hostile()
    bad = np.asarray(gh.case_input(gh.cases["h_dflt_qnan_mid"]), np.float32)
    S, k = 8, 3
    n = ((bad.size + 2048) // 64) * 64
    x = R._signals({}, S, n, seed=21)
    x[k] = 0
    x[k, :bad.size] = bad
    cut = (int(np.nonzero(np.isnan(bad))[0][0]) // 64 + 2) * 64      # past the NaN
    ctrl = wm.FSKEngine(S, {}, precision=_prec(prec), options=opts or None)
    src = wm.FSKEngine(S, {}, precision=_prec(prec), options=opts or None)
    ctrl.demodulate_data(x[:, :cut])
    src.demodulate_data(x[:, :cut])
    assert list(np.nonzero(src.faults())[0]) == [k]
    blob = bytes(src.snapshot())
    src.close()
    keep = np.array([k, 0, k, 5, -1, 7, k], np.int64)
    d1 = wm.FSKEngine.from_snapshot(blob, keep, options=opts or None)
    assert list(np.nonzero(d1.faults())[0]) == [0, 2, 6]
    cb, ce = ctrl.demodulate_data(x[:, cut:])
    din = x[np.maximum(keep, 0), cut:].copy()
    din[4] = 0
    db, de = d1.demodulate_data(din)
    for i, s in enumerate(keep):
        if s >= 0:
            assert db[i] == cb[s] and de[i] == ce[s], (i, s)
            assert d1.get_status(i) == ctrl.get_status(int(s))
        if s == k:
            assert db[i] == b"" and de[i] == 0                       # poisoned: quiet
    assert list(np.nonzero(d1.faults())[0]) == [0, 2, 6]
    assert any(len(cb[s]) for s in (0, 5, 7))                        # the neighbours decode
    d1.close()
    ctrl.close()


def test_signal_quality_estimates_travel():
    wm = _wm()
    S = 16
    x = R._signals({}, S, N, seed=61)
    ctrl = wm.FSKEngine(S, {}, precision=wm.PRECISION_F32)
    src = wm.FSKEngine(S, {}, precision=wm.PRECISION_F32)
    for e in (ctrl, src):
        e.enable_signal_quality(True)
        e.demodulate_data(x[:, :4000])
    blob = bytes(src.snapshot())
    src.close()
    m = np.arange(S - 1, -1, -1, dtype=np.int64)
    dst = wm.FSKEngine.from_snapshot(blob, m)
    for i, s in enumerate(m):
        assert dst.get_signal_quality(i) == ctrl.get_signal_quality(int(s)), i
    ctrl.demodulate_data(x[:, 4000:])
    dst.demodulate_data(x[m, 4000:])
    for i, s in enumerate(m):
        assert dst.get_signal_quality(i) == ctrl.get_signal_quality(int(s)), i
    assert any(ctrl.get_signal_quality(s)["frames"] > 1 for s in range(S))
    dst.close()
    ctrl.close()


# ---- 6. refusals leave the destination usable ---------------------------------------------------------------------------
def test_restore_refusals_leave_dst_usable():
    wm = _wm()
    from webaudio_modem_amd import _lib
    L = _lib.lib()
    x = R._signals({}, 4, 4096, seed=41)
    src = wm.FSKEngine(4, {}, precision=wm.PRECISION_F32)
    src.demodulate_data(x[:, :2048])
    blob = src.snapshot()

    def refused(dst, b, m, n_map=None, code=_lib.E_INVALID, pattern=""):
        mm = np.ascontiguousarray(m, np.int64)
        rc = L.fskhip_restore_streams(dst._h, b.ctypes.data, b.nbytes, mm.ctypes.data, len(mm) if n_map is None else n_map)
        assert rc == code, (rc, L.fskhip_last_error())
        assert pattern in L.fskhip_last_error().decode(), L.fskhip_last_error()

    dst = wm.FSKEngine(3, [{}, {"markFrequency": 1700}, {}], precision=wm.PRECISION_F32)
    refused(dst, blob, [0, 1, 2], pattern="stream 1 differs from that of snapshot record 1")
    dst.close()
    dst = wm.FSKEngine(3, {}, precision=wm.PRECISION_F32)
    refused(dst, blob, [0, 1, 2], n_map=2, pattern="n_map")
    refused(dst, blob, [0, 4, 2], pattern="map[1] = 4, the snapshot has 4 records")
    refused(dst, blob, [0, -3, 2], pattern="map[1]")
    damaged = blob.copy()
    damaged[2000] ^= 1
    refused(dst, damaged, [0, 1, 2], pattern="checksum")
    f64 = wm.FSKEngine(3, {}, precision=wm.PRECISION_F64)
    refused(f64, blob, [0, 1, 2], pattern="precision")
    f64.close()
    for other_cfg in ({"baudRate": 300}, {"preamblePattern": [0x55, 0x55, 0x55]}, {"sampleRate": 44100}):
        other = wm.FSKEngine(3, other_cfg, precision=wm.PRECISION_F32)
        refused(other, blob, [-1, -1, -1], pattern="configurations differ")
        refused(other, blob, [0, -1, 1], pattern="configurations differ")
        other.close()
    used = wm.FSKEngine(3, {}, precision=wm.PRECISION_F32)
    used.demodulate_data(np.zeros((3, 64), np.float32))
    refused(used, blob, [0, 1, 2], pattern="demodulated")
    used.close()
    # after all of that, dst still takes options and a restore, and continues the source
    dst.set_option("kernel", "four-wave")
    dst.restore_from(blob, [2, 0, -1])
    dst.set_option("blk_resets", "1")
    ctrl = wm.FSKEngine(4, {}, precision=wm.PRECISION_F32)
    ctrl.demodulate_data(x[:, :2048])
    cb, ce = ctrl.demodulate_data(x[:, 2048:])
    inp = np.zeros((3, 2048), np.float32)
    inp[0], inp[1] = x[2, 2048:], x[0, 2048:]
    db, de = dst.demodulate_data(inp)
    assert db[0] == cb[2] and db[1] == cb[0] and de[0] == ce[2] and de[1] == ce[0]
    assert any(len(v) for v in cb)
    assert dst.get_status(2)["demodulationCalls"] == 1
    assert dst.get_status(0) == ctrl.get_status(2)
    for e in (dst, src, ctrl):
        e.close()


# ---- 7. full size, once per precision -------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [0, 1])
def test_snapshot_full_size_random_permutation(prec):
    """65 536 config-#3 streams: 0.5 s, snapshot, destroy, restore with a random permutation (nine slabs of records, every
    destination group served by several), 0.5 s more; a strided sample of 262 streams against the control"""
    wm = _wm()
    S, n, calls = 65536, 2400, 10
    cfg = dict(baudRate=1200, markFrequency=1200, spaceFrequency=2200)
    ctrl = wm.FSKEngine(S, cfg, precision=_prec(prec))
    src = wm.FSKEngine(S, cfg, precision=_prec(prec))
    pitch = ctrl.max_bytes(n)
    x = ctrl.device_malloc(S * n * 4)
    xp = ctrl.device_malloc(S * n * 4)
    bufs = [ctrl.device_malloc(S * pitch) for _ in range(2)] + [ctrl.device_malloc(S * 4) for _ in range(4)]
    out, out2, cnt, eod, cnt2, eod2 = bufs
    ctrl.synth_device(x, n, n, 100, 67001, 400, 0.1, 1.0)
    ctrl.synchronize()

    def call(eng, xx, o, c, e):
        eng.demodulate_device(xx, n, n, o, pitch, c, e)
        eng.synchronize()

    for _ in range(calls):
        call(ctrl, x, out, cnt, eod)
        call(src, x, out2, cnt2, eod2)
    blob = src.snapshot()
    src.close()
    info = wm.snapshot_info(blob)
    assert info["n_streams"] == S and info["demodulationCalls"] == calls
    perm = np.random.default_rng(5).permutation(S).astype(np.int64)
    dst = wm.FSKEngine.from_snapshot(blob, perm)
    del blob
    h = np.zeros((S, n), np.float32)           # dst stream i is fed the control's row perm[i]
    ctrl.d2h(h, x)
    ctrl.h2d(xp, h[perm])
    del h
    sample = np.arange(0, S, 251)
    assert len(sample) >= 257
    for i in sample:
        assert R._same_state(R._state(dst, int(i)), R._state(ctrl, int(perm[i]))), i

    def fetch(o, c, e):
        cc, ee = np.zeros(S, np.uint32), np.zeros(S, np.uint32)
        ctrl.d2h(cc, c)
        ctrl.d2h(ee, e)
        oo = np.zeros((S, pitch), np.uint8)
        ctrl.d2h(oo, o)
        return oo, cc, ee

    got = 0
    for _ in range(calls):
        call(ctrl, x, out, cnt, eod)
        call(dst, xp, out2, cnt2, eod2)
        co, cc, ce = fetch(out, cnt, eod)
        do, dc, de = fetch(out2, cnt2, eod2)
        for i in sample:
            s = perm[i]
            assert dc[i] == cc[s] and de[i] == ce[s], (i, s)
            assert np.array_equal(do[i, :dc[i]], co[s, :cc[s]]), (i, s)
            got += int(dc[i])
    assert got > 0
    if not prec:
        assert "demod_kernel<" not in dst.last_kernel()
    for i in sample:
        assert dst.get_status(int(i)) == ctrl.get_status(int(perm[i]))
        assert R._same_state(R._state(dst, int(i)), R._state(ctrl, int(perm[i])))
    for b in [x, xp] + bufs:
        ctrl.device_free(b)
    dst.close()
    ctrl.close()


# ---- 8. the staging pipeline's slab boundaries --------------------------------------------------------------------------------
SLAB = 8192          # fsk_stage.h kSnapSlab: records per staging slab


@pytest.mark.parametrize("kind", ["uniform", "per-stream"])
@pytest.mark.parametrize("prec", [0, 1])
def test_restore_equals_remap_across_slab_boundaries(prec, kind):
    """2 x 8 192 + 1 streams: three slabs with a last one of a single record, the smallest batch at which a slab has to wait for the
    staging buffer of the slab two before it, on the way out and on the way in.  Then a selection of exactly one slab, and one
    of no records at all (a restore of none still creates the new streams).  Each time a destination restored from the image
    and one made by src.remapped() with the same map are the same engine: image against image over every word of every
    stream, state words at the slab edges and a strided sample, and every stream's output of one more call."""
    wm = _wm()
    S, n, cut = 2 * SLAB + 1, 600, 300
    rng = np.random.default_rng(17 + prec)
    x = R._signals(R._cfgs(kind, S), S, n, seed=19, lead_max=100)
    src = wm.FSKEngine(S, R._cfgs(kind, S), precision=_prec(prec))
    src.demodulate_data(x[:, :cut])

    def check(blob, n_records, rec_map, src_map):
        """rec_map names records of the blob, src_map the same streams in src"""
        assert wm.snapshot_info(blob)["n_streams"] == n_records
        dcfg = None if kind == "uniform" else [R._cfg(kind, int(v) if v >= 0 else i) for i, v in enumerate(src_map)]
        a = src.remapped(src_map, configs=dcfg)
        b = wm.FSKEngine.from_snapshot(blob, rec_map, configs=dcfg)
        n_dst = len(src_map)
        edges = [i for i in (0, 1, SLAB - 1, SLAB, SLAB + 1, 2 * SLAB - 1, 2 * SLAB) if i < n_dst]
        sample = sorted(set(edges) | set(range(0, n_dst, 127)))
        din = np.where((src_map >= 0)[:, None], x[np.maximum(src_map, 0), cut:], 0).astype(np.float32)
        for step in range(2):
            assert np.array_equal(a.snapshot(), b.snapshot()), step
            for i in sample:
                assert R._same_state(R._state(a, i), R._state(b, i)), (step, i)
                assert a.get_status(i) == b.get_status(i), (step, i)
            if step == 0:
                (ab, ae), (bb, be) = a.demodulate_data(din), b.demodulate_data(din)
                assert ab == bb and np.array_equal(ae, be)
                assert a.last_kernel() == b.last_kernel()
        a.close()
        b.close()

    # three slabs, the last ragged: every record, shuffled, 40 slots new
    m = rng.permutation(S).astype(np.int64)
    m[rng.choice(S, 40, replace=False)] = -1
    check(src.snapshot(), S, m, m)
    # exactly one slab, out and in: a selection that reorders, restored in another order with 9 slots new
    sel = rng.permutation(S)[:SLAB].astype(np.int64)
    m = rng.permutation(SLAB).astype(np.int64)
    m[rng.choice(SLAB, 9, replace=False)] = -1
    check(src.snapshot(sel), SLAB, m, np.where(m >= 0, sel[np.maximum(m, 0)], -1))
    # no records: new streams only
    m = -np.ones(70, np.int64)
    check(src.snapshot([]), 0, m, m)
    src.close()
