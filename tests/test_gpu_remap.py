"""Stream remapping on the GPU (fskhip_remap_streams, include/fskhip.h): stream i of a new engine continues stream map[i] of a live
one exactly as if that FSKCore had been moved, or starts as a new FSKCore where map[i] = -1.

The bar, against a CONTROL engine that demodulates the whole input without a remap:
  * every continued stream equals the control's stream map[i] bit for bit after the cut -- bytes, per-call 'eod' counts, status and
    every carried state word (fskhip_debug_state) after each later call;
  * every new stream equals a freshly created engine fed the same samples -- bytes, 'eod', status counters; state words too on fp64
    where the source has taken a multiple of 32 samples (the NCO phasor's refresh grid) -- and the reference's own golden cases;
  * a lock-step fp32 engine stays on its whole-tile kernels after an even cut, new streams and all;
  * the fault flag follows its stream; chained remaps and a 65 536-stream batch hold the same bar; every refusal leaves the
    destination usable."""
import numpy as np
import pytest

from conftest import golden, golden_hostile

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

VARIANTS = [("f64", 1, {}), ("f32-auto", 0, {}), ("f32-seven-wave", 0, {"kernel": "seven-wave"}),
            ("f32-four-wave", 0, {"kernel": "four-wave"}), ("f32-four-wave-resets", 0, {"kernel": "four-wave", "blk_resets": 1}),
            ("f32-two-wave", 0, {"kernel": "two-wave"}), ("f32-one-wave", 0, {"kernel": "one-wave"}), ("f32-generic", 0, {"force_generic": 1})]

S_SRC = 130          # three 64-stream groups, the last one ragged
N = 9600             # about three frames per stream behind a staggered lead-in
PAYLOAD = 4
LEAD_MAX = 800
K_HAND_PAIRS = 98    # fsk_params.h kHandPairs = kZeroLagPairs + 2 + kHandLag


def _wm():
    import webaudio_modem_amd as wm
    return wm


def _cfg(kind, s):
    if kind == "uniform":
        return {}
    mark = 1650 + 20 * (s % 4)
    return {"markFrequency": mark, "spaceFrequency": mark + 200}


def _cfgs(kind, n, key=lambda s: s):
    return {} if kind == "uniform" else [_cfg(kind, key(s)) for s in range(n)]


def _signals(configs, n_streams, n, seed, lead_max=LEAD_MAX):
    """[n_streams, n] float32: back-to-back modulateData frames behind lead-ins (fskhip_synth_device), stream s with its config"""
    wm = _wm()
    eng = wm.FSKEngine(n_streams, configs, precision=wm.PRECISION_F64)
    d = eng.device_malloc(n_streams * n * 4)
    try:
        eng.synth_device(d, n, n, PAYLOAD, seed, lead_max, 0.3, 1.0)
        eng.synchronize()
        x = np.zeros((n_streams, n), np.float32)
        eng.d2h(x, d)
    finally:
        eng.device_free(d)
        eng.close()
    return x


def _state(eng, s):
    r, i = eng.debug_state(s)
    return np.array(r, np.float64), np.array(i, np.uint32)


def _same_state(a, b, skip_int=()):
    keep = np.ones(len(a[1]), bool)
    keep[list(skip_int)] = False
    return np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)) and np.array_equal(a[1][keep], b[1][keep])


def _family(name):
    return name.split("<")[0].replace("_rp", "").replace("_r", "").replace("blk6", "blk")


_CUTS = {}


def _post_reset_cut(kind, x):
    """an even cut inside the span after a reset: some stream had its 'eod' (resetState, fsk.ts:288-291) within the last 64
    samples, so its fp32 correction is still carried (zr_dph < kHandPairs)"""
    if kind not in _CUTS:
        wm = _wm()
        eng = wm.FSKEngine(S_SRC, _cfgs(kind, S_SRC), precision=wm.PRECISION_F32)
        eng.demodulate_data(x[:, :2048])
        cut = None
        for off in range(2048, N - 2048, 64):
            _, eod = eng.demodulate_data(x[:, off:off + 64])
            if eod.any():
                cut = off + 64
                break
        eng.close()
        assert cut is not None
        _CUTS[kind] = cut
    return _CUTS[kind]


def _maps(n_dst, seed):
    rng = np.random.default_rng(seed)
    if n_dst < S_SRC:        # drops 50, duplicates 10, 7 new streams
        m = np.concatenate([rng.permutation(S_SRC)[:80], rng.integers(0, S_SRC, 10), -np.ones(7, np.int64)])
    else:                    # every stream, 50 duplicates, 20 new
        m = np.concatenate([rng.permutation(S_SRC), rng.integers(0, S_SRC, n_dst - S_SRC - 20), -np.ones(20, np.int64)])
    return rng.permutation(m).astype(np.int64)


def _check_calls(ctrl, dst, fresh, m, fidx, xc, y, chunks, fresh_rel, cont_rel=0):
    """feed the control x[:, chunk], dst its rows by the map (new streams y), the fresh engine y; compare after every call.
    fresh_rel = 0: new streams equal the fresh engine's bit for bit, state words included but for the two ring positions (a new
    stream's rings sit on the engine's grid); otherwise their status reals within fresh_rel and no state words.  cont_rel: the
    same for the continued streams (0 = bit for bit)"""
    grid = (wm_int_index("poly_phase"), wm_int_index("amp_pos"))
    off = 0
    kernels = []
    for c in chunks:
        xin = xc[:, off:off + c]
        din = np.where((m >= 0)[:, None], xc[np.maximum(m, 0), off:off + c], 0).astype(np.float32)
        if len(fidx):
            din[fidx] = y[:, off:off + c]
        cb, ce = ctrl.demodulate_data(xin)
        db, de = dst.demodulate_data(din)
        kernels.append((ctrl.last_kernel(), dst.last_kernel()))
        fb, fe = fresh.demodulate_data(y[:, off:off + c]) if fresh is not None else ([], [])
        cstate = {}
        for i, src in enumerate(m):
            if src >= 0:
                assert db[i] == cb[src], (i, src, db[i], cb[src])
                assert de[i] == ce[src], (i, src)
                a, b = dst.get_status(i), ctrl.get_status(int(src))
                if cont_rel:
                    for k in ("silenceThreshold", "agcGain"):
                        assert a.pop(k) == pytest.approx(b.pop(k), rel=cont_rel), (i, k)
                assert a == b, (i, src, a, b)
                if not cont_rel:
                    if src not in cstate:
                        cstate[src] = _state(ctrl, int(src))
                    assert _same_state(_state(dst, i), cstate[src]), (i, src)
        for j, i in enumerate(fidx):
            assert db[i] == fb[j], (i, db[i], fb[j])
            assert de[i] == fe[j], i
            a, b = dst.get_status(int(i)), fresh.get_status(j)
            if fresh_rel:
                for k in ("silenceThreshold", "agcGain"):
                    assert a.pop(k) == pytest.approx(b.pop(k), rel=fresh_rel), (i, k)
            assert a == b, (i, a, b)
            if not fresh_rel:
                assert _same_state(_state(dst, int(i)), _state(fresh, j), grid), i
        off += c
    return kernels


@pytest.mark.parametrize("cut_name", ["even", "odd", "midframe", "postreset"])
@pytest.mark.parametrize("kind", ["uniform", "per-stream"])
@pytest.mark.parametrize("vname,prec,opts", VARIANTS)
def test_remap_continues_and_starts_streams(vname, prec, opts, kind, cut_name):
    wm = _wm()
    precision = wm.PRECISION_F64 if prec else wm.PRECISION_F32
    x = _signals(_cfgs(kind, S_SRC), S_SRC, N, seed=11)
    cut = {"even": 4096, "odd": 4097, "midframe": 2050}.get(cut_name) or _post_reset_cut(kind, x)

    def upto_cut():
        e = wm.FSKEngine(S_SRC, _cfgs(kind, S_SRC), precision=precision, options=opts or None)
        for a, b in ((0, 1000), (1000, cut)):     # two calls up to the cut
            e.demodulate_data(x[:, a:b])
        return e

    src = upto_cut()
    rest = N - cut
    chunks = [rest // 3 + (rest // 3) % 2, rest - (rest // 3 + (rest // 3) % 2)]
    for n_dst, seed in ((97, 5), (200, 6)):
        ctrl = upto_cut()                          # the control of this destination: the whole input, no remap
        if cut_name == "postreset" and vname == "f32-four-wave":
            zr = [_state(ctrl, s)[1][wm_int_index("zr_dph")] for s in range(S_SRC)]
            assert min(zr) < K_HAND_PAIRS          # some stream is inside the span after its reset
        m = _maps(n_dst, seed + cut)
        fidx = np.nonzero(m < 0)[0]
        dcfg = _cfgs(kind, n_dst, key=lambda i: int(m[i]) if m[i] >= 0 else i)
        dst = src.remapped(m, configs=dcfg if kind != "uniform" else None, options=opts or None)
        fcfg = _cfgs(kind, len(fidx), key=lambda j: int(fidx[j]))
        fresh = wm.FSKEngine(len(fidx), fcfg, precision=precision, options=opts or None)
        y = _signals(fcfg, len(fidx), rest, seed=100 + seed)
        # new streams: state words bit for bit on fp64 where src has taken a multiple of 32 samples (the NCO phasor's grid);
        # elsewhere bytes, 'eod' and status counters exact, the status reals to the precision's rounding (include/fskhip.h)
        fresh_rel = (1e-12 if cut % 32 else 0) if prec else 1e-5
        # an odd cut with new streams takes a fp32 engine out of lock step (include/fskhip.h): its whole-tile kernels give way to the
        # per-sample generic kernel, whose fp32 rounding differs from theirs -- the continued streams then hold the same bar
        cont_rel = 1e-5 if (not prec and cut % 2 and vname != "f32-generic") else 0
        kern = _check_calls(ctrl, dst, fresh, m, fidx, x[:, cut:], y, chunks, fresh_rel, cont_rel)
        if not prec and vname != "f32-generic" and cut % 2 == 0:
            c_name, d_name = kern[1]                     # the long call after the cut
            assert "demod_kernel<" not in d_name and "tail" not in d_name, d_name
            assert _family(c_name) == _family(d_name), (c_name, d_name)
        for e in (dst, fresh, ctrl):
            e.close()
    # the source is untouched and usable: it goes on like the control from the cut
    c2 = wm.FSKEngine(S_SRC, _cfgs(kind, S_SRC), precision=precision, options=opts or None)
    for a, b in ((0, 1000), (1000, cut), (cut, N)):
        cb, ce = c2.demodulate_data(x[:, a:b])
    sb, se = src.demodulate_data(x[:, cut:])
    assert sb == cb and np.array_equal(se, ce)
    c2.close()
    src.close()


def wm_int_index(name):
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import state_fields
    return state_fields.INT.index(name)


@pytest.mark.parametrize("vname,prec,opts", [VARIANTS[0], VARIANTS[1], VARIANTS[7]])
def test_remap_new_streams_match_golden_reference_cases(vname, prec, opts):
    """new streams of a remapped engine decode the reference's own captures like a fresh engine (fp64: the reference's numbers)"""
    wm = _wm()
    g = golden()
    cases = [c for c in g.manifest["cases"] if c.get("kind") == "demod" and c["config"] == {} and not c["chunk"]]
    by_len = {}
    for c in cases:
        by_len.setdefault(int(g.case_input(c).size), []).append(c)
    L, group = max(by_len.items(), key=lambda kv: len(kv[1]))
    x = _signals({}, 70, 4096, seed=3)
    src = wm.FSKEngine(70, {}, precision=wm.PRECISION_F64 if prec else wm.PRECISION_F32, options=opts or None)
    src.demodulate_data(x)
    m = np.array([5, -1, 69, -1, 0, -1] + [-1] * (len(group) - 3), np.int64)
    dst = src.remapped(m, options=opts or None)
    fidx = np.nonzero(m < 0)[0]
    inp = np.zeros((len(m), L), np.float32)
    for j, i in enumerate(fidx):
        inp[i] = g.case_input(group[j % len(group)])
    out, eod = dst.demodulate_data(inp)
    for j, i in enumerate(fidx):
        c = group[j % len(group)]
        assert list(out[i]) == c["bytes"], (c["name"], i)
        assert int(eod[i]) == c["eod_total"]
        st = dst.get_status(int(i))
        for k in ("frameStarted", "globalSampleCounter", "receivedBitsLength", "demodulationCalls", "syncDetections",
                  "totalSamplesProcessed"):
            assert st[k] == c["status"][k], (c["name"], k, st[k], c["status"][k])
        assert st["silenceThreshold"] == pytest.approx(c["status"]["silenceThreshold"], rel=1e-12 if prec else 1e-5)
    dst.close()
    src.close()


@pytest.mark.parametrize("vname,prec,opts", [VARIANTS[0], VARIANTS[1], VARIANTS[3], VARIANTS[7]])
def test_remap_faults_follow_the_stream(vname, prec, opts):
    wm = _wm()
    gh = golden_hostile()
    c = gh.cases["h_dflt_qnan_mid"]
    bad = np.asarray(gh.case_input(c), np.float32)
    S, k = 8, 3
    n = ((bad.size + 2048) // 64) * 64
    x = _signals({}, S, n, seed=21)
    x[k] = 0
    x[k, :bad.size] = bad
    cut = (int(np.nonzero(np.isnan(bad))[0][0]) // 64 + 2) * 64      # past the NaN
    precision = wm.PRECISION_F64 if prec else wm.PRECISION_F32
    ctrl = wm.FSKEngine(S, {}, precision=precision, options=opts or None)
    src = wm.FSKEngine(S, {}, precision=precision, options=opts or None)
    ctrl.demodulate_data(x[:, :cut])
    src.demodulate_data(x[:, :cut])
    assert list(np.nonzero(src.faults())[0]) == [k]
    keep = np.array([k, 0, k, 5, -1, 7, k], np.int64)
    d1 = src.remapped(keep, options=opts or None)
    assert list(np.nonzero(d1.faults())[0]) == [0, 2, 6]
    drop = np.array([0, 1, 2, 4, 5, 6, 7], np.int64)
    d2 = src.remapped(drop, options=opts or None)
    f = np.zeros(len(drop), np.uint8)
    import ctypes as C
    nf = C.c_uint32(99)
    from webaudio_modem_amd import _lib
    _lib.check(d2._L.fskhip_get_faults(d2._h, f.ctypes.data, C.byref(nf)))
    assert nf.value == 0
    cb, ce = ctrl.demodulate_data(x[:, cut:])
    db, de = d2.demodulate_data(x[drop, cut:])
    for i, s in enumerate(drop):
        assert db[i] == cb[s] and de[i] == ce[s]
        assert d2.get_status(i) == ctrl.get_status(int(s))
    for e in (ctrl, src, d1, d2):
        e.close()


@pytest.mark.parametrize("vname,prec,opts", [VARIANTS[0], VARIANTS[1], VARIANTS[3], VARIANTS[6]])
def test_remap_chains(vname, prec, opts):
    """three successive remaps with random maps (permutations, duplicates, drops) still match the control"""
    wm = _wm()
    precision = wm.PRECISION_F64 if prec else wm.PRECISION_F32
    x = _signals({}, S_SRC, N, seed=31)
    ctrl = wm.FSKEngine(S_SRC, {}, precision=precision, options=opts or None)
    eng = wm.FSKEngine(S_SRC, {}, precision=precision, options=opts or None)
    rng = np.random.default_rng(7)
    who = np.arange(S_SRC)                    # control stream behind each stream of `eng`
    bounds = [0, 1500, 3001, 5200, N]
    cb = None
    for step in range(4):
        a, b = bounds[step], bounds[step + 1]
        cb, ce = ctrl.demodulate_data(x[:, a:b])
        db, de = eng.demodulate_data(x[who, a:b])
        for i, s in enumerate(who):
            assert db[i] == cb[s] and de[i] == ce[s], (step, i, s)
        if step < 3:
            n_new = int(rng.integers(60, 180))
            m = rng.integers(0, len(who), n_new).astype(np.int64)
            nxt = eng.remapped(m, options=opts or None)
            eng.close()
            eng, who = nxt, who[m]
    for i, s in enumerate(who):
        assert eng.get_status(i) == ctrl.get_status(int(s))
        assert _same_state(_state(eng, i), _state(ctrl, int(s)))
    eng.close()
    ctrl.close()


def test_remap_full_size_random_permutation():
    """65 536 config-#3 streams: 1 s, a random permutation, 1 s more; a strided sample of 262 streams against the control"""
    wm = _wm()
    S, n = 65536, 2400
    cfg = dict(baudRate=1200, markFrequency=1200, spaceFrequency=2200)
    ctrl = wm.FSKEngine(S, cfg, precision=wm.PRECISION_F32)
    src = wm.FSKEngine(S, cfg, precision=wm.PRECISION_F32)
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

    for _ in range(20):                       # 1 s at 48 kHz
        call(ctrl, x, out, cnt, eod)
        call(src, x, out2, cnt2, eod2)
    perm = np.random.default_rng(5).permutation(S).astype(np.int64)
    dst = src.remapped(perm)
    src.close()
    h = np.zeros((S, n), np.float32)           # dst stream i is fed the control's row perm[i]
    ctrl.d2h(h, x)
    ctrl.h2d(xp, h[perm])
    del h
    sample = np.arange(0, S, 251)
    assert len(sample) >= 257

    def fetch(o, c, e):
        cc, ee = np.zeros(S, np.uint32), np.zeros(S, np.uint32)
        ctrl.d2h(cc, c)
        ctrl.d2h(ee, e)
        oo = np.zeros((S, pitch), np.uint8)
        ctrl.d2h(oo, o)
        return oo, cc, ee

    for _ in range(20):
        call(ctrl, x, out, cnt, eod)
        call(dst, xp, out2, cnt2, eod2)
        co, cc, ce = fetch(out, cnt, eod)
        do, dc, de = fetch(out2, cnt2, eod2)
        for i in sample:
            s = perm[i]
            assert dc[i] == cc[s] and de[i] == ce[s], (i, s)
            assert np.array_equal(do[i, :dc[i]], co[s, :cc[s]]), (i, s)
    assert "demod_kernel<" not in dst.last_kernel()
    for i in sample:
        assert dst.get_status(int(i)) == ctrl.get_status(int(perm[i]))
        assert _same_state(_state(dst, int(i)), _state(ctrl, int(perm[i])))
    for b in [x, xp] + bufs:
        ctrl.device_free(b)
    dst.close()
    ctrl.close()


def test_remap_refusals_leave_dst_usable():
    wm = _wm()
    from webaudio_modem_amd import _lib
    L = _lib.lib()
    x = _signals({}, 4, 4096, seed=41)
    src = wm.FSKEngine(4, {}, precision=wm.PRECISION_F32)
    src.demodulate_data(x[:, :2048])

    def refused(dst, s, m, n_map=None, code=_lib.E_INVALID, pattern=""):
        mm = np.ascontiguousarray(m, np.int64)
        rc = L.fskhip_remap_streams(dst._h, s._h, mm.ctypes.data, len(mm) if n_map is None else n_map)
        assert rc == code, (rc, L.fskhip_last_error())
        assert pattern in L.fskhip_last_error().decode(), L.fskhip_last_error()

    dst = wm.FSKEngine(3, [{}, {"markFrequency": 1700}, {}], precision=wm.PRECISION_F32)
    refused(dst, src, [0, 1, 2], pattern="stream 1")                       # config mismatch, named by index
    dst.close()
    dst = wm.FSKEngine(3, {}, precision=wm.PRECISION_F32)
    refused(dst, src, [0, 1, 2], n_map=2, pattern="n_map")                  # bad n_map
    refused(dst, src, [0, 4, 2], pattern="map[1]")                          # index beyond the source
    refused(dst, src, [0, -3, 2], pattern="map[1]")
    refused(dst, dst, [0, 1, 2], pattern="dst is src")
    f64 = wm.FSKEngine(3, {}, precision=wm.PRECISION_F64)
    refused(f64, src, [0, 1, 2], pattern="precision")
    f64.close()
    if L.fskhip_device_count() > 1:
        other = wm.FSKEngine(3, {}, device=1, precision=wm.PRECISION_F32)
        refused(other, src, [0, 1, 2], pattern="device")
        other.close()
    # another geometry (baud rate, preamble) is refused whatever the map -- all -1 included: dst takes over src's ring grid
    for other_cfg in ({"baudRate": 300}, {"preamblePattern": [0x55, 0x55, 0x55]}, {"sampleRate": 44100}):
        for prec_ in (wm.PRECISION_F32, wm.PRECISION_F64):
            s_ = src if prec_ == wm.PRECISION_F32 else None
            if s_ is None:
                s_ = wm.FSKEngine(4, {}, precision=prec_)
                s_.demodulate_data(x[:, :2048])
            other = wm.FSKEngine(3, other_cfg, precision=prec_)
            refused(other, s_, [-1, -1, -1], pattern="configurations differ")
            refused(other, s_, [0, -1, 1], pattern="configurations differ")
            other.close()
            if s_ is not src:
                s_.close()
    used = wm.FSKEngine(3, {}, precision=wm.PRECISION_F32)
    used.demodulate_data(np.zeros((3, 64), np.float32))
    refused(used, src, [0, 1, 2], pattern="demodulated")
    used.close()
    # after all of that, dst still takes options and a remap, and continues the source
    dst.set_option("kernel", "four-wave")
    dst.remap_from(src, [2, 0, -1])
    dst.set_option("blk_resets", "1")
    ctrl = wm.FSKEngine(4, {}, precision=wm.PRECISION_F32)
    ctrl.demodulate_data(x[:, :2048])
    cb, ce = ctrl.demodulate_data(x[:, 2048:])
    inp = np.zeros((3, 2048), np.float32)
    inp[0], inp[1] = x[2, 2048:], x[0, 2048:]
    db, de = dst.demodulate_data(inp)
    assert db[0] == cb[2] and db[1] == cb[0] and de[0] == ce[2] and de[1] == ce[0]
    assert dst.get_status(2)["demodulationCalls"] == 1
    for e in (dst, src, ctrl):
        e.close()


def test_remap_per_stream_source_into_one_shared_config():
    """regrouping a bank by tone pair: a per-stream source (stream 0 on another tone pair) into a destination of ONE shared config,
    with new streams.  The new streams join the free-running I/Q frame of the continued streams (fp32), which is not stream 0's:
    every continued stream is bit for bit a shared-config engine that ran its input from the start"""
    wm = _wm()
    S = 96
    cfgs = [_cfg("per-stream", s) for s in range(S)]       # tone pair by s % 4; stream 0 is on pair 0
    x = _signals(cfgs, S, N, seed=51)
    keep = np.array([s for s in range(S) if s % 4 == 1], np.int64)
    shared = _cfg("per-stream", 1)
    rng = np.random.default_rng(9)
    m = rng.permutation(np.concatenate([keep, keep[:5], -np.ones(11, np.int64)])).astype(np.int64)
    for prec, opts in ((0, {}), (0, {"kernel": "four-wave"}), (0, {"kernel": "one-wave"}), (1, {})):
        precision = wm.PRECISION_F64 if prec else wm.PRECISION_F32
        src = wm.FSKEngine(S, cfgs, precision=precision, options=opts or None)
        ctrl = wm.FSKEngine(len(keep), shared, precision=precision, options=opts or None)   # the kept streams, one config, no remap
        cut = 4096
        for a, b in ((0, 1000), (1000, cut)):
            src.demodulate_data(x[:, a:b])
            ctrl.demodulate_data(x[keep, a:b])
        dst = src.remapped(m, configs=shared, options=opts or None)
        fidx = np.nonzero(m < 0)[0]
        fresh = wm.FSKEngine(len(fidx), shared, precision=precision, options=opts or None)
        y = _signals(shared, len(fidx), N - cut, seed=52)
        row = {int(s): j for j, s in enumerate(keep)}
        mc = np.array([row[int(v)] if v >= 0 else -1 for v in m], np.int64)   # the map in the control's rows
        _check_calls(ctrl, dst, fresh, mc, fidx, x[keep, cut:], y, [1834, N - cut - 1834], 0 if prec else 1e-5)
        if not prec and "one-wave" not in str(opts):
            assert "demod_kernel<" not in dst.last_kernel(), dst.last_kernel()
        for e in (src, ctrl, dst, fresh):
            e.close()


def test_remap_carries_signal_quality_estimates():
    """the opt-in estimates belong to the streams: a remap carries both the accumulators and whether they run"""
    wm = _wm()
    S = 16
    x = _signals({}, S, N, seed=61)
    ctrl = wm.FSKEngine(S, {}, precision=wm.PRECISION_F32)
    src = wm.FSKEngine(S, {}, precision=wm.PRECISION_F32)
    for e in (ctrl, src):
        e.enable_signal_quality(True)
        e.demodulate_data(x[:, :4000])
    m = np.arange(S - 1, -1, -1, dtype=np.int64)
    dst = src.remapped(m)
    ctrl.demodulate_data(x[:, 4000:])
    dst.demodulate_data(x[m, 4000:])
    for i, s in enumerate(m):
        q = dst.get_signal_quality(i)
        assert q == ctrl.get_signal_quality(int(s)), (i, q)
    assert any(ctrl.get_signal_quality(s)["frames"] > 1 for s in range(S))
    for e in (ctrl, src, dst):
        e.close()
