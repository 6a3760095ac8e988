"""The compacted RX drain on the GPU (include/fskhip_next.h: fskhip_processor_rx_drain_sparse_host / _device;
FSKProcessorBatch.demodulate_sparse / demodulate_active).  Ring states are set directly: the processor image of a fresh batch is
rewritten in numpy (tests/drain_ref.py) and restored, and the expected lists, bytes and ring words afterwards come from the
same numpy state, independently of the code under test.  The shapes are those where the three launches can go wrong: a partial
wave, exactly one wave, one lane into the next, the same around a 256-stream workgroup, several workgroups, and 66 000 streams
-- 258 workgroup pairs, so the scan kernel makes a second pass, and a partial last workgroup.  At 66 000 streams the capacities
stop at 100: 1 024 takes no other path (the byte positions stay far below 2^32) and would move a 72 MB image for it."""
import ctypes as C

import numpy as np
import pytest

import drain_ref
from conftest import golden_next

pytestmark = pytest.mark.gpu

E_INVALID, E_OVERFLOW = -1, -7
DENSITIES = ("empty", "full", "one_in_500", "random30")


class Bench:
    """a fresh fp32 batch of one shape, its snapshot taken once: clones with any ring state come from it"""

    def __init__(self, n_streams, cap):
        import webaudio_modem_amd as wm
        self.wm, self.n_streams, self.cap = wm, n_streams, cap
        eng = wm.FSKEngine(n_streams, {}, precision=wm.PRECISION_F32)
        proc = wm.FSKProcessorBatch(eng, rx_capacity=cap)
        self.fresh = proc.snapshot()
        proc.close()
        eng.close()
        self.made = []

    def clone(self, rings, **kw):
        snap = self.wm.ProcessorBatchSnapshot(engine=self.fresh.engine, processor=rings.image(fresh=self.fresh.processor))
        p = self.wm.FSKProcessorBatch.from_snapshot(snap, **kw)
        self.made.append(p)
        return p

    def close(self):
        for p in self.made:
            p.close()
            p.engine.close()


@pytest.fixture
def bench():
    made = []

    def make(n_streams, cap):
        made.append(Bench(n_streams, cap))
        return made[-1]
    yield make
    for b in made:
        b.close()


def _hip_runtime():
    """the HIP runtime libfskhip.so has loaded into this process (found in the process's own map, so that it is that copy)"""
    with open("/proc/self/maps") as fh:
        paths = {line.split()[-1] for line in fh if "libamdhip64.so" in line and "/torch/" not in line}   # (not a copy some package brought)
    assert len(paths) == 1, paths
    hip = C.CDLL(paths.pop())
    hip.hipStreamCreate.argtypes, hip.hipStreamSynchronize.argtypes, hip.hipStreamDestroy.argtypes = [C.POINTER(C.c_void_p)], [C.c_void_p], [C.c_void_p]
    return hip


def check_drain(proc, fresh, rings, mask=None, min_len=1, expect_min_len=None):
    streams, offsets, data = proc.demodulate_sparse(mask=mask, min_len=min_len)
    ws, wo, wd, after = rings.drained(mask=mask, min_len=min_len if expect_min_len is None else expect_min_len)
    assert streams.dtype == np.uint32 and offsets.dtype == np.uint32 and data.dtype == np.uint8
    assert np.array_equal(streams, ws) and np.array_equal(offsets, wo) and np.array_equal(data, wd)
    assert proc.snapshot().processor == after.image(fresh=fresh)   # every ring word (and live byte) of every stream
    return after


@pytest.mark.parametrize("n_streams", [1, 63, 64, 65, 255, 256, 257, 1000, 66000])
def test_lists_bytes_and_rings_match_numpy(bench, n_streams):
    rng = np.random.default_rng(0xD7A1 + n_streams)
    if n_streams == 66000:
        cases = [(1, "full"), (16, "random30"), (16, "empty"), (100, "one_in_500")]
    else:
        cases = [(cap, d) for cap in (1, 16, 100, 1024) for d in DENSITIES]
    benches = {}
    for cap, density in cases:
        b = benches.get(cap) or benches.setdefault(cap, bench(n_streams, cap))
        rings = drain_ref.random_rings(rng, n_streams, cap, density)
        proc = b.clone(rings)
        after = check_drain(proc, b.fresh.processor, rings)
        if density == "random30":   # drained once, nothing is left; the rings stay where the first drain put them
            check_drain(proc, b.fresh.processor, after)
        b.close()
        b.made = []


@pytest.mark.parametrize("n_streams,cap", [(257, 100), (1000, 16), (70, 1024)])
def test_equals_the_dense_drain(bench, n_streams, cap):
    b = bench(n_streams, cap)
    rings = drain_ref.random_rings(np.random.default_rng(n_streams), n_streams, cap, "random30")
    sparse, dense = b.clone(rings), b.clone(rings)
    got = sparse.demodulate_active()
    want = dense.demodulate()
    assert got == {s: v for s, v in enumerate(want) if v} and len(got) > 0
    assert sparse.snapshot().processor == dense.snapshot().processor


def test_mask_and_min_len(bench):
    n_streams, cap = 300, 16
    b = bench(n_streams, cap)
    rng = np.random.default_rng(5)
    rings = drain_ref.random_rings(rng, n_streams, cap, "random30")
    fresh = b.fresh.processor
    mask = rng.random(n_streams) < 0.5
    proc = b.clone(rings)
    after = check_drain(proc, fresh, rings, mask=mask, min_len=4)     # excluded by either: all three words kept ...
    assert (after.n > 0).sum() > 10
    after = check_drain(proc, fresh, after, min_len=cap + 1)          # min_len > cap selects nothing
    assert np.array_equal(after.n, rings.drained(mask=mask, min_len=4)[3].n)
    after = check_drain(proc, fresh, after, min_len=0, expect_min_len=1)   # ... and returned by a later call; 0 behaves as 1
    assert not after.n.any()
    assert proc.demodulate_active() == {}


def test_overflow_is_atomic_and_sizes_are_reported(bench):
    n_streams, cap = 600, 100
    b = bench(n_streams, cap)
    rings = drain_ref.random_rings(np.random.default_rng(9), n_streams, cap, "random30")
    proc = b.clone(rings)
    ws, wo, wd, after = rings.drained()
    before = proc.snapshot().processor
    L, lib = proc._L, b.wm._lib
    streams, offsets, data = np.zeros(len(ws), np.uint32), np.zeros(len(ws) + 1, np.uint32), np.zeros(len(wd), np.uint8)
    na, nb = C.c_uint32(0), C.c_uint32(0)

    def call(cap_streams, cap_bytes, lists=True):
        na.value = nb.value = 0xFFFFFFFF
        return L.fskhip_processor_rx_drain_sparse_host(proc._h, None, 1, streams.ctypes.data if lists else None, offsets.ctypes.data if lists else None,
                                                       cap_streams, data.ctypes.data if lists else None, cap_bytes, C.byref(na), C.byref(nb))
    for cap_streams, cap_bytes, lists in ((len(ws) - 1, len(wd), True), (len(ws), len(wd) - 1, True), (0, 0, False)):
        assert call(cap_streams, cap_bytes, lists) == E_OVERFLOW
        assert "nothing was drained" in L.fskhip_last_error().decode()
        assert (na.value, nb.value) == (len(ws), len(wd))
        assert proc.snapshot().processor == before
    assert call(len(ws), len(wd)) == 0 and (na.value, nb.value) == (len(ws), len(wd))
    assert np.array_equal(streams, ws) and np.array_equal(offsets, wo) and np.array_equal(data, wd)
    assert proc.snapshot().processor == after.image(fresh=b.fresh.processor)
    assert call(0, 0, False) == 0 and (na.value, nb.value) == (0, 0)   # the size query of a drained batch
    with pytest.raises(lib.FskHipError, match="null streams or offsets with cap_streams 3"):
        lib.check(L.fskhip_processor_rx_drain_sparse_host(proc._h, None, 1, None, None, 3, None, 0, C.byref(na), C.byref(nb)))


def test_device_form(bench):
    n_streams, cap = 700, 100
    b = bench(n_streams, cap)
    rng = np.random.default_rng(11)
    rings = drain_ref.random_rings(rng, n_streams, cap, "random30")
    mask = (rng.random(n_streams) < 0.7).astype(np.uint8)
    ws, wo, wd, after = rings.drained(mask=mask, min_len=3)
    host, dev = b.clone(rings), b.clone(rings)
    hs, ho, hd = host.demodulate_sparse(mask=mask, min_len=3)
    L, eh = dev._L, dev.engine._h
    hip, stream = _hip_runtime(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0 and stream.value   # a stream of the caller's own, not the null stream
    sizes = {"mask": n_streams, "streams": 4 * len(ws), "offsets": 4 * (len(ws) + 1), "data": len(wd), "totals": 12}
    d = {}
    for k, nbytes in sizes.items():
        p = C.c_void_p()
        b.wm._lib.check(L.fskhip_device_malloc(eh, nbytes, C.byref(p)))
        d[k] = p
    try:
        b.wm._lib.check(L.fskhip_memcpy_h2d(eh, d["mask"], mask.ctypes.data, n_streams))
        before = dev.snapshot().processor

        def run(cap_streams, cap_bytes):
            b.wm._lib.check(L.fskhip_processor_rx_drain_sparse_device(dev._h, d["mask"], 3, d["streams"], d["offsets"], cap_streams, d["data"], cap_bytes,
                                                                      d["totals"], stream))
            assert hip.hipStreamSynchronize(stream) == 0
            totals = np.zeros(3, np.uint32)
            b.wm._lib.check(L.fskhip_memcpy_d2h(eh, totals.ctypes.data, d["totals"], 12))
            return list(totals)
        # caps too short: the totals are the true sizes, the flag is 0 and nothing is drained
        assert run(len(ws) - 1, len(wd)) == [len(ws), len(wd), 0]
        assert run(len(ws), len(wd) - 1) == [len(ws), len(wd), 0]
        assert dev.snapshot().processor == before
        assert run(len(ws), len(wd)) == [len(ws), len(wd), 1]
        gs, go, gd = np.zeros(len(ws), np.uint32), np.zeros(len(ws) + 1, np.uint32), np.zeros(len(wd), np.uint8)
        for arr, k in ((gs, "streams"), (go, "offsets"), (gd, "data")):
            b.wm._lib.check(L.fskhip_memcpy_d2h(eh, arr.ctypes.data, d[k], arr.nbytes))
        for got, hostform, want in ((gs, hs, ws), (go, ho, wo), (gd, hd, wd)):
            assert np.array_equal(got, hostform) and np.array_equal(got, want)
        assert dev.snapshot().processor == host.snapshot().processor == after.image(fresh=b.fresh.processor)
    finally:
        for p in d.values():
            L.fskhip_device_free(eh, p)
        hip.hipStreamDestroy(stream)


@pytest.mark.parametrize("use_graph", [False, True], ids=["launches", "graph"])
def test_after_real_traffic_matches_the_golden_run(use_graph):
    """a golden FSKProcessor run whose ring never overflows, drained sparsely every 7 quanta instead of densely where the
    reference drained: the concatenated bytes per stream are the golden's; with the graph, the uncaptured drain sits between
    replays of the captured quantum"""
    import webaudio_modem_amd as wm
    from oracle import pyoracle as po
    from test_oracle_next import rx_run_input
    run = next(r for r in golden_next().manifest["processor"] if r["name"] == "rx_v21_2x16")
    want = bytes(sum((d["bytes"] for d in run["drains"]), []))
    assert 0 < len(want) <= run["ring_capacity"]
    S = 3
    eng = wm.FSKEngine(S, run["config"], precision=wm.PRECISION_F32)
    proc = wm.FSKProcessorBatch(eng, rx_capacity=run["ring_capacity"], use_graph=use_graph)
    buf = rx_run_input(lambda: po.OracleCore(run["config"]), run)
    got = [b""] * S
    calls_with_bytes = 0
    for q in range(run["quanta"]):
        proc.process(np.tile(buf[q * 128:(q + 1) * 128], (S, 1)), 0)
        if q % 7 == 6 or q == run["quanta"] - 1:
            active = proc.demodulate_active()
            calls_with_bytes += bool(active)
            for s, v in active.items():
                got[s] += v
    assert got == [want] * S and calls_with_bytes > 1
    assert not proc.rx_lengths().any()
    proc.close()
    eng.close()


def test_remap_refuses_a_destination_that_has_been_drained_sparsely():
    import webaudio_modem_amd as wm
    engs = [wm.FSKEngine(4, {}, precision=wm.PRECISION_F32) for _ in range(2)]
    src, dst = (wm.FSKProcessorBatch(e, rx_capacity=16) for e in engs)
    assert dst.demodulate_active() == {}
    m = np.arange(4, dtype=np.int64)
    rc = dst._L.fskhip_processor_remap(dst._h, src._h, m.ctypes.data, 4)
    assert rc == E_INVALID
    assert dst._L.fskhip_last_error().decode() == ("fskhip_processor_remap: the destination has been used already (process, modulate, drain or reset: "
                                                   "remap into a freshly created processor)")
    for p in (src, dst):
        p.close()
    for e in engs:
        e.close()
