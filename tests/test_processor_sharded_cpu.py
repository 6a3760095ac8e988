"""FSKProcessorBatchSharded and fskhip_processor_snapshot_concat without a GPU: the shard arithmetic, the no-copy slicing of the
caller's arrays, the merge of the per-shard sparse drains, the rate-handle refusals and the worker count through stand-in
processors (processor_factory: no HIP is involved); the concatenation of processor images through the library's host-only call
on images crafted by hand, and through the header's own definition as a stand-alone program under ASan + UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_processor_snapshot_cpu import _image, _record, _flip, HEADER, FIXED


@pytest.fixture(scope="module")
def wm():
    import __graft_entry__ as ge
    ge.build()
    import webaudio_modem_amd
    return webaudio_modem_amd


class StandIn:
    """a processor that records what it is handed"""

    def __init__(self, count, cfg, device, precision, log):
        self.n_streams, self.cfg, self.device, self.precision, self.log = count, cfg, device, precision, log
        self.processDemodulationCallCount = 0
        self.calls = []
        self.sparse = (np.zeros(0, np.uint32), np.zeros(1, np.uint32), np.zeros(0, np.uint8))
        log.append(self)

    def close(self):
        pass

    def process(self, inputs, n_out, out=None):
        self.calls.append(("process", inputs, n_out, out))
        if out is not None:
            out[...] = self.device
        return out

    def process_samples(self, inputs, in_fmt, in_layout, n_out, out_fmt, out_layout, out=None):
        self.calls.append(("process_samples", inputs, in_fmt, in_layout, n_out, out_fmt, out_layout, out))
        if out is not None:
            out[...] = self.device
        return out

    def process_samples_at(self, *a, **kw):
        self.calls.append(("process_samples_at", a, kw))

    def process_samples_at_any(self, *a, **kw):
        self.calls.append(("process_samples_at_any", a, kw))

    def demodulate_sparse(self, mask=None, min_len=1):
        self.calls.append(("demodulate_sparse", mask, min_len))
        return self.sparse


def _sharded(wm, S, devices, **kw):
    log = []
    b = wm.FSKProcessorBatchSharded(S, {}, devices=devices, processor_factory=lambda c, cfg, d, p: StandIn(c, cfg, d, p, log), **kw)
    return b, log


@pytest.mark.parametrize("S,devices", [(131, [4, 6]), (131, [0, 1, 2]), (3, [0, 1, 2, 3, 4])])
def test_the_shard_blocks_are_all_shards(wm, S, devices):
    b, log = _sharded(wm, S, devices)
    want = [(first, count, dev) for (first, count), dev in zip(wm.sharding.all_shards(S, len(devices)), devices) if count]
    assert b.shards == want and sum(c for _, c, _ in want) == S
    assert [(p.n_streams, p.device) for p in log] == [(c, d) for _, c, d in want]
    assert b.processors == log and b.engines == [None] * len(log)
    if S == 131:
        assert [c for _, c, _ in want] == ([66, 65] if len(devices) == 2 else [44, 44, 43])
    else:
        assert len(want) == 3                       # two of the five devices have nothing to do and get no processor
    for i, (first, count, _dev) in enumerate(want):
        assert b.locate(first) == (i, 0) and b.locate(first + count - 1) == (i, count - 1)
    with pytest.raises(ValueError):
        b.locate(S)
    b.close()
    with pytest.raises(ValueError, match="devices"):
        wm.FSKProcessorBatchSharded(4, {}, processor_factory=lambda *a: None)


def _addr(a):
    return a.__array_interface__["data"][0]


@pytest.mark.parametrize("devices", [[0, 1], [0, 1, 2]])
def test_every_stand_in_gets_a_view_of_the_callers_arrays(wm, devices):
    S, n = 131, 24
    b, log = _sharded(wm, S, devices)
    # stream-major float32 through process(): row blocks, input and output
    x = np.arange(S * n, dtype=np.float32).reshape(S, n)
    out = np.full((S, n), -1, np.float32)
    assert b.process(x, n, out=out) is out
    for p, (first, count, dev) in zip(log, b.shards):
        _, xi, n_out, oi = p.calls[-1]
        assert np.shares_memory(xi, x) and np.shares_memory(oi, out) and n_out == n
        assert _addr(xi) == _addr(x) + first * n * 4 and xi.shape == (count, n) and xi.strides == (n * 4, 4)
        assert _addr(oi) == _addr(out) + first * n * 4 and oi.shape == (count, n)
        assert (out[first:first + count] == dev).all()
    assert b.processDemodulationCallCount == 1
    # stream-major rows of a WIDER caller array: the pitch is the wider array's
    wide = np.zeros((S, n + 8), np.int16)
    got = b.process_samples(wide[:, 3:3 + n], "s16", "stream", n, "s16", "stream", out=wide[:, 3:3 + n])
    assert np.shares_memory(got, wide)
    for p, (first, count, dev) in zip(log, b.shards):
        _, xi, in_fmt, in_lay, n_out, out_fmt, out_lay, oi = p.calls[-1]
        assert (in_fmt, in_lay, out_fmt, out_lay) == (wm.SAMPLE_FORMATS["s16"], wm.SAMPLE_LAYOUTS["stream"]) * 2
        assert np.shares_memory(xi, wide) and _addr(xi) == _addr(wide) + (first * (n + 8) + 3) * 2 and xi.strides == ((n + 8) * 2, 2)
        assert np.shares_memory(oi, wide) and _addr(oi) == _addr(xi)
    assert (wide[:, :3] == 0).all() and (wide[:, 3 + n:] == 0).all()
    # interleaved frames: COLUMN blocks at the full frame pitch, guard columns either side of the caller's out untouched
    frames = np.zeros((n, S), np.uint8)
    guard = np.full((n, S + 2), 0xEE, np.uint8)
    got = b.process_samples(frames, "mulaw", "sample", n, "mulaw", "sample", out=guard[:, 1:S + 1])
    assert np.shares_memory(got, guard) and got.shape == (n, S)
    for p, (first, count, dev) in zip(log, b.shards):
        _, xi, in_fmt, in_lay, n_out, out_fmt, out_lay, oi = p.calls[-1]
        assert in_lay == out_lay == wm.SAMPLE_LAYOUTS["sample"]
        assert np.shares_memory(xi, frames) and _addr(xi) == _addr(frames) + first and xi.shape == (n, count) and xi.strides == (S, 1)
        assert np.shares_memory(oi, guard) and _addr(oi) == _addr(guard) + 1 + first and oi.shape == (n, count) and oi.strides == (S + 2, 1)
        assert (guard[:, 1 + first:1 + first + count] == dev).all()
    assert (guard[:, 0] == 0xEE).all() and (guard[:, S + 1] == 0xEE).all()
    assert b.processDemodulationCallCount == 3
    # an out the call cannot express is refused before any stand-in is called
    before = [len(p.calls) for p in log]
    for bad in (np.zeros((n, S), np.int16), np.zeros((n, S + 1), np.uint8), np.zeros((n, 2 * S), np.uint8)[:, ::2], np.zeros((S, n), np.uint8).T):
        with pytest.raises(ValueError):
            b.process_samples(frames, "mulaw", "sample", n, "mulaw", "sample", out=bad)
    with pytest.raises(ValueError, match="n_out is 0"):
        b.process(x, 0, out=out)
    assert [len(p.calls) for p in log] == before and b.processDemodulationCallCount == 3
    b.close()


def test_the_sparse_drain_merges_into_global_streams_and_one_csr(wm):
    b, log = _sharded(wm, 131, [0, 1, 2])          # 44 + 44 + 43
    log[0].sparse = (np.array([0, 43], np.uint32), np.array([0, 3, 8], np.uint32), np.frombuffer(b"abcDEFGH", np.uint8))
    # (the shard in the middle holds nothing)
    log[2].sparse = (np.array([1, 2, 42], np.uint32), np.array([0, 1, 5, 6], np.uint32), np.frombuffer(b"xWXYZq", np.uint8))
    mask = np.arange(131) % 2 == 0
    streams, offsets, data = b.demodulate_sparse(mask=mask, min_len=3)
    assert streams.dtype == offsets.dtype == np.uint32 and data.dtype == np.uint8
    assert streams.tolist() == [0, 43, 89, 90, 130] and (np.diff(streams.astype(np.int64)) > 0).all()
    assert offsets.tolist() == [0, 3, 8, 9, 13, 14] and data.tobytes() == b"abcDEFGHxWXYZq"
    for p, (first, count, _dev) in zip(log, b.shards):
        name, m, min_len = p.calls[-1]
        assert name == "demodulate_sparse" and min_len == 3 and m.tolist() == mask[first:first + count].tolist()
    assert b.demodulate_active() == {0: b"abc", 43: b"DEFGH", 89: b"x", 90: b"WXYZ", 130: b"q"}
    for p in log:
        p.sparse = (np.zeros(0, np.uint32), np.zeros(1, np.uint32), np.zeros(0, np.uint8))
    streams, offsets, data = b.demodulate_sparse()
    assert streams.tolist() == [] and offsets.tolist() == [0] and data.size == 0
    with pytest.raises(ValueError, match="mask"):
        b.demodulate_sparse(mask=[True] * 130)
    b.close()


def test_rate_handle_refusals_come_before_any_stand_in_is_called(wm, monkeypatch):
    f = wm.filters
    monkeypatch.setattr(f.CaptureConverter, "position", property(lambda self: self._pos), raising=False)
    monkeypatch.setattr(f.PlaybackConverter, "position", property(lambda self: self._pos), raising=False)

    def h(cls, n, dev, pos=0):
        o = object.__new__(cls)
        o.n_streams, o.device, o.up, o.down, o._h, o._pos = n, dev, 160, 147, None, pos
        return o
    b, log = _sharded(wm, 131, [3, 5])             # 66 on device 3, 65 on device 5
    frames = np.zeros((128, 131), np.int16)
    good_up = [h(f.CaptureConverter, 66, 3), h(f.CaptureConverter, 65, 5)]
    good_down = [h(f.PlaybackConverter, 66, 3), h(f.PlaybackConverter, 65, 5)]
    bad = [
        (dict(upsampler=good_up[:1], downsampler=good_down), ValueError, "one per shard"),
        (dict(upsampler=good_up[0], downsampler=good_down), ValueError, "one per shard"),
        (dict(upsampler=None, downsampler=good_down), ValueError, "one per shard"),
        (dict(upsampler=good_up, downsampler=good_down + good_down[:1]), ValueError, "one per shard"),
        (dict(upsampler=[good_up[0], h(f.CaptureConverter, 66, 5)], downsampler=good_down), ValueError, "has 66 streams, the batch 65"),
        (dict(upsampler=[good_up[0], h(f.CaptureConverter, 65, 3)], downsampler=good_down), ValueError, "is on device 3, the batch on 5"),
        (dict(upsampler=good_up, downsampler=[good_down[0], h(f.CaptureConverter, 65, 5)]), ValueError, "must be a filters.Downsampler"),
        (dict(upsampler=good_up, downsampler=[good_down[0], h(f.PlaybackConverter, 65, 5, pos=7)]), ValueError, "different positions"),
        (dict(upsampler=[h(f.Upsampler, 66, 3), h(f.Upsampler, 65, 5)], downsampler=good_down), TypeError, "any length"),
    ]
    for kw, exc, pattern in bad:
        with pytest.raises(exc, match=pattern):
            b.process_samples_at_any(frames, "s16", "sample", n_out=128, out_fmt="s16", out_layout="sample", **kw)
    # the whole-period form: its count checks come first as well, and it does not look at positions
    with pytest.raises(ValueError, match="multiple of the converter's down factor"):
        b.process_samples_at(frames, "s16", "sample", upsampler=good_up, n_out=160, out_fmt="s16", out_layout="sample", downsampler=good_down)
    with pytest.raises(ValueError, match="not one of each"):
        b.process_samples_at(frames[:147], "s16", "sample", upsampler=good_up, n_out=160, out_fmt="s16", out_layout="sample",
                             downsampler=[h(f.Downsampler, 66, 3), h(f.Downsampler, 65, 5)])
    assert all(p.calls == [] for p in log) and b.processDemodulationCallCount == 0
    # and the good call reaches every stand-in with its own handles and its column blocks of ONE out
    out = b.process_samples_at_any(frames, "s16", "sample", upsampler=good_up, n_out=128, out_fmt="s16", out_layout="sample", downsampler=good_down)
    assert out.shape == (128, 131) and out.dtype == np.int16
    for i, (p, (first, count, _dev)) in enumerate(zip(log, b.shards)):
        name, a, kw = p.calls[-1]
        assert name == "process_samples_at_any" and a[3] is good_up[i] and a[7] is good_down[i]
        assert np.shares_memory(a[0], frames) and a[0].shape == (128, count) and np.shares_memory(kw["out"], out) and _addr(kw["out"]) == _addr(out) + 2 * first
    assert b.processDemodulationCallCount == 1
    # a side without samples needs no handles
    b.process_samples_at_any(frames, "s16", "sample", upsampler=good_up)
    assert log[0].calls[-1][1][7] is None
    b.close()


@pytest.mark.parametrize("n_dev", [1, 3, 16, 40])
def test_the_worker_count_is_the_shard_count_and_at_most_16(wm, n_dev):
    b, log = _sharded(wm, 200, list(range(n_dev)))
    assert len(b.shards) == n_dev and b._pool._max_workers == min(n_dev, 16)
    x = np.zeros((200, 4), np.float32)
    b.process(x, 0)
    assert [len(p.calls) for p in log] == [1] * n_dev          # (more shards than workers: every shard is still called)
    b.close()
    e = wm.FSKEngineSharded(200, {}, devices=list(range(n_dev)), engine_factory=lambda c, cfg, d, p: StandIn(c, cfg, d, p, []))
    assert e._pool._max_workers == min(n_dev, 16)              # one definition: the engine class's pool is the same
    assert type(e)._fan_out is type(b)._fan_out and type(e).locate is type(b).locate
    e.close()


# ---- fskhip_processor_snapshot_concat on hand-made images (the layout include/fskhip_next.h documents) -----------------------------
def _records(g0, n, rx_cap):
    out = []
    for g in range(g0, g0 + n):
        ring = bytes((g * 7 + i) % 255 + 1 for i in range((0, 5, rx_cap, 2)[g % 4]))
        pay = bytes((g + i) & 0xFF for i in range(1 + g * 13 % 40)) if g % 3 == 1 else b""
        out.append((ring, (rx_cap - 2) if g % 4 == 1 else g % rx_cap if len(ring) < rx_cap else 3, pay, g))
    return out


def _image_of(recs, rx_cap):
    pay_cap = (max((len(p) for _, _, p, _ in recs), default=0) + 15) // 16 * 16
    return _image([_record(rx_cap, pay_cap, ring=r, read=rd, payload=p, pos=g if p else 0, total=4800 if p else 0, completed=g % 3,
                           phase=0.5 * g if p else 0.0, cursor=(g % 40, g % 9, g & 1) if p else (0, 0, 0)) for r, rd, p, g in recs],
                  rx_cap=rx_cap, pay_cap=pay_cap)


@pytest.mark.parametrize("counts", [(0,), (65,), (1, 65), (65, 0, 1), (0, 0), (2, 65, 3)], ids=str)
def test_concatenated_images_are_the_one_image_of_all_records(wm, counts):
    rx_cap = 50
    recs = _records(0, sum(counts), rx_cap)
    parts, at = [], 0
    for c in counts:
        parts.append(_image_of(recs[at:at + c], rx_cap))
        at += c
    whole = _image_of(recs, rx_cap)
    got = wm.processor_snapshot_concat(parts)
    assert isinstance(got, bytes) and got == whole
    assert wm.processor_snapshot_info(got)["n_streams"] == sum(counts)
    if len(counts) > 1 and 65 in counts:
        assert len({wm.processor_snapshot_info(p)["payload_capacity"] for p in parts}) > 1      # the parts do differ in their pitch


def test_the_concatenation_refuses_what_it_must(wm):
    from webaudio_modem_amd import _lib
    L = _lib.lib()
    a, b = _image(), _image()

    def call(blobs, cap=None, sizes=None):
        bufs = [(C.c_char * max(len(x), 1)).from_buffer_copy(x.ljust(1, b"\0")) for x in blobs]
        ptrs = (C.c_void_p * len(bufs))(*[C.addressof(x) for x in bufs])
        sz = (C.c_size_t * len(bufs))(*(sizes or [len(x) for x in blobs]))
        need = 2 * HEADER + sum(len(x) for x in blobs)
        out = (C.c_char * need)()
        w = C.c_size_t(0)
        rc = L.fskhip_processor_snapshot_concat(ptrs, sz, len(bufs), out if cap != 0 else None, need if cap is None else cap, C.byref(w))
        return rc, L.fskhip_last_error().decode(), w.value, out.raw
    true_size = len(a) + len(b) - HEADER
    rc, msg, w, _ = call([a, b])
    assert rc == 0 and w == true_size, msg
    rc, msg, w, _ = call([a, b], cap=0)
    assert rc == _lib.E_OVERFLOW and w == true_size and "fskhip_processor_snapshot_concat" in msg
    rc, msg, w, raw = call([a, b], cap=true_size - 1)
    assert rc == _lib.E_OVERFLOW and w == true_size and not any(raw), msg
    for blobs, pattern in (([a, _image(rx_cap=64, records=[])], "differ in rx_capacity"), ([a, _image(magic=0x534B5346)], "magic"),
                           ([a, _image(format=7)], "format 7"), ([a[:-16], b], "do not match n_records x record_bytes"),
                           ([a, _flip(b, 33)], "checksum"), ([a, _flip(b, HEADER + FIXED + 1)], "checksum")):
        rc, msg, w, raw = call(blobs)
        assert rc == _lib.E_INVALID and pattern in msg and "fskhip_processor_snapshot_concat" in msg and not any(raw), (pattern, msg)
    assert "(snapshot 1)" in call([a, _flip(b, 33)])[1] and "(snapshot 0)" in call([a[:-16], b])[1]
    assert L.fskhip_processor_snapshot_concat(None, None, 0, None, 0, None) == _lib.E_INVALID
    with pytest.raises(wm.FskHipError, match="rx_capacity"):
        wm.processor_snapshot_concat([a, _image(rx_cap=64, records=[])])


def test_the_concatenation_is_declared_exported_and_bound(wm):
    import re
    from webaudio_modem_amd import _lib
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fskhip_next.h")).read(), flags=re.S)
    assert re.search(r"\bint fskhip_processor_snapshot_concat\(", code)
    assert "fskhip_processor_snapshot_concat" in _lib.SYMBOL_NAMES and _lib.lib().fskhip_abi_version() == 8     # additions only
    addon = open(os.path.join(ROOT, "napi", "fsk_addon_next.cc")).read()
    assert "fskhip_processor_snapshot_concat(" in addon and '"processorSnapshotConcat"' in addon
    js = open(os.path.join(ROOT, "napi", "fsk-processor.js")).read()
    assert "class FSKProcessorBatchSharded" in js and "addon.processorSnapshotConcat(" in js
    dts = open(os.path.join(ROOT, "napi", "fsk-processor.d.ts")).read()
    assert "export declare class FSKProcessorBatchSharded" in dts and "export declare function processorSnapshotConcat(" in dts
    # (through N-API: tests/test_node_processor_sharded.py)


def test_the_header_definition_holds_as_a_host_program(tmp_path):
    """tests/cpp/processor_image_concat_check.cpp under ASan + UBSan: no library"""
    exe = str(tmp_path / "processor_image_concat_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "webaudio_modem_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "processor_image_concat_check.cpp")],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.stdout, r.stderr)
    assert r.stdout.strip() == "ok 78 concatenations, 88 refusals"
