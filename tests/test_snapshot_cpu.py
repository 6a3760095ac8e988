"""Stream snapshots without a GPU (include/fskhip.h): the six functions are declared, exported and bound on both hosts, and the
host-side ones -- fskhip_snapshot_info_get, _stream_config, _concat, and the checks fskhip_restore_streams makes before it needs
its engine -- are loud on every damaged image, and the host-only validator (csrc/fsk_snapshot_image.h) walks the same images as a
stand-alone program under ASan + UBSan.  The images are crafted by hand here from the documented layout (a 352-byte header,
fixed-size records); no engine is involved."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))

NAMES = ["fskhip_snapshot_bytes", "fskhip_snapshot_streams", "fskhip_snapshot_info_get", "fskhip_snapshot_stream_config",
         "fskhip_snapshot_concat", "fskhip_restore_streams"]
HEADER = 352
D = 20            # dsSPB of the default configuration: 48000 / 2 / 1200


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from webaudio_modem_amd import _lib
    return _lib


def _stamp():
    """the state-layout stamp: FNV-1a over the field names in fsk_params.h order and the two spans the fp32 reset words count in"""
    import state_fields
    text = open(os.path.join(ROOT, "webaudio_modem_amd", "csrc", "fsk_params.h")).read()
    zlag = int(re.search(r"#define FSK_ZLAG (\d+)", text).group(1))
    hlag = int(re.search(r"#define FSK_HLAG (\d+)", text).group(1))
    names = "".join(n + "," for n in state_fields.REAL) + "|" + "".join(n + "," for n in state_fields.INT)
    h = 0xcbf29ce484222325
    for b in list(names.encode()) + [zlag, hlag]:
        h = ((h ^ b) * 0x100000001b3) & (2**64 - 1)
    return len(state_fields.REAL), len(state_fields.INT), h


def _record_bytes(precision=0):
    rf, nif, _ = _stamp()
    words = 12 + 8 * D + rf * (2 if precision else 1) + nif + D
    return 4 * ((words + 3) // 4 * 4)


def _checksum(blob):
    w = np.frombuffer(bytes(blob), dtype="<u8")
    with np.errstate(over="ignore"):
        a = np.cumsum(w, dtype=np.uint64)
        b = np.sum(a, dtype=np.uint64)
        return int((a[-1] * np.uint64(0x9E3779B97F4A7C15)) ^ b)


def _image(n=0, precision=0, calls=3, records=None, **over):
    """a well-formed snapshot of n streams of the default configuration (records: all zero but for the per-stream config fields)"""
    rf, nif, stamp = _stamp()
    rb = _record_bytes(precision)
    f = dict(magic=0x534B5346, format=1, rf=rf, nif=nif, stamp=stamp, header_bytes=HEADER, record_bytes=rb, n=n, precision=precision,
             per_stream=0, d=D, amp_cap=8 * D, wide=0, frac=0, n_bits=30, ring_cap=1364, calls=calls, total=calls * 100)
    f.update(over)
    head = struct.pack("<4IQQ3Ii", f["magic"], f["format"], f["rf"], f["nif"], f["stamp"], 0, f["header_bytes"], f["record_bytes"], f["n"], f["precision"])
    head += struct.pack("<14I2I4Q", f["per_stream"], f["d"], f["amp_cap"], f["wide"], f["frac"], f["n_bits"], f["ring_cap"], 0, 1, 0, 0, 0, 0, 0, 0, 0,
                        0, f["calls"], f["total"], f["total"] // 2)
    head += struct.pack("<6d", 48000, 1200, 1650, 1850, 0.85, 800)
    head += struct.pack("<16i16i8i", *([0x55, 0x55] + [0] * 14 + [0x7E] + [0] * 15 + [2, 1, 1, 1, 0, 1, 1, 0]))
    assert len(head) == HEADER
    if records is None:
        records = b"".join(struct.pack("<3d2I2Q", 1650 + 10 * i, 1850 + 10 * i, 800, 1, 0, 0, 0).ljust(rb, b"\0") for i in range(n))
    blob = bytearray(head + records)
    blob[24:32] = struct.pack("<Q", _checksum(blob))
    return bytes(blob)


def _buf(b):
    return (C.c_char * max(len(b), 1)).from_buffer_copy(b.ljust(1, b"\0"))


def _info(lib, blob, size=None):
    L = lib.lib()
    info = lib.SnapshotInfo()
    rc = L.fskhip_snapshot_info_get(_buf(blob) if blob is not None else None, len(blob) if size is None else size, C.byref(info))
    return rc, L.fskhip_last_error().decode(), info


def _config(lib, blob, i=0):
    L = lib.lib()
    c = lib.Config()
    rc = L.fskhip_snapshot_stream_config(_buf(blob) if blob is not None else None, len(blob or b""), i, C.byref(c))
    return rc, L.fskhip_last_error().decode(), c


def _concat(lib, blobs):
    L = lib.lib()
    bufs = [_buf(b) if b is not None else None for b in blobs]
    ptrs = (C.c_void_p * len(blobs))(*[C.cast(b, C.c_void_p) if b is not None else None for b in bufs])
    sizes = (C.c_size_t * len(blobs))(*[len(b or b"") for b in blobs])
    out = (C.c_char * (1 << 16))()
    w = C.c_size_t(0)
    rc = L.fskhip_snapshot_concat(ptrs, sizes, len(blobs), out, len(out), C.byref(w))
    return rc, L.fskhip_last_error().decode(), bytes(out[:w.value]) if rc == 0 else b""


def _restore(lib, blob, m=(), dst=None):
    L = lib.lib()
    a = np.ascontiguousarray(m, np.int64)
    rc = L.fskhip_restore_streams(dst, _buf(blob) if blob is not None else None, len(blob or b""), a.ctypes.data if len(a) else None, len(a))
    return rc, L.fskhip_last_error().decode()


def test_snapshot_functions_are_declared_exported_and_bound(lib):
    hdr = open(os.path.join(ROOT, "include", "fskhip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = C.CDLL(lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b(int|size_t) %s\(" % name, code), name
        assert hasattr(L, name), name
        assert name in lib.SYMBOL_NAMES, name
    assert "typedef struct fskhip_snapshot_info {" in code
    import webaudio_modem_amd as wm
    for meth in ("snapshot", "restore_from", "from_snapshot"):
        assert callable(getattr(wm.FSKEngine, meth)), meth
    for meth in ("snapshot", "remapped", "from_snapshot"):
        assert callable(getattr(wm.FSKEngineSharded, meth)), meth
    assert callable(wm.snapshot_info) and callable(wm.snapshot_concat)
    addon = open(os.path.join(ROOT, "napi", "fsk_addon.cc")).read()
    for call, js_name in (("fskhip_snapshot_streams(", '"snapshotStreams"'), ("fskhip_restore_streams(", '"restoreStreams"'),
                          ("fskhip_snapshot_info_get(", '"snapshotInfo"'), ("fskhip_snapshot_concat(", '"snapshotConcat"')):
        assert call in addon and js_name in addon, js_name
    js = open(os.path.join(ROOT, "napi", "fsk-core.js")).read()
    for use in ("addon.snapshotStreams(", "addon.restoreStreams(", "addon.snapshotInfo(", "addon.snapshotConcat(", "static fromSnapshot(buf, map, configs, device)"):
        assert use in js, use
    assert re.search(r"\n  snapshot\(streams\)", js) and re.search(r"\n  remap\(map, configs, options = \{\}\)", js)
    dts = open(os.path.join(ROOT, "napi", "fsk-core.d.ts")).read()
    for decl in ("snapshot(streams?: ArrayLike<number>): Buffer;", "static fromSnapshot(buf: Uint8Array", "): FSKBatchSharded;", "snapshot(): Buffer;",
                 "export function snapshotInfo(", "export function snapshotConcat("):
        assert decl in dts, decl


def test_abi_version_is_still_8(lib):
    assert lib.lib().fskhip_abi_version() == 8


def test_well_formed_images_are_read_on_the_host(lib):
    rc, msg, info = _info(lib, _image(0))
    assert rc == 0, msg
    assert (info.n_streams, info.precision, info.per_stream_configs, info.record_bytes) == (0, 0, 0, _record_bytes(0))
    assert (info.demodulationCalls, info.totalSamplesProcessed) == (3, 300)
    rc, msg, c = _config(lib, _image(0))                      # an empty snapshot still yields the shared configuration
    assert rc == 0, msg
    d = lib.Config()
    lib.lib().fskhip_default_config(C.byref(d))
    assert bytes(c) == bytes(d)
    blob = _image(3, precision=1)
    rc, msg, info = _info(lib, blob)
    assert rc == 0 and (info.n_streams, info.precision, info.record_bytes) == (3, 1, _record_bytes(1)), msg
    for i in range(3):
        rc, msg, c = _config(lib, blob, i)
        assert rc == 0 and (c.markFrequency, c.spaceFrequency, c.preFilterBandwidth, c.baudRate) == (1650 + 10 * i, 1850 + 10 * i, 800, 1200), msg
    rc, msg, _ = _config(lib, blob, 3)
    assert rc == lib.E_INVALID and "record 3" in msg
    # an unaligned copy reads the same
    raw = bytearray(1 + len(blob))
    raw[1:] = blob
    info = lib.SnapshotInfo()
    arr = (C.c_char * len(raw)).from_buffer(raw)
    assert lib.lib().fskhip_snapshot_info_get(C.addressof(arr) + 1, len(blob), C.byref(info)) == 0 and info.n_streams == 3


BAD = [
    ("null", None, "null snapshot"),
    ("short", lambda: _image(2)[:HEADER - 8], "fewer than a snapshot header"),
    ("magic", lambda: _image(2, magic=0x12345678), "magic"),
    ("format", lambda: _image(2, format=7), "format 7"),
    ("layout-count", lambda: _image(2, rf=_stamp()[0] + 1), "state layout"),
    ("layout-stamp", lambda: _image(2, stamp=_stamp()[2] ^ 1), "state layout"),
    ("precision", lambda: _image(2, precision=5), "precision 5"),
    ("record-bytes", lambda: _image(2, record_bytes=_record_bytes(0) + 16), "record_bytes"),
    ("size", lambda: _image(2) + b"\0" * 8, "do not match n_streams x record_bytes"),
    ("truncated", lambda: _image(2)[:-16], "do not match n_streams x record_bytes"),
    ("flipped-record-byte", lambda: _flip(_image(2), HEADER + 777), "checksum"),
    ("flipped-header-byte", lambda: _flip(_image(2), 130), "checksum"),
]


def _flip(blob, at):
    b = bytearray(blob)
    b[at] ^= 0x40
    return bytes(b)


@pytest.mark.parametrize("name,make,pattern", BAD, ids=[b[0] for b in BAD])
def test_damaged_images_are_refused_with_a_telling_message(lib, name, make, pattern):
    blob = make() if make else None
    for fn, call in (("fskhip_snapshot_info_get", lambda: _info(lib, blob, size=len(blob or b""))[:2]),
                     ("fskhip_snapshot_stream_config", lambda: _config(lib, blob)[:2]),
                     ("fskhip_restore_streams", lambda: _restore(lib, blob, [0, 1])),
                     ("fskhip_snapshot_concat", lambda: _concat(lib, [_image(2), blob])[:2])):
        rc, msg = call()
        assert rc == lib.E_INVALID, (fn, rc, msg)
        assert pattern in msg and fn in msg, (fn, msg)
    rc, msg = _concat(lib, [_image(2), blob])[:2]
    assert "snapshot 1" in msg                                   # concat says which of its inputs


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    from test_processor_snapshot_cpu import build_image_check
    return build_image_check(tmp_path_factory)


def test_the_validator_walks_the_same_images_as_a_host_program(lib, program):
    from test_processor_snapshot_cpu import walk_images
    good = [_image(0), _image(3, precision=1), _image(2), _image(3), _image(1)]
    bad = [(make() if make else None, pattern) for _, make, pattern in BAD]
    blobs = good + [b for b, _ in bad]
    lines = walk_images(program, "S", blobs)
    for blob, line in zip(blobs, lines):
        rc, msg, info = _info(lib, blob, size=len(blob or b""))
        if rc == 0:
            assert line == "0 %d %d %d %d %d" % (info.n_streams, info.precision, info.per_stream_configs, info.record_bytes, sum(blob[HEADER:])), line
        else:
            assert line.startswith("-1 ") and msg == "fskhip_snapshot_info_get: " + line[3:], (line, msg)
    assert [ln[0] for ln in lines[:len(good)]] == ["0"] * len(good)
    for (_, pattern), line in zip(bad, lines[len(good):]):
        assert line.startswith("-1 ") and pattern in line, (pattern, line)


def test_concat_joins_images_of_one_history_and_names_the_field_that_differs(lib):
    a, b = _image(2), _image(3)
    rc, msg, out = _concat(lib, [a, b, _image(0)])
    assert rc == 0, msg
    rb = _record_bytes(0)
    assert len(out) == HEADER + 5 * rb
    assert out[HEADER:] == a[HEADER:] + b[HEADER:]               # the records, in order, untouched
    rc, msg, info = _info(lib, out)
    assert rc == 0 and info.n_streams == 5 and info.demodulationCalls == 3, msg
    rc, msg, one = _concat(lib, [a])
    assert rc == 0 and one == a, msg                             # deterministic: one input comes back byte for byte
    for other, field in ((_image(2, calls=4), "calls"), (_image(2, precision=1), "precision"), (_image(2, ring_cap=1365), "ring_cap"),
                         (_image(2, n_bits=40), "n_bits")):
        rc, msg, _ = _concat(lib, [a, other])
        assert rc == lib.E_INVALID and "differ in " + field in msg, msg
    L = lib.lib()
    assert L.fskhip_snapshot_concat(None, None, 0, None, 0, None) == lib.E_INVALID
    # too small an output: the size needed comes back
    bufs = [_buf(a), _buf(b)]
    ptrs = (C.c_void_p * 2)(*[C.cast(x, C.c_void_p) for x in bufs])
    sizes = (C.c_size_t * 2)(len(a), len(b))
    w = C.c_size_t(0)
    assert L.fskhip_snapshot_concat(ptrs, sizes, 2, (C.c_char * 64)(), 64, C.byref(w)) == lib.E_OVERFLOW
    assert w.value == HEADER + 5 * rb


def test_engine_calls_fail_loudly_without_an_engine(lib):
    L = lib.lib()
    w = C.c_size_t(0)
    assert L.fskhip_snapshot_streams(None, None, 0, (C.c_char * 64)(), 64, C.byref(w)) == lib.E_INVALID
    assert "null engine" in L.fskhip_last_error().decode()
    assert L.fskhip_snapshot_bytes(None, 4) == 0
    rc, msg = _restore(lib, _image(2), [0, 1])
    assert rc == lib.E_INVALID and "null engine" in msg
    rc, msg = _restore(lib, _image(2), [0, 1, -2, -3])
    assert rc == lib.E_INVALID and "map[2] = -2" in msg          # the first offending index, as the remap names it
    a = lib.lib().fskhip_restore_streams(None, _buf(_image(2)), len(_image(2)), None, 4)
    assert a == lib.E_INVALID and "null map" in L.fskhip_last_error().decode()


def test_python_host_reads_images(lib):
    import webaudio_modem_amd as wm
    blob = _image(3)
    info = wm.snapshot_info(blob)
    assert info["n_streams"] == 3 and info["precision"] == wm.PRECISION_F32
    cfg = wm.snapshot_stream_config(np.frombuffer(blob, np.uint8), 2)
    assert cfg["markFrequency"] == 1670 and cfg["preamblePattern"] == [0x55, 0x55] and cfg["parity"] == "none" and cfg["agcEnabled"] is True
    out = wm.snapshot_concat([blob, _image(1)])
    assert wm.snapshot_info(out)["n_streams"] == 4
    with pytest.raises(wm.FskHipError, match="differ in calls"):
        wm.snapshot_concat([blob, _image(1, calls=9)])
    with pytest.raises(wm.FskHipError, match="checksum"):
        wm.snapshot_info(_flip(blob, 400))


def test_node_addon_binds_snapshots():
    node = shutil.which("node")
    addon = os.path.join(ROOT, "napi", "fsk_addon.node")
    import __graft_entry__ as ge
    ge.build()
    if node is None or not os.path.exists(addon):
        pytest.skip("node / the N-API addon not available")
    blob = _image(2)
    script = ("const a = require(%r); const b = Buffer.from(%r, 'hex');"
              "console.log(typeof a.snapshotStreams, typeof a.restoreStreams, typeof a.snapshotInfo, typeof a.snapshotConcat);"
              "console.log(a.snapshotInfo(b).nStreams, a.snapshotConfig(b, 1).markFrequency, a.snapshotInfo(a.snapshotConcat([b, b])).nStreams);"
              "try { a.restoreStreams(null, b, [0]); } catch (e) { console.log('threw'); }"
              "b[400] ^= 1; try { a.snapshotInfo(b); } catch (e) { console.log(/checksum/.test(e.message) ? 'checksum' : e.message); }"
              % (addon, blob.hex()))
    out = subprocess.run([node, "-e", script], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["function"] * 4 + ["2", "1660", "4", "threw", "checksum"]
