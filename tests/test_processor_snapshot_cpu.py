"""Processor remapping and snapshots without a GPU (include/fskhip_next.h): the five functions are declared, exported and bound
on both hosts, fskhip_processor_snapshot_info_get reads an image crafted by hand here from the documented layout (a 48-byte
header, fixed-size records), it and fskhip_processor_restore are loud on every damaged image, and the host-only validator (csrc/fsk_processor_image.h) walks the
same images as a stand-alone program under ASan + UBSan.  No processor is involved."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NAMES = ["fskhip_processor_remap", "fskhip_processor_snapshot_bytes", "fskhip_processor_snapshot", "fskhip_processor_snapshot_info_get",
         "fskhip_processor_restore"]
HEADER = 48
FIXED = 64


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from webaudio_modem_amd import _lib
    return _lib


def _checksum(blob):
    w = np.frombuffer(bytes(blob), dtype="<u8")
    with np.errstate(over="ignore"):
        a = np.cumsum(w, dtype=np.uint64)
        b = np.sum(a, dtype=np.uint64)
        return int((a[-1] * np.uint64(0x9E3779B97F4A7C15)) ^ b)


def _record(rx_cap, pay_cap, ring=b"", read=0, payload=b"", pos=0, total=0, completed=0, pending=None, phase=0.0, cursor=(0, 0, 0)):
    """one canonical record: `ring` is the live content, oldest byte first, starting at index `read`"""
    pending = (1 if payload else 0) if pending is None else pending
    words = struct.pack("<12Id2I", (read + len(ring)) % rx_cap, read, len(ring), pending, completed, pos, total, len(payload), *cursor, 0, phase, 0, 0)
    assert len(words) == FIXED
    store = bytearray((rx_cap + 15) // 16 * 16)
    for i, b in enumerate(ring):
        store[(read + i) % rx_cap] = b
    return words + bytes(payload).ljust(pay_cap, b"\0") + bytes(store)


def _image(records=None, rx_cap=48, pay_cap=16, **over):
    """a well-formed processor snapshot (default: three records -- a drained ring, a wrapped ring, a stream mid-signal)"""
    if records is None:
        records = [_record(rx_cap, pay_cap, completed=2),
                   _record(rx_cap, pay_cap, ring=bytes(range(1, 21)), read=40),
                   _record(rx_cap, pay_cap, ring=b"abc", read=5, payload=b"Hello", pos=300, total=4800, phase=1.25, cursor=(20, 3, 1))]
    rb = FIXED + pay_cap + (rx_cap + 15) // 16 * 16
    f = dict(magic=0x504B5346, format=1, header_bytes=HEADER, record_bytes=rb, n=len(records), rx_cap=rx_cap, pay_cap=pay_cap)
    f.update(over)
    head = struct.pack("<8I2Q", f["magic"], f["format"], f["header_bytes"], f["record_bytes"], f["n"], f["rx_cap"], f["pay_cap"], 0, 0, 0)
    assert len(head) == HEADER
    blob = bytearray(head + b"".join(records))
    blob[32:40] = struct.pack("<Q", _checksum(blob))
    return bytes(blob)


def _buf(b):
    return (C.c_char * max(len(b), 1)).from_buffer_copy(b.ljust(1, b"\0"))


def _info(lib, blob, size=None):
    L = lib.lib()
    info = lib.ProcessorSnapshotInfo()
    rc = L.fskhip_processor_snapshot_info_get(_buf(blob) if blob is not None else None, len(blob or b"") if size is None else size, C.byref(info))
    return rc, L.fskhip_last_error().decode(), info


def _restore(lib, blob, m=(), dst=None):
    L = lib.lib()
    a = np.ascontiguousarray(m, np.int64)
    rc = L.fskhip_processor_restore(dst, _buf(blob) if blob is not None else None, len(blob or b""), a.ctypes.data if len(a) else None, len(a))
    return rc, L.fskhip_last_error().decode()


def _patch(blob, at, data):
    return bytes(blob[:at]) + data + bytes(blob[at + len(data):])


def _flip(blob, at):
    b = bytearray(blob)
    b[at] ^= 0x40
    return bytes(b)


def test_processor_lifecycle_functions_are_declared_exported_and_bound(lib):
    hdr = open(os.path.join(ROOT, "include", "fskhip_next.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = C.CDLL(lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b(int|size_t) %s\(" % name, code), name
        assert hasattr(L, name), name
        assert name in lib.SYMBOL_NAMES, name
    assert "typedef struct fskhip_processor_snapshot_info {" in code
    import webaudio_modem_amd as wm
    for meth in ("remapped", "snapshot", "from_snapshot"):
        assert callable(getattr(wm.FSKProcessorBatch, meth)), meth
    assert callable(wm.processor_snapshot_info)
    addon = open(os.path.join(ROOT, "napi", "fsk_addon_next.cc")).read()
    for call, js_name in (("fskhip_processor_remap(", '"processorRemap"'), ("fskhip_processor_snapshot(", '"processorSnapshot"'),
                          ("fskhip_processor_restore(", '"processorRestore"'), ("fskhip_processor_snapshot_info_get(", '"processorSnapshotInfo"')):
        assert call in addon and js_name in addon, js_name
    js = open(os.path.join(ROOT, "napi", "fsk-processor.js")).read()
    for use in ("addon.processorRemap(", "addon.processorSnapshot(", "addon.processorRestore(", "addon.processorSnapshotInfo(",
                "static fromSnapshot(snap, map, configs, device, options = {})"):
        assert use in js, use
    assert re.search(r"\n  remap\(map, configs\)", js) and re.search(r"\n  snapshot\(streams\)", js)
    dts = open(os.path.join(ROOT, "napi", "fsk-processor.d.ts")).read()
    for decl in ("remap(map: ArrayLike<number>", "snapshot(streams?: ArrayLike<number>): ProcessorBatchSnapshot;", "static fromSnapshot(snap: ProcessorBatchSnapshot",
                 "export declare function processorSnapshotInfo("):
        assert decl in dts, decl


def test_abi_version_stays_8_with_the_processor_additions(lib):
    assert lib.lib().fskhip_abi_version() == 8
    assert hasattr(lib.lib(), "fskhip_processor_remap")


def test_a_hand_made_image_is_read_on_the_host(lib):
    rc, msg, info = _info(lib, _image())
    assert rc == 0, msg
    assert (info.n_streams, info.rx_capacity, info.payload_capacity, info.record_bytes) == (3, 48, 16, 64 + 16 + 48)
    rc, msg, info = _info(lib, _image([], rx_cap=1024, pay_cap=0))
    assert rc == 0 and (info.n_streams, info.rx_capacity, info.payload_capacity, info.record_bytes) == (0, 1024, 0, 64 + 1024), msg
    # a capacity that is no multiple of 16: the ring is padded with zeros to the next one
    rc, msg, info = _info(lib, _image([_record(50, 0, ring=b"xyz", read=49)], rx_cap=50, pay_cap=0))
    assert rc == 0 and info.record_bytes == 64 + 64, msg
    # an unaligned copy reads the same
    blob = _image()
    raw = bytearray(1 + len(blob))
    raw[1:] = blob
    arr = (C.c_char * len(raw)).from_buffer(raw)
    info = lib.ProcessorSnapshotInfo()
    assert lib.lib().fskhip_processor_snapshot_info_get(C.addressof(arr) + 1, len(blob), C.byref(info)) == 0 and info.n_streams == 3
    import webaudio_modem_amd as wm
    assert wm.processor_snapshot_info(blob) == dict(n_streams=3, rx_capacity=48, payload_capacity=16, record_bytes=128)
    with pytest.raises(wm.FskHipError, match="checksum"):
        wm.processor_snapshot_info(_flip(blob, HEADER + FIXED + 2))


BAD = [
    ("null", None, "null snapshot"),
    ("short", lambda: _image()[:HEADER - 8], "fewer than a processor snapshot header"),
    ("magic", lambda: _image(magic=0x534B5346), "magic"),
    ("format", lambda: _image(format=7), "format 7"),
    ("header-bytes", lambda: _image(header_bytes=64), "header_bytes 64"),
    ("record-bytes", lambda: _image(record_bytes=128 + 16), "record_bytes 144"),
    ("record-count", lambda: _image(n=4), "do not match n_records x record_bytes"),
    ("payload-capacity", lambda: _image(pay_cap=8), "payload_capacity 8"),
    ("truncated", lambda: _image()[:-16], "do not match n_records x record_bytes"),
    ("overlong", lambda: _image() + b"\0" * 8, "do not match n_records x record_bytes"),
    ("flipped-payload-byte", lambda: _flip(_image(), HEADER + 2 * 128 + FIXED + 1), "checksum"),
    ("flipped-header-byte", lambda: _flip(_image(), 42), "checksum"),
    ("read-index", lambda: _image([_record(48, 16, ring=b"ab", read=48)]), "record 0: ring words"),
    ("payload-length", lambda: _image([_record(48, 16), _patch(_record(48, 16, payload=b"x" * 16, total=99), 28, struct.pack("<I", 17))]), "record 1: modulator words"),
]


@pytest.mark.parametrize("name,make,pattern", BAD, ids=[b[0] for b in BAD])
def test_damaged_images_are_refused_with_a_telling_message(lib, name, make, pattern):
    blob = make() if make else None
    for fn, call in (("fskhip_processor_snapshot_info_get", lambda: _info(lib, blob)[:2]),
                     ("fskhip_processor_restore", lambda: _restore(lib, blob, [0, 1]))):
        rc, msg = call()
        assert rc == lib.E_INVALID, (fn, rc, msg)
        assert pattern in msg and fn in msg, (fn, msg)


def build_image_check(tmp_path_factory):
    """tests/cpp/snapshot_image_check.cpp (the stream and processor snapshots' host-only validators) under ASan + UBSan: no library"""
    exe = str(tmp_path_factory.mktemp("si") / "snapshot_image_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "webaudio_modem_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "snapshot_image_check.cpp")],
                   check=True)
    return exe


def walk_images(program, kind, blobs):
    """the program's line for each image of one kind (None: no image at all)"""
    text = "".join("%s %s\n" % (kind, "null" if b is None else b.hex() or "-") for b in blobs)
    r = subprocess.run([program], input=text, capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.stdout, r.stderr)
    lines = r.stdout.splitlines()
    assert len(lines) == len(blobs)
    return lines


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build_image_check(tmp_path_factory)


def test_the_validator_walks_the_same_images_as_a_host_program(lib, program):
    good = [_image(), _image([], rx_cap=1024, pay_cap=0), _image([_record(50, 0, ring=b"xyz", read=49)], rx_cap=50, pay_cap=0)]
    bad = [(make() if make else None, pattern) for _, make, pattern in BAD]
    blobs = good + [b for b, _ in bad]
    lines = walk_images(program, "P", blobs)
    for blob, line in zip(blobs, lines):
        rc, msg, info = _info(lib, blob)
        if rc == 0:
            assert line == "0 %d %d %d %d %d" % (info.n_streams, info.rx_capacity, info.payload_capacity, info.record_bytes, sum(blob[HEADER:])), line
        else:
            assert line.startswith("-1 ") and msg == "fskhip_processor_snapshot_info_get: " + line[3:], (line, msg)
    assert [ln[0] for ln in lines[:len(good)]] == ["0"] * len(good)
    for (_, pattern), line in zip(bad, lines[len(good):]):
        assert line.startswith("-1 ") and pattern in line, (pattern, line)


def test_device_calls_fail_loudly_without_a_processor(lib):
    L = lib.lib()
    w = C.c_size_t(0)
    assert L.fskhip_processor_snapshot(None, None, 0, (C.c_char * 64)(), 64, C.byref(w)) == lib.E_INVALID
    assert "null processor" in L.fskhip_last_error().decode()
    assert L.fskhip_processor_snapshot_bytes(None, None, 4) == 0
    assert L.fskhip_processor_remap(None, None, None, 0) == lib.E_INVALID
    assert "null processor" in L.fskhip_last_error().decode()
    rc, msg = _restore(lib, _image(), [0, 1, 2])
    assert rc == lib.E_INVALID and "null processor" in msg
    rc, msg = _restore(lib, _image(), [0, 1, -2, -3])
    assert rc == lib.E_INVALID and "map[2] = -2" in msg          # the first offending index, as the remap names it
    assert L.fskhip_processor_restore(None, _buf(_image()), len(_image()), None, 4) == lib.E_INVALID
    assert "null map" in L.fskhip_last_error().decode()
    assert L.fskhip_processor_snapshot_info_get(_buf(_image()), len(_image()), None) == lib.E_INVALID
    assert "null info" in L.fskhip_last_error().decode()
    if L.fskhip_device_count() == 0:
        # no device: a processor needs an engine, and an engine needs a GPU -- there is no CPU path to fall back to
        import webaudio_modem_amd as wm
        with pytest.raises(wm.FskHipError) as ei:
            wm.FSKEngine(2, {})
        assert ei.value.code == lib.E_NO_DEVICE


def test_node_addon_binds_processor_snapshots():
    node = shutil.which("node")
    addon = os.path.join(ROOT, "napi", "fsk_addon.node")
    import __graft_entry__ as ge
    ge.build()
    if node is None or not os.path.exists(addon):
        pytest.skip("node / the N-API addon not available")
    blob = _image()
    script = ("const a = require(%r); const b = Buffer.from(%r, 'hex');"
              "console.log(typeof a.processorRemap, typeof a.processorSnapshot, typeof a.processorRestore, typeof a.processorSnapshotInfo);"
              "const i = a.processorSnapshotInfo(b); console.log(i.nStreams, i.rxCapacity, i.payloadCapacity, i.recordBytes);"
              "try { a.processorRestore(null, b, [0]); } catch (e) { console.log('threw'); }"
              "b[%d] ^= 1; try { a.processorSnapshotInfo(b); } catch (e) { console.log(/checksum/.test(e.message) ? 'checksum' : e.message); }"
              % (addon, blob.hex(), HEADER + FIXED + 3))
    out = subprocess.run([node, "-e", script], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["function"] * 4 + ["3", "48", "16", "128", "threw", "checksum"]
