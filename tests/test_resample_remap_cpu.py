"""A resampler through remap, snapshot and restore, without a GPU (include/fskhip_next.h: fskhip_resampler_remap, _snapshot_bytes,
_snapshot, _restore, _snapshot_info_get): the five functions are declared with their signatures, exported and bound on both hosts;
fskhip_resampler_snapshot_info_get reads images crafted by hand here from the documented layout (a 48-byte header, the taps, the rows
packed tightly, zeros to 16 bytes); every refusal that needs no device returns its code and text in the header's order, NULL handles
included; and the host-only validator (csrc/fsk_resample_image.h) walks its cases as a stand-alone program under ASan + UBSan.  No
handle is involved and no kernel is linked into the sanitizer build."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_processor_snapshot_cpu import _checksum, _buf, _flip

NAMES = ["fskhip_resampler_" + f for f in ("remap", "snapshot_bytes", "snapshot", "restore", "snapshot_info_get")]
HEADER = 48
UP, DOWN = 0, 1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from webaudio_modem_amd import _lib
    return _lib


def history(direction, factor, n_taps):
    return -(-(n_taps - 1) // factor) if direction == UP else n_taps - 1


def image(direction=UP, factor=2, n_taps=6, n_records=3, precision=0, rows=None, pad=None, seal=True, **over):
    """a well-formed resampler snapshot; h_<field>=value replaces a header field after the body has been laid out by the real ones
    (the checksum is made over the header as it then stands, so the field's own check is what refuses it)"""
    h = history(direction, factor, n_taps)
    f = dict(magic=0x524B5346, format=1, header_bytes=HEADER, record_bytes=4 * h, n_records=n_records, direction=direction, factor=factor, n_taps=n_taps,
             precision=precision, history=h)
    f.update({k[2:]: v for k, v in over.items() if k.startswith("h_") or pytest.fail(k)})
    taps = np.arange(n_taps, dtype="<f8") * 0.5 - 1.0
    if rows is None:
        rows = (np.arange(n_records * h, dtype="<u4") * np.uint32(2654435761) + np.uint32(0x7FC00001)).view("<f4")   # any word is a history word
    body = taps.tobytes() + np.ascontiguousarray(rows, "<f4").tobytes()
    tail = bytes(-(HEADER + len(body)) % 16) if pad is None else pad
    head = struct.pack("<10IQ", *(f[k] for k in ("magic", "format", "header_bytes", "record_bytes", "n_records", "direction", "factor", "n_taps", "precision", "history")), 0)
    blob = bytearray(head + body + tail)
    if seal and len(blob) % 8 == 0:
        blob[40:48] = struct.pack("<Q", _checksum(blob))
    return bytes(blob)


def _info(lib, blob):
    L = lib.lib()
    info = lib.ResamplerSnapshotInfo()
    rc = L.fskhip_resampler_snapshot_info_get(_buf(blob) if blob is not None else None, len(blob or b""), C.byref(info))
    return rc, L.fskhip_last_error().decode(), info


def _restore(lib, blob, m=None, n=None, out=True):
    L = lib.lib()
    a = None if m is None else np.ascontiguousarray(m, np.int64)
    h = C.c_void_p()
    rc = L.fskhip_resampler_restore(0, _buf(blob) if blob is not None else None, len(blob or b""), None if a is None or not len(a) else a.ctypes.data,
                                    (0 if a is None else len(a)) if n is None else n, C.byref(h) if out else None)
    assert h.value is None      # a refused restore creates nothing
    return rc, L.fskhip_last_error().decode()


def test_the_five_functions_are_declared_exported_and_bound(lib):
    hdr = open(os.path.join(ROOT, "include", "fskhip_next.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    code = re.sub(r"\s+", " ", code)
    L = C.CDLL(lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in lib.SYMBOL_NAMES, name
    for decl in ("int fskhip_resampler_remap(const fskhip_resampler *src, const int64_t *map, uint32_t n_map, fskhip_resampler **out);",
                 "int fskhip_resampler_snapshot_bytes(const fskhip_resampler *r, uint32_t n_sel, size_t *bytes);",
                 "int fskhip_resampler_snapshot(const fskhip_resampler *r, const int64_t *streams, uint32_t n_sel, void *image, size_t cap, size_t *written);",
                 "int fskhip_resampler_restore(int device, const void *image, size_t bytes, const int64_t *map, uint32_t n_map, fskhip_resampler **out);",
                 "int fskhip_resampler_snapshot_info_get(const void *image, size_t bytes, fskhip_resampler_snapshot_info *info);"):
        assert decl in code, decl
    assert "typedef struct fskhip_resampler_snapshot_info {" in code
    assert lib.lib().fskhip_abi_version() == 8
    assert "Snapshot images hold no resampler" not in hdr
    sym = {s[0]: s for s in lib._SYMBOLS}
    P = C.c_void_p
    assert sym["fskhip_resampler_remap"][1:] == (C.c_int, [P, P, C.c_uint32, C.POINTER(P)])
    assert sym["fskhip_resampler_snapshot_bytes"][1:] == (C.c_int, [P, C.c_uint32, C.POINTER(C.c_size_t)])
    assert sym["fskhip_resampler_snapshot"][1:] == (C.c_int, [P, P, C.c_uint32, P, C.c_size_t, C.POINTER(C.c_size_t)])
    assert sym["fskhip_resampler_restore"][1:] == (C.c_int, [C.c_int, P, C.c_size_t, P, C.c_uint32, C.POINTER(P)])
    assert sym["fskhip_resampler_snapshot_info_get"][1:] == (C.c_int, [P, C.c_size_t, C.POINTER(lib.ResamplerSnapshotInfo)])
    import webaudio_modem_amd as wm
    for cls in (wm.Upsampler, wm.Downsampler):
        for meth in ("remapped", "snapshot", "from_snapshot", "state", "set_state"):
            assert callable(getattr(cls, meth)), (cls, meth)
    assert callable(wm.resampler_snapshot_info)
    addon = open(os.path.join(ROOT, "napi", "fsk_addon_next.cc")).read()
    js = open(os.path.join(ROOT, "napi", "filters.js")).read()
    dts = open(os.path.join(ROOT, "napi", "filters.d.ts")).read()
    for f in ("Remap", "Snapshot", "Restore", "SnapshotInfo"):
        assert '"resampler%s"' % f in addon and "addon.resampler%s(" % f in js, f
    for call in ("fskhip_resampler_remap(", "fskhip_resampler_snapshot_bytes(", "fskhip_resampler_snapshot(", "fskhip_resampler_restore(", "fskhip_resampler_snapshot_info_get("):
        assert call in addon, call
    for text in ("remap(map: ArrayLike<number>)", "snapshot(streams?: ArrayLike<number> | null): Buffer;", "export declare function resamplerSnapshotInfo("):
        assert text in dts, text
    assert dts.count("static fromSnapshot(buf: Uint8Array") == 2
    # the sources of the library: the new unit is built, its launch interface is declared once
    mk = open(os.path.join(ROOT, "webaudio_modem_amd", "csrc", "Makefile")).read()
    assert "fsk_resample_remap.hip" in mk and "fsk_resample_image.h" in mk
    assert "launch_resampler_hist_gather(" in open(os.path.join(ROOT, "webaudio_modem_amd", "csrc", "fsk_launch.h")).read()
    kern = open(os.path.join(ROOT, "webaudio_modem_amd", "csrc", "fsk_resample_remap.hip")).read()
    assert "rs_hist_gather_kernel<true>" in kern and "rs_hist_gather_kernel<false>" in kern and "__shared__" not in kern


GOOD = [
    (dict(), (3, UP, 2, 6, 0, 3)),
    (dict(direction=DOWN), (3, DOWN, 2, 6, 0, 5)),
    (dict(factor=3, n_taps=13, n_records=2, precision=1), (2, UP, 3, 13, 1, 4)),
    (dict(direction=DOWN, factor=3, n_taps=13, n_records=1), (1, DOWN, 3, 13, 0, 12)),
    (dict(factor=6, n_taps=97, n_records=5), (5, UP, 6, 97, 0, 16)),
    (dict(direction=DOWN, factor=6, n_taps=97, n_records=2), (2, DOWN, 6, 97, 0, 96)),
    (dict(factor=1, n_taps=1, n_records=9), (9, UP, 1, 1, 0, 0)),
    (dict(direction=DOWN, factor=1, n_taps=1, n_records=0), (0, DOWN, 1, 1, 0, 0)),
    (dict(direction=DOWN, factor=1, n_taps=4096, n_records=1), (1, DOWN, 1, 4096, 0, 4095)),
    (dict(factor=32, n_taps=2, n_records=4), (4, UP, 32, 2, 0, 1)),
]


def test_hand_made_images_are_read_on_the_host(lib):
    for kw, want in GOOD:
        blob = image(**kw)
        rc, msg, info = _info(lib, blob)
        assert rc == 0, (kw, msg)
        assert (info.n_streams, info.direction, info.factor, info.n_taps, info.precision, info.history) == want
        assert len(blob) == (HEADER + 8 * want[3] + 4 * want[0] * want[5] + 15) // 16 * 16
    # an unaligned copy reads the same
    blob = image()
    raw = bytearray(1 + len(blob))
    raw[1:] = blob
    arr = (C.c_char * len(raw)).from_buffer(raw)
    info = lib.ResamplerSnapshotInfo()
    assert lib.lib().fskhip_resampler_snapshot_info_get(C.addressof(arr) + 1, len(blob), C.byref(info)) == 0 and info.n_streams == 3
    import webaudio_modem_amd as wm
    assert wm.resampler_snapshot_info(image(direction=DOWN)) == dict(n_streams=3, direction=DOWN, factor=2, n_taps=6, precision=0, history=5)
    with pytest.raises(wm.FskHipError, match="checksum"):
        wm.resampler_snapshot_info(_flip(image(), HEADER + 3))


LIVE = HEADER + 48 + 36    # image(): 6 taps, 3 rows of 3 floats, then 12 bytes of padding
BAD = [
    ("null", None, "null snapshot"),
    ("empty", lambda: b"", "fewer than a resampler snapshot header"),
    ("short", lambda: image()[:HEADER - 8], "fewer than a resampler snapshot header"),
    ("magic", lambda: image(h_magic=0x584B5346), "not a resampler snapshot"),
    ("format", lambda: image(h_format=2), "format 2"),
    ("header-bytes", lambda: image(h_header_bytes=64), "header_bytes 64"),
    ("direction", lambda: image(h_direction=2), "direction 2"),
    ("factor-0", lambda: image(h_factor=0), "factor 0 outside 1..32"),
    ("factor-33", lambda: image(h_factor=33), "factor 33 outside 1..32"),
    ("taps-0", lambda: image(h_n_taps=0), "n_taps 0 outside 1..4096"),
    ("taps-4097", lambda: image(h_n_taps=4097), "n_taps 4097 outside 1..4096"),
    ("precision", lambda: image(h_precision=2), "precision 2"),
    ("history-other-direction", lambda: image(h_history=5, h_record_bytes=20), "history 5, 6 taps at factor 2 up keep 3"),
    ("history-down", lambda: image(direction=DOWN, h_history=3, h_record_bytes=12), "history 3, 6 taps at factor 2 down keep 5"),
    ("record-bytes", lambda: image(h_record_bytes=16), "record_bytes 16, a row of 3 floats has 12"),
    ("record-count", lambda: image(h_n_records=5), "do not match the layout"),
    ("record-count-huge", lambda: image(h_n_records=0xFFFFFFFF), "do not match the layout"),
    ("truncated", lambda: image()[:-16], "do not match the layout"),
    ("truncated-odd", lambda: image()[:-3], "do not match the layout"),
    ("overlong", lambda: image() + b"\0" * 16, "do not match the layout"),
    ("flipped-header-byte", lambda: _flip(image(), 33), "precision"),
    ("flipped-tap", lambda: _flip(image(), HEADER + 5), "checksum"),
    ("flipped-row", lambda: _flip(image(), HEADER + 48 + 7), "checksum"),
    ("flipped-padding", lambda: _flip(image(), LIVE + 3), "checksum"),
    ("flipped-checksum", lambda: _flip(image(), 41), "checksum"),
    ("padding", lambda: image(pad=b"\0" * 10 + b"\1\0"), "padding byte 10"),
]


@pytest.mark.parametrize("name,make,pattern", BAD, ids=[b[0] for b in BAD])
def test_damaged_images_are_refused_with_a_telling_message(lib, name, make, pattern):
    blob = make() if make else None
    for fn, (rc, msg) in (("fskhip_resampler_snapshot_info_get", _info(lib, blob)[:2]), ("fskhip_resampler_restore", _restore(lib, blob, [0]))):
        assert rc == lib.E_INVALID, (fn, rc, msg)
        assert pattern in msg and fn in msg, (fn, msg)


def test_refusals_come_in_the_headers_order_before_any_device_call(lib):
    L = lib.lib()
    err = lambda: L.fskhip_last_error().decode()
    good = image()
    m = np.array([0, 1], np.int64)
    out = C.c_void_p()
    # (there is no handle without a device: the calls that take one are checked with NULL)
    # remap: a null source, then a null out
    assert L.fskhip_resampler_remap(None, m.ctypes.data, 2, C.byref(out)) == lib.E_INVALID and "fskhip_resampler_remap: null resampler" in err()
    assert L.fskhip_resampler_remap(None, None, 0, None) == lib.E_INVALID and "null resampler" in err()
    assert out.value is None
    # snapshot_bytes, snapshot
    size = C.c_size_t(77)
    assert L.fskhip_resampler_snapshot_bytes(None, 4, C.byref(size)) == lib.E_INVALID and "fskhip_resampler_snapshot_bytes: null resampler" in err()
    assert size.value == 77
    w = C.c_size_t(77)
    buf = (C.c_char * 64)(*([b"\x5a"] * 64))
    assert L.fskhip_resampler_snapshot(None, None, 0, buf, 64, C.byref(w)) == lib.E_INVALID and "fskhip_resampler_snapshot: null resampler" in err()
    assert w.value == 77 and bytes(buf) == b"\x5a" * 64
    # restore: out, then the image, then the map against itself and against the image
    assert L.fskhip_resampler_restore(0, None, 0, None, 0, None) == lib.E_INVALID and "fskhip_resampler_restore: null out" in err()
    rc, msg = _restore(lib, good, [0], out=False)
    assert rc == lib.E_INVALID and "null out" in msg
    rc, msg = _restore(lib, _flip(good, HEADER + 1), [-7])      # the image comes before the map
    assert rc == lib.E_INVALID and "checksum" in msg
    empty = np.zeros(1, np.int64)
    h = C.c_void_p()
    assert L.fskhip_resampler_restore(0, _buf(good), len(good), empty.ctypes.data, 0, C.byref(h)) == lib.E_INVALID and "n_map is 0" in err() and h.value is None
    norec = image(n_records=0)
    assert L.fskhip_resampler_restore(0, _buf(norec), len(norec), None, 5, C.byref(h)) == lib.E_INVALID and "n_map is 0" in err() and h.value is None
    rc, msg = _restore(lib, good, [0, 1, -2, -3])
    assert rc == lib.E_INVALID and "map[2] = -2, the snapshot has 3 records" in msg
    rc, msg = _restore(lib, good, [0, 3, 1])
    assert rc == lib.E_INVALID and "map[1] = 3, the snapshot has 3 records" in msg
    # info_get: the image before the null info
    assert L.fskhip_resampler_snapshot_info_get(_buf(good), len(good), None) == lib.E_INVALID and "null info" in err()
    assert L.fskhip_resampler_snapshot_info_get(_buf(_flip(good, 60)), len(good), None) == lib.E_INVALID and "checksum" in err()
    # a valid image and map reach the device: without one, that is the answer (and no handle)
    if L.fskhip_device_count() == 0:
        rc, msg = _restore(lib, good, [2, -1, 0])
        assert rc == lib.E_NO_DEVICE, msg
    import webaudio_modem_amd as wm
    with pytest.raises(ValueError, match="goes down, not up"):
        wm.Upsampler.from_snapshot(image(direction=DOWN))
    with pytest.raises(ValueError, match="goes up, not down"):
        wm.Downsampler.from_snapshot(image(direction=UP))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rs") / "resample_image_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "webaudio_modem_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "resample_image_check.cpp")],
                   check=True)
    return exe


def test_the_validator_walks_its_cases_as_a_host_program(lib, program):
    good = [image(**kw) for kw, _ in GOOD]
    bad = [(make(), pattern) for _, make, pattern in BAD if make]
    blobs = good + [b for b, _ in bad]
    text = "".join((b.hex() or "-") + "\n" for b in blobs)
    r = subprocess.run([program], input=text, capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.stdout, r.stderr)
    lines = r.stdout.splitlines()
    head, cases = lines[:len(blobs)], lines[len(blobs):]
    # the images of this file: the program's validator and the library's say the same, word for word
    for blob, line in zip(blobs, head):
        rc, msg, info = _info(lib, blob)
        if rc == 0:
            taps = np.frombuffer(blob, "<f8", info.n_taps, HEADER)
            rows = blob[HEADER + 8 * info.n_taps:HEADER + 8 * info.n_taps + 4 * info.n_streams * info.history]
            assert line == "0 %d %d %d %d %d %d %.17g %d" % (info.n_streams, info.direction, info.factor, info.n_taps, info.precision, info.history,
                                                             float(sum(taps.tolist())), sum(rows)), line
        else:
            assert line.startswith("-1 ") and msg == "fskhip_resampler_snapshot_info_get: " + line[3:], (line, msg)
    assert [ln[0] for ln in head[:len(good)]] == ["0"] * len(good)
    for (_, pattern), line in zip(bad, head[len(good):]):
        assert line.startswith("-1 ") and pattern in line, (pattern, line)
    # the images the program builds itself through the header: every case it walks passed, and the list is the issue's
    assert cases and all(re.fullmatch(r"case \S+ ok", ln) for ln in cases), cases
    names = {ln.split()[1] for ln in cases}
    want = {"null", "good-up", "good-down", "good-default-up", "good-default-down", "good-no-history", "good-no-records", "good-longest",
            "cut-at-header", "cut-in-taps", "cut-at-taps", "cut-in-rows", "cut-padding", "overlong", "flip-header", "flip-taps", "flip-rows", "flip-padding",
            "flip-checksum", "magic", "format", "header-bytes", "direction", "precision", "record-count-more", "record-count-fewer", "record-count-huge",
            "history-of-the-other-direction", "history-off-by-one", "record-bytes", "factor-0", "factor-33", "taps-0", "taps-4097", "padding"}
    want |= {"cut-header-%d" % c for c in range(0, HEADER, 4)}
    assert names == want, names ^ want


def test_node_addon_binds_resampler_snapshots():
    node = shutil.which("node")
    addon = os.path.join(ROOT, "napi", "fsk_addon.node")
    import __graft_entry__ as ge
    ge.build()
    if node is None or not os.path.exists(addon):
        pytest.skip("node / the N-API addon not available")
    blob = image(direction=DOWN)
    names = ["resampler" + f for f in ("Remap", "Snapshot", "Restore", "SnapshotInfo")]
    script = ("const a = require(%r); const f = require(%r); const b = Buffer.from(%r, 'hex');"
              "console.log(%s.map((n) => typeof a[n]).join(' '));"
              "const i = f.resamplerSnapshotInfo(b); console.log(i.nStreams, i.direction, i.factor, i.nTaps, i.precision, i.history, Array.from(i.taps).join(','));"
              "try { f.Upsampler.fromSnapshot(b); } catch (e) { console.log(/goes down, not up/.test(e.message) ? 'direction' : e.message); }"
              "try { a.resamplerRestore(b, [0, 5], 0); } catch (e) { console.log(/map\\[1\\] = 5, the snapshot has 3 records/.test(e.message) ? 'map' : e.message); }"
              "try { a.resamplerRestore(b, [], 0); } catch (e) { console.log(/n_map is 0/.test(e.message) ? 'empty' : e.message); }"
              "b[%d] ^= 1; try { f.resamplerSnapshotInfo(b); } catch (e) { console.log(/checksum/.test(e.message) ? 'checksum' : e.message); }"
              % (addon, os.path.join(ROOT, "napi", "filters.js"), blob.hex(), names, HEADER + 3))
    out = subprocess.run([node, "-e", script], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["function"] * 4 + ["3", "1", "2", "6", "0", "5", "-1,-0.5,0,0.5,1,1.5", "direction", "map", "empty", "checksum"]
