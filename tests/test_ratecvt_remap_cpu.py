"""A rate converter through remap, snapshot and restore, without a GPU (include/fskhip_next.h: fskhip_ratecvt_remap, _snapshot_bytes,
_snapshot, _restore, _snapshot_info_get): the five functions are declared with their signatures, exported and bound on both hosts;
fskhip_ratecvt_snapshot_info_get reads images crafted by hand here from the documented layout (a 64-byte header, the taps, the rows
packed tightly, zeros to 16 bytes); every refusal that needs no device returns its code and text in the header's order, NULL handles
included; CaptureConverter / PlaybackConverter refuse an image of the other direction and rates of another ratio; and the host-only
validator (csrc/fsk_ratecvt_image.h) walks its cases as a stand-alone program under ASan + UBSan.  No handle is involved and no
kernel is linked into the sanitizer build."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_processor_snapshot_cpu import _checksum, _buf, _flip

NAMES = ["fskhip_ratecvt_" + f for f in ("remap", "snapshot_bytes", "snapshot", "restore", "snapshot_info_get")]
HEADER = 64
CAPTURE, PLAYBACK = 0, 1
FIELDS = ("magic", "format", "header_bytes", "record_bytes", "n_records", "direction", "up", "down", "n_taps", "precision", "history", "position",
          "reserved0", "reserved1")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from webaudio_modem_amd import _lib
    return _lib


def history(up, n_taps):
    return -(-(n_taps - 1) // up)


def image(direction=CAPTURE, up=2, down=3, n_taps=6, n_records=3, precision=0, position=2, rows=None, pad=None, seal=True, **over):
    """a well-formed rate converter snapshot; h_<field>=value replaces a header field after the body has been laid out by the real
    ones (the checksum is made over the header as it then stands, so the field's own check is what refuses it)"""
    h = history(up, n_taps)
    f = dict(magic=0x434B5346, format=1, header_bytes=HEADER, record_bytes=4 * h, n_records=n_records, direction=direction, up=up, down=down, n_taps=n_taps,
             precision=precision, history=h, position=position, reserved0=0, reserved1=0)
    f.update({k[2:]: v for k, v in over.items() if k.startswith("h_") or pytest.fail(k)})
    taps = np.arange(n_taps, dtype="<f8") * 0.5 - 1.0
    if rows is None:
        rows = (np.arange(n_records * h, dtype="<u4") * np.uint32(2654435761) + np.uint32(0x7FC00001)).view("<f4")   # any word is a history word
    body = taps.tobytes() + np.ascontiguousarray(rows, "<f4").tobytes()
    tail = bytes(-(HEADER + len(body)) % 16) if pad is None else pad
    head = struct.pack("<14IQ", *(f[k] for k in FIELDS), 0)
    blob = bytearray(head + body + tail)
    if seal and len(blob) % 8 == 0:
        blob[56:64] = struct.pack("<Q", _checksum(blob))
    return bytes(blob)


def resampler_image():
    """a resampler's snapshot of 6 taps at factor 2 up and 3 records (include/fskhip_next.h: "FSKR", a 48-byte header)"""
    head = struct.pack("<10IQ", 0x524B5346, 1, 48, 12, 3, 0, 2, 6, 0, 3, 0)
    blob = bytearray(head + bytes(48 + 36) + bytes(12))
    blob[40:48] = struct.pack("<Q", _checksum(blob))
    return bytes(blob)


def _info(lib, blob):
    L = lib.lib()
    info = lib.RatecvtSnapshotInfo()
    rc = L.fskhip_ratecvt_snapshot_info_get(_buf(blob) if blob is not None else None, len(blob or b""), C.byref(info))
    return rc, L.fskhip_last_error().decode(), info


def _restore(lib, blob, m=None, n=None, out=True):
    L = lib.lib()
    a = None if m is None else np.ascontiguousarray(m, np.int64)
    h = C.c_void_p()
    rc = L.fskhip_ratecvt_restore(0, _buf(blob) if blob is not None else None, len(blob or b""), None if a is None or not len(a) else a.ctypes.data,
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
    for decl in ("int fskhip_ratecvt_remap(const fskhip_ratecvt *src, const int64_t *map, uint32_t n_map, fskhip_ratecvt **out);",
                 "int fskhip_ratecvt_snapshot_bytes(const fskhip_ratecvt *r, uint32_t n_sel, size_t *bytes);",
                 "int fskhip_ratecvt_snapshot(const fskhip_ratecvt *r, const int64_t *streams, uint32_t n_sel, void *image, size_t cap, size_t *written);",
                 "int fskhip_ratecvt_restore(int device, const void *image, size_t bytes, const int64_t *map, uint32_t n_map, fskhip_ratecvt **out);",
                 "int fskhip_ratecvt_snapshot_info_get(const void *image, size_t bytes, fskhip_ratecvt_snapshot_info *info);"):
        assert decl in code, decl
    assert "typedef struct fskhip_ratecvt_snapshot_info {" in code
    assert lib.lib().fskhip_abi_version() == 8
    assert "These handles have no remap, snapshot or restore yet" not in hdr
    sym = {s[0]: s for s in lib._SYMBOLS}
    P = C.c_void_p
    assert sym["fskhip_ratecvt_remap"][1:] == (C.c_int, [P, P, C.c_uint32, C.POINTER(P)])
    assert sym["fskhip_ratecvt_snapshot_bytes"][1:] == (C.c_int, [P, C.c_uint32, C.POINTER(C.c_size_t)])
    assert sym["fskhip_ratecvt_snapshot"][1:] == (C.c_int, [P, P, C.c_uint32, P, C.c_size_t, C.POINTER(C.c_size_t)])
    assert sym["fskhip_ratecvt_restore"][1:] == (C.c_int, [C.c_int, P, C.c_size_t, P, C.c_uint32, C.POINTER(P)])
    assert sym["fskhip_ratecvt_snapshot_info_get"][1:] == (C.c_int, [P, C.c_size_t, C.POINTER(lib.RatecvtSnapshotInfo)])
    assert [f[0] for f in lib.RatecvtSnapshotInfo._fields_] == ["n_streams", "direction", "up", "down", "n_taps", "precision", "history", "position"]
    import webaudio_modem_amd as wm
    for cls in (wm.CaptureConverter, wm.PlaybackConverter):
        for meth in ("remapped", "snapshot", "from_snapshot", "state", "set_state", "_adopt"):
            assert callable(getattr(cls, meth)), (cls, meth)
    assert callable(wm.ratecvt_snapshot_info)
    addon = open(os.path.join(ROOT, "napi", "fsk_addon_next.cc")).read()
    js = open(os.path.join(ROOT, "napi", "filters.js")).read()
    dts = open(os.path.join(ROOT, "napi", "filters.d.ts")).read()
    for f in ("Remap", "Snapshot", "Restore", "SnapshotInfo"):
        assert '"ratecvt%s"' % f in addon and "addon.ratecvt%s(" % f in js, f
    for call in ("fskhip_ratecvt_remap(", "fskhip_ratecvt_snapshot_bytes(", "fskhip_ratecvt_snapshot(", "fskhip_ratecvt_restore(", "fskhip_ratecvt_snapshot_info_get("):
        assert call in addon, call
    assert "export declare function ratecvtSnapshotInfo(" in dts and "static fromSnapshot(image: Uint8Array" in dts


GOOD = [
    (dict(), (3, CAPTURE, 2, 3, 6, 0, 3, 2)),
    (dict(direction=PLAYBACK, position=0), (3, PLAYBACK, 2, 3, 6, 0, 3, 0)),
    (dict(up=3, down=2, n_taps=13, n_records=2, precision=1, position=1), (2, CAPTURE, 3, 2, 13, 1, 4, 1)),
    (dict(direction=PLAYBACK, up=1, down=1, n_taps=1, n_records=9, position=0), (9, PLAYBACK, 1, 1, 1, 0, 0, 0)),
    (dict(up=160, down=147, n_taps=2561, n_records=5, position=146), (5, CAPTURE, 160, 147, 2561, 0, 16, 146)),
    (dict(direction=PLAYBACK, up=147, down=160, n_taps=2561, n_records=2, position=128), (2, PLAYBACK, 147, 160, 2561, 0, 18, 128)),
    (dict(up=3, down=2, n_taps=13, n_records=0, position=0), (0, CAPTURE, 3, 2, 13, 0, 4, 0)),
    (dict(direction=PLAYBACK, up=1, down=256, n_taps=4096, n_records=1, position=255), (1, PLAYBACK, 1, 256, 4096, 0, 4095, 255)),
    (dict(up=256, down=255, n_taps=2, n_records=4, position=254), (4, CAPTURE, 256, 255, 2, 0, 1, 254)),
]


def test_hand_made_images_are_read_on_the_host(lib):
    for kw, want in GOOD:
        blob = image(**kw)
        rc, msg, info = _info(lib, blob)
        assert rc == 0, (kw, msg)
        assert (info.n_streams, info.direction, info.up, info.down, info.n_taps, info.precision, info.history, info.position) == want
        assert len(blob) == (HEADER + 8 * want[4] + 4 * want[0] * want[6] + 15) // 16 * 16
    # an unaligned copy reads the same
    blob = image()
    raw = bytearray(1 + len(blob))
    raw[1:] = blob
    arr = (C.c_char * len(raw)).from_buffer(raw)
    info = lib.RatecvtSnapshotInfo()
    assert lib.lib().fskhip_ratecvt_snapshot_info_get(C.addressof(arr) + 1, len(blob), C.byref(info)) == 0 and info.n_streams == 3
    import webaudio_modem_amd as wm
    assert wm.ratecvt_snapshot_info(image(direction=PLAYBACK)) == dict(n_streams=3, direction=PLAYBACK, up=2, down=3, n_taps=6, precision=0, history=3,
                                                                        position=2)
    with pytest.raises(wm.FskHipError, match="checksum"):
        wm.ratecvt_snapshot_info(_flip(image(), HEADER + 3))


LIVE = HEADER + 48 + 36    # image(): 6 taps, 3 rows of 3 floats, then 12 bytes of padding
BAD = [   # in the header's order of refusals
    ("null", None, "null snapshot"),
    ("empty", lambda: b"", "fewer than a rate converter snapshot header"),
    ("short", lambda: image()[:HEADER - 8], "fewer than a rate converter snapshot header"),
    ("magic", lambda: image(h_magic=0x584B5346), "not a rate converter snapshot"),
    ("magic-resampler", resampler_image, "is a resampler snapshot's"),
    ("format", lambda: image(h_format=2), "format 2"),
    ("header-bytes", lambda: image(h_header_bytes=48), "header_bytes 48"),
    ("reserved-0", lambda: image(h_reserved0=1), "reserved words 0x00000001 0x00000000 are not zero"),
    ("reserved-1", lambda: image(h_reserved1=2), "reserved words 0x00000000 0x00000002 are not zero"),
    ("direction", lambda: image(h_direction=2), "direction 2"),
    ("up-0", lambda: image(h_up=0), "up 0 outside 1..256"),
    ("up-257", lambda: image(h_up=257), "up 257 outside 1..256"),
    ("down-0", lambda: image(h_down=0), "down 0 outside 1..256"),
    ("down-257", lambda: image(h_down=257), "down 257 outside 1..256"),
    ("lowest-terms", lambda: image(h_down=4), "2 / 4 is not in lowest terms"),
    ("taps-0", lambda: image(h_n_taps=0), "n_taps 0 outside 1..4096"),
    ("taps-4097", lambda: image(h_n_taps=4097), "n_taps 4097 outside 1..4096"),
    ("precision", lambda: image(h_precision=2), "precision 2"),
    ("history-of-a-decimator", lambda: image(h_history=5, h_record_bytes=20), "history 5, 6 taps at an up factor of 2 keep 3"),
    ("position", lambda: image(h_position=3), "position 3 is not below the down factor 3"),
    ("record-bytes", lambda: image(h_record_bytes=16), "record_bytes 16, a row of 3 floats has 12"),
    ("record-count", lambda: image(h_n_records=5), "do not match the layout"),
    ("record-count-huge", lambda: image(h_n_records=0xFFFFFFFF), "do not match the layout"),
    ("truncated", lambda: image()[:-16], "do not match the layout"),
    ("truncated-odd", lambda: image()[:-3], "do not match the layout"),
    ("overlong", lambda: image() + b"\0" * 16, "do not match the layout"),
    ("flipped-header-byte", lambda: _flip(image(), 37), "precision"),
    ("flipped-tap", lambda: _flip(image(), HEADER + 5), "checksum"),
    ("flipped-row", lambda: _flip(image(), HEADER + 48 + 7), "checksum"),
    ("flipped-padding", lambda: _flip(image(), LIVE + 3), "checksum"),
    ("flipped-checksum", lambda: _flip(image(), 57), "checksum"),
    ("padding", lambda: image(pad=b"\0" * 10 + b"\1\0"), "padding byte 10"),
]


@pytest.mark.parametrize("name,make,pattern", BAD, ids=[b[0] for b in BAD])
def test_damaged_images_are_refused_with_a_telling_message(lib, name, make, pattern):
    blob = make() if make else None
    for fn, (rc, msg) in (("fskhip_ratecvt_snapshot_info_get", _info(lib, blob)[:2]), ("fskhip_ratecvt_restore", _restore(lib, blob, [0]))):
        assert rc == lib.E_INVALID, (fn, rc, msg)
        assert pattern in msg and fn in msg, (fn, msg)


def test_refusals_come_in_the_headers_order_before_any_device_call(lib):
    L = lib.lib()
    err = lambda: L.fskhip_last_error().decode()
    good = image()
    m = np.array([0, 1], np.int64)
    out = C.c_void_p()
    # (there is no handle without a device: the calls that take one are checked with NULL)
    assert L.fskhip_ratecvt_remap(None, m.ctypes.data, 2, C.byref(out)) == lib.E_INVALID and "fskhip_ratecvt_remap: null rate converter" in err()
    assert L.fskhip_ratecvt_remap(None, None, 0, None) == lib.E_INVALID and "null rate converter" in err()
    assert out.value is None
    size = C.c_size_t(77)
    assert L.fskhip_ratecvt_snapshot_bytes(None, 4, C.byref(size)) == lib.E_INVALID and "fskhip_ratecvt_snapshot_bytes: null rate converter" in err()
    assert size.value == 77
    w = C.c_size_t(77)
    buf = (C.c_char * 64)(*([b"\x5a"] * 64))
    assert L.fskhip_ratecvt_snapshot(None, None, 0, buf, 64, C.byref(w)) == lib.E_INVALID and "fskhip_ratecvt_snapshot: null rate converter" in err()
    assert w.value == 77 and bytes(buf) == b"\x5a" * 64
    # restore: out, then the image, then the map against itself and against the image
    assert L.fskhip_ratecvt_restore(0, None, 0, None, 0, None) == lib.E_INVALID and "fskhip_ratecvt_restore: null out" in err()
    rc, msg = _restore(lib, good, [0], out=False)
    assert rc == lib.E_INVALID and "null out" in msg
    rc, msg = _restore(lib, _flip(good, HEADER + 1), [-7])      # the image comes before the map
    assert rc == lib.E_INVALID and "checksum" in msg
    empty = np.zeros(1, np.int64)
    h = C.c_void_p()
    assert L.fskhip_ratecvt_restore(0, _buf(good), len(good), empty.ctypes.data, 0, C.byref(h)) == lib.E_INVALID and "n_map is 0: a rate converter" in err()
    assert h.value is None
    norec = image(n_records=0)
    assert L.fskhip_ratecvt_restore(0, _buf(norec), len(norec), None, 5, C.byref(h)) == lib.E_INVALID and "n_map is 0" in err() and h.value is None
    rc, msg = _restore(lib, good, [0, 1, -2, -3])
    assert rc == lib.E_INVALID and "map[2] = -2, the snapshot has 3 records" in msg
    rc, msg = _restore(lib, good, [0, 3, 1])
    assert rc == lib.E_INVALID and "map[1] = 3, the snapshot has 3 records" in msg
    # info_get: the image before the null info
    assert L.fskhip_ratecvt_snapshot_info_get(_buf(good), len(good), None) == lib.E_INVALID and "null info" in err()
    assert L.fskhip_ratecvt_snapshot_info_get(_buf(_flip(good, 70)), len(good), None) == lib.E_INVALID and "checksum" in err()
    # an image with several flaws is refused for the first of the header's order
    for kw, pattern in ((dict(h_format=2, h_header_bytes=48, h_direction=2), "format 2"), (dict(h_header_bytes=48, h_reserved0=1), "header_bytes 48"),
                        (dict(h_reserved1=1, h_direction=2), "reserved words"), (dict(h_direction=2, h_up=0), "direction 2"), (dict(h_up=0, h_down=0), "up 0"),
                        (dict(h_down=0, h_n_taps=0), "down 0"), (dict(h_down=4, h_n_taps=0), "lowest terms"), (dict(h_n_taps=0, h_precision=2), "n_taps 0"),
                        (dict(h_precision=2, h_history=9), "precision 2"), (dict(h_history=9, h_position=3), "history 9"),
                        (dict(h_position=3, h_record_bytes=16), "position 3"), (dict(h_record_bytes=16, h_n_records=5), "record_bytes 16")):
        rc, msg, _ = _info(lib, image(**kw))
        assert rc == lib.E_INVALID and pattern in msg, (kw, msg)
    rc, msg, _ = _info(lib, _flip(image(h_n_records=5), HEADER + 1))          # the size before the checksum
    assert rc == lib.E_INVALID and "do not match the layout" in msg
    rc, msg, _ = _info(lib, _flip(image(pad=b"\0" * 10 + b"\1\0"), HEADER + 1))   # the checksum before the padding
    assert rc == lib.E_INVALID and "checksum" in msg
    # a valid image and map reach the device: without one, that is the answer (and no handle)
    if L.fskhip_device_count() == 0:
        rc, msg = _restore(lib, good, [2, -1, 0])
        assert rc == lib.E_NO_DEVICE, msg


def test_the_classes_refuse_the_other_direction_and_rates_of_another_ratio(lib):
    import webaudio_modem_amd as wm
    from webaudio_modem_amd.filters import _RateConverter
    with pytest.raises(ValueError, match="for playback, not capture"):
        wm.CaptureConverter.from_snapshot(image(direction=PLAYBACK))
    with pytest.raises(ValueError, match="for capture, not playback"):
        wm.PlaybackConverter.from_snapshot(image(direction=CAPTURE))
    default = image(up=160, down=147, n_taps=2561, n_records=2, position=128)
    for cls in (wm.CaptureConverter, _RateConverter):
        with pytest.raises(ValueError, match="is 147 / 160, the snapshot converts by 160 / 147"):
            cls.from_snapshot(default, in_rate=48000, out_rate=44100)
        with pytest.raises(ValueError, match="is 6 / 1, the snapshot converts by 160 / 147"):
            cls.from_snapshot(default, in_rate=8000, out_rate=48000)
        with pytest.raises(ValueError, match="both in_rate and out_rate"):
            cls.from_snapshot(default, in_rate=44100)
        with pytest.raises(ValueError, match="whole numbers"):
            cls.from_snapshot(default, in_rate=44100.5, out_rate=48000)
    with pytest.raises(wm.FskHipError, match="checksum"):       # the image is looked at first
        wm.PlaybackConverter.from_snapshot(_flip(default, HEADER + 9), in_rate=1, out_rate=2)
    # rates that fit pass the host's checks: what is left is the device's answer
    if lib.lib().fskhip_device_count() == 0:
        for kw in (dict(in_rate=44100, out_rate=48000), dict(in_rate=147, out_rate=160), dict()):
            with pytest.raises(wm.FskHipError) as e:
                _RateConverter.from_snapshot(default, **kw)
            assert e.value.code == lib.E_NO_DEVICE


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rc") / "ratecvt_image_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "webaudio_modem_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "ratecvt_image_check.cpp")],
                   check=True)
    return exe


def test_the_validator_walks_its_cases_as_a_host_program(lib, program):
    good = [image(**kw) for kw, _ in GOOD]
    bad = [(make(), pattern) for _, make, pattern in BAD if make]
    bad.append((image()[:HEADER + 21], "do not match the layout"))        # a truncated buffer, at the program's odd address
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
            assert line == "0 %d %d %d %d %d %d %d %d %.17g %d" % (info.n_streams, info.direction, info.up, info.down, info.n_taps, info.precision, info.history,
                                                                   info.position, float(sum(taps.tolist())), sum(rows)), line
        else:
            assert line.startswith("-1 ") and msg == "fskhip_ratecvt_snapshot_info_get: " + line[3:], (line, msg)
    assert [ln[0] for ln in head[:len(good)]] == ["0"] * len(good)
    for (_, pattern), line in zip(bad, head[len(good):]):
        assert line.startswith("-1 ") and pattern in line, (pattern, line)
    # the images the program builds itself through the layout functions: every case it walks passed, and the list is this
    assert cases and all(re.fullmatch(r"case \S+ ok", ln) for ln in cases), cases
    names = {ln.split()[1] for ln in cases}
    want = {"null", "good-capture", "good-playback", "good-default-capture", "good-default-playback", "good-no-history", "good-no-records", "good-longest",
            "cut-at-header", "cut-in-taps", "cut-at-taps", "cut-in-rows", "cut-padding", "overlong", "flip-header", "flip-taps", "flip-rows", "flip-padding",
            "flip-checksum", "magic", "magic-resampler", "resampler-truncated", "format", "header-bytes", "reserved-0", "reserved-1", "direction", "up-0", "up-257",
            "down-0", "down-257", "lowest-terms", "taps-0", "taps-4097", "precision", "history-of-a-decimator", "history-off-by-one", "position-at-down",
            "position-huge", "record-bytes", "record-count-more", "record-count-fewer", "record-count-huge", "padding", "order-size", "order-checksum"}
    want |= {"cut-header-%d" % c for c in range(0, HEADER, 4)}
    want |= {"order-" + n for n in ("magic", "format", "header-bytes", "reserved", "direction", "up", "down", "taps", "precision", "history", "position", "record-bytes")}
    assert names == want, names ^ want
