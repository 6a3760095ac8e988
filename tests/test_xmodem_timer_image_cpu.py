"""The XModem wait timers' snapshot image ("FSKW", include/fskhip_next.h) without a GPU: images built here in numpy from the
documented format are accepted by fskhip_xmodem_timer_snapshot_info_get and every listed flaw is refused by name; the one
validator (csrc/fsk_xmodem_timer_image.h) as a host program under ASan + UBSan over every truncation and every single-byte
corruption of an image (tests/cpp/xmodem_timer_image_check.cpp); and the refusals of the five calls that need no device."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_processor_snapshot_cpu import _checksum, _buf

NAMES = ["fskhip_xmodem_timer_" + n for n in ("snapshot_info_get", "remap", "snapshot_bytes", "snapshot", "restore")]
MAGIC, XM_MAGIC, HEADER = 0x574B5346, 0x584B5346, 48
TX, RECV = 2, 3


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from webaudio_modem_amd import _lib
    _lib.lib()
    return _lib


def _image(kind, records, timeout=12288, pad=None, cut=0, **over):
    """a well-formed timer snapshot of `records` (waited, mark); `over` replaces header fields, `pad` the padding, `cut` drops
    bytes off the end before the checksum is taken"""
    f = dict(magic=MAGIC, format=1, header_bytes=HEADER, kind=kind, n=len(records), record_words=2, timeout=timeout, res0=0, res1=0)
    f.update(over)
    head = struct.pack("<8I2Q", f["magic"], f["format"], f["header_bytes"], f["kind"], f["n"], f["record_words"], f["timeout"], f["res0"], 0, f["res1"])
    table = b"".join(struct.pack("<2I", w, m) for w, m in records)
    tail = bytes(-(HEADER + len(table)) % 16) if pad is None else pad
    blob = bytearray(head + table + tail)
    if cut:
        del blob[-cut:]
    blob[32:40] = struct.pack("<Q", _checksum(blob))
    return bytes(blob)


def _info(lib, blob):
    L = lib.lib()
    info = lib.XModemTimerSnapshotInfo()
    rc = L.fskhip_xmodem_timer_snapshot_info_get(_buf(blob) if blob is not None else None, len(blob or b""), C.byref(info))
    return rc, L.fskhip_last_error().decode(), info


RECV_RECORDS = [(0, 0), (1, 1), (12287, 2), (12288, 4), (0xFFFFFFFF, 5), (77, 6)]
TX_RECORDS = [(0, 0), (8191, 4), (0xFFFFFFFF, 0)]


def test_the_five_functions_are_declared_exported_and_bound(lib):
    import re
    hdr = open(os.path.join(ROOT, "include", "fskhip_next.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = C.CDLL(lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b(int|size_t) +%s\(" % name, code), name
        assert hasattr(L, name) and name in lib.SYMBOL_NAMES, name
    assert "typedef struct fskhip_xmodem_timer_snapshot_info {" in code
    assert "#define FSKHIP_ABI_VERSION 8" in open(os.path.join(ROOT, "include", "fskhip.h")).read() + hdr
    import webaudio_modem_amd as wm
    assert all(callable(getattr(wm.XModemTimers, m)) for m in ("remapped", "snapshot", "from_snapshot")) and callable(wm.xmodem_timer_snapshot_info)
    assert "set_state" not in wm.XModemTimers.__doc__ and "from_snapshot" in wm.XModemTimers.__doc__


@pytest.mark.parametrize("kind,records,timeout", [(RECV, RECV_RECORDS, 12288), (TX, TX_RECORDS, 8192), (RECV, [], 1), (TX, [(5, 4)], 0xFFFFFFFF)])
def test_images_built_from_the_documented_format_are_accepted(lib, kind, records, timeout):
    blob = _image(kind, records, timeout)
    assert len(blob) == (HEADER + 8 * len(records) + 15) // 16 * 16
    rc, msg, info = _info(lib, blob)
    assert rc == 0, msg
    assert (info.kind, info.n_streams, info.timeout_samples, info.reserved) == (kind, len(records), timeout, 0)
    import webaudio_modem_amd as wm
    assert wm.xmodem_timer_snapshot_info(blob) == dict(kind=kind, n_streams=len(records), timeout_samples=timeout, reserved=0)


THREE = [(10, 0), (20, 2), (30, 4)]
FLAWS = [
    # (name, image, what the message must say)
    ("magic", _image(RECV, THREE, magic=0x12345678), "not an XModem timer snapshot (magic 0x12345678"),
    ("an FSKX image", _image(RECV, THREE, magic=XM_MAGIC), "is an XModem handle's snapshot's"),
    ("format", _image(RECV, THREE, format=2), "format 2, this library reads format 1"),
    ("header_bytes", _image(RECV, THREE, header_bytes=64), "header_bytes 64, expected 48"),
    ("kind 1", _image(1, THREE), "kind 1 is neither 2 (tx) nor 3 (recv)"),
    ("kind 4", _image(4, THREE), "kind 4 is neither 2 (tx) nor 3 (recv)"),
    ("record_words", _image(RECV, THREE, record_words=8), "record_words 8, a timer record has 2"),
    ("timeout_samples", _image(RECV, THREE, timeout=0), "timeout_samples is 0"),
    ("the reserved word", _image(RECV, THREE, res0=1), "reserved header fields 0x00000001 0x0000000000000000 are not zero"),
    ("the reserved quad", _image(RECV, THREE, res1=1 << 40), "reserved header fields 0x00000000 0x0000010000000000 are not zero"),
    ("a 3-record image truncated by 8 bytes", _image(RECV, THREE, cut=8), "72 bytes do not match the layout (48 + 8 x n_records 3, rounded up to 16)"),
    ("a count that the size does not hold", _image(RECV, THREE, n=5), "80 bytes do not match the layout (48 + 8 x n_records 5"),
    ("sixteen bytes too many", _image(RECV, THREE, pad=bytes(24)), "96 bytes do not match the layout"),
    ("a non-zero pad byte", _image(RECV, THREE, pad=bytes(5) + b"\x01" + bytes(2)), "padding byte 5 behind the records is 0x01, not zero"),
    ("a mark of 8", _image(RECV, [(1, 0), (2, 8)]), "record 1: mark 8 is not a mark"),
    ("a mark of 3", _image(RECV, [(1, 3)]), "record 0: mark 3 is not a mark"),
    ("a mark of 7", _image(RECV, [(1, 0), (1, 1), (1, 7)]), "record 2: mark 7 is not a mark"),
    ("a tx image with mark 1", _image(TX, [(1, 0), (1, 4), (1, 1)]), "record 2: mark 1 has a stage, a sender's timer has none"),
    ("a tx image with mark 6", _image(TX, [(1, 6)]), "record 0: mark 6 has a stage, a sender's timer has none"),
]


@pytest.mark.parametrize("name,blob,text", FLAWS, ids=[f[0] for f in FLAWS])
def test_every_flaw_is_refused_by_name(lib, name, blob, text):
    rc, msg, info = _info(lib, blob)
    assert rc == lib.E_INVALID and msg.startswith("fskhip_xmodem_timer_snapshot_info_get: ") and text in msg, msg
    assert (info.kind, info.n_streams, info.timeout_samples) == (0, 0, 0)   # nothing is reported of a refused image


def test_the_checksum_and_the_front(lib):
    good = _image(RECV, RECV_RECORDS)
    for at in (4 * 6, HEADER, HEADER + 4, len(good) - 9):   # the timeout, a waited, a mark, the last record
        bad = bytearray(good)
        bad[at] ^= 0x04
        rc, msg, _ = _info(lib, bytes(bad))
        assert rc == lib.E_INVALID and "a damaged snapshot" in msg, (at, msg)
    bad = bytearray(good)
    bad[32] ^= 1   # the checksum itself
    rc, msg, _ = _info(lib, bytes(bad))
    assert rc == lib.E_INVALID and "a damaged snapshot" in msg, msg
    rc, msg, _ = _info(lib, good[:40])
    assert rc == lib.E_INVALID and "40 bytes are fewer than an XModem timer snapshot header's 48" in msg, msg
    rc, msg, _ = _info(lib, b"")
    assert rc == lib.E_INVALID and "0 bytes are fewer" in msg, msg


def test_the_validator_as_a_host_program(tmp_path):
    exe = str(tmp_path / "xmodem_timer_image_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "webaudio_modem_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "xmodem_timer_image_check.cpp")],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    last = lines[-1].split()
    # per kind: 3 + 5 records, 96 truncations, 96 x 255 corruptions; and the null image
    assert int(last[0]) == 2 * (3 + 5 + 96 + 96 * 255) + 1 and last[1:] == ["expectations,", "0", "failed"], r.stdout[-2000:]
    assert "3: 40 bytes: 40 bytes are fewer than an XModem timer snapshot header's 48" in lines
    assert "3: 88 bytes: 88 bytes do not match the layout (48 + 8 x n_records 5, rounded up to 16)" in lines


def test_the_calls_refuse_without_a_device(lib):
    L = lib.lib()
    good = _image(RECV, THREE)
    fake = np.zeros(256, np.uint8)   # a non-null timer that must not be looked at
    m = np.zeros(3, np.int64)

    def refused(rc, text):
        assert (rc, L.fskhip_last_error().decode()) == (lib.E_INVALID, text)
    refused(L.fskhip_xmodem_timer_snapshot_info_get(None, 64, C.byref(lib.XModemTimerSnapshotInfo())), "fskhip_xmodem_timer_snapshot_info_get: null snapshot")
    refused(L.fskhip_xmodem_timer_snapshot_info_get(_buf(good), len(good), None), "fskhip_xmodem_timer_snapshot_info_get: null info")
    refused(L.fskhip_xmodem_timer_remap(None, fake.ctypes.data, m.ctypes.data, 3), "fskhip_xmodem_timer_remap: null timer")
    refused(L.fskhip_xmodem_timer_remap(fake.ctypes.data, None, m.ctypes.data, 3), "fskhip_xmodem_timer_remap: null timer")
    refused(L.fskhip_xmodem_timer_remap(fake.ctypes.data, fake.ctypes.data, m.ctypes.data, 3), "fskhip_xmodem_timer_remap: dst and src are the same timer")
    refused(L.fskhip_xmodem_timer_restore(None, _buf(good), len(good), m.ctypes.data, 3), "fskhip_xmodem_timer_restore: null timer")
    w = C.c_size_t(7)
    refused(L.fskhip_xmodem_timer_snapshot(None, None, 0, (C.c_char * 64)(), 64, C.byref(w)), "fskhip_xmodem_timer_snapshot: null timer")
    assert w.value == 7 and not fake.any()
    assert L.fskhip_xmodem_timer_snapshot_bytes(None, None, 0) == 0 and L.fskhip_xmodem_timer_snapshot_bytes(None, m.ctypes.data, 3) == 0
    import webaudio_modem_amd as wm
    with pytest.raises(wm.FskHipError, match="is an XModem handle's snapshot's"):
        wm.XModemTimers.from_snapshot(None, _image(RECV, THREE, magic=XM_MAGIC))
