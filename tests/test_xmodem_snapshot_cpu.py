"""XModem handle remapping and snapshots without a GPU (include/fskhip_next.h): the thirteen functions are declared, exported and
bound on both hosts; fskhip_xmodem_snapshot_info_get reads images of each kind crafted by hand here from the documented layout (a
48-byte header, a word table, the files packed tightly and padded to 16) with the checksum helper of test_processor_snapshot_cpu.py;
every single damage the header lists is refused with a message that names it, by info_get and by the restore of the image's kind;
restore and remap refuse null arguments, a wrong-kind image and a map that does not fit before any device call; and the host-only
validator (csrc/fsk_xmodem_image.h) walks the same images as a stand-alone program under ASan + UBSan.  No handle is involved."""
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

KINDS = ("rx", "tx", "recv")
NAMES = ["fskhip_xmodem_%s_%s" % (k, f) for k in KINDS for f in ("remap", "snapshot_bytes", "snapshot", "restore")] + ["fskhip_xmodem_snapshot_info_get"]
HEADER = 48
RX, TX, RECV = 1, 2, 3
WORDS = {RX: 4, TX: 8, RECV: 8}
LENS = [0, 1, 15, 16, 17]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from webaudio_modem_amd import _lib
    return _lib


def _file(i, n):
    return bytes((7 * i + 3 * k + 1) & 0xFF for k in range(n))


def _image(kind, records, files=(), param0=0, param1=0, pad=None, **over):
    """a well-formed XModem snapshot: `records` are tuples of record words, `files` the bytes behind them in record order"""
    data = b"".join(files)
    f = dict(magic=0x584B5346, format=1, header_bytes=HEADER, kind=kind, n=len(records), record_words=WORDS.get(kind, 8), param0=param0, param1=param1,
             file_bytes=len(data))
    f.update(over)
    f["kind"] = f.pop("header_kind", f["kind"])
    head = struct.pack("<8I2Q", f["magic"], f["format"], f["header_bytes"], f["kind"], f["n"], f["record_words"], f["param0"], f["param1"], 0, f["file_bytes"])
    table = b"".join(struct.pack("<%dI" % len(r), *r) for r in records)
    tail = bytes(-len(data) % 16) if pad is None else pad
    blob = bytearray(head + table + data + tail)
    if len(blob) % 8 == 0:
        blob[32:40] = struct.pack("<Q", _checksum(blob))
    return bytes(blob)


def rx_image(**over):
    return _image(RX, [(1, 0, 0, 0), (255, 7, 2, 0), (17, 1000, 3, 0)], **over)


def tx_records(lens=LENS, p0=16):
    """a sender in every state: an IDLE stream without a file, then files of `lens` bytes -- the first, empty one is the one fragment
    of an empty file, waiting to go out"""
    recs = [(0, 1, 0, 0, 0, 0, 0, 0)]
    for i, n in enumerate(lens):
        frags = max(1, -(-n // p0))
        recs.append(((1, 2, 3, 0)[i % 4], 1 + i, (frags - 1) if i % 4 in (1, 2) else 0, i, 3 * i, i, n, 1))
    return recs


def tx_image(lens=LENS, p0=16, records=None, **over):
    return _image(TX, tx_records(lens, p0) if records is None else records, [_file(i, n) for i, n in enumerate(lens)], param0=p0, param1=10, **over)


def recv_image(lens=LENS, cap=17, records=None, **over):
    recs = [((0, 1, 2, 3, 0)[i % 5], 1 + i, i % 3, n, i, 2 * i, i + 1, 0) for i, n in enumerate(lens)] if records is None else records
    return _image(RECV, recs, [_file(i + 40, n) for i, n in enumerate(lens)], param0=cap, param1=5, **over)


def _info(lib, blob):
    L = lib.lib()
    info = lib.XModemSnapshotInfo()
    rc = L.fskhip_xmodem_snapshot_info_get(_buf(blob) if blob is not None else None, len(blob or b""), C.byref(info))
    return rc, L.fskhip_last_error().decode(), info


def _restore(lib, kind, blob, m=(), dst=None):
    L = lib.lib()
    a = np.ascontiguousarray(m, np.int64)
    rc = getattr(L, "fskhip_xmodem_%s_restore" % kind)(dst, _buf(blob) if blob is not None else None, len(blob or b""), a.ctypes.data if len(a) else None, len(a))
    return rc, L.fskhip_last_error().decode()


def test_the_thirteen_functions_are_declared_exported_and_bound(lib):
    assert len(NAMES) == 13
    hdr = open(os.path.join(ROOT, "include", "fskhip_next.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = C.CDLL(lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b(int|size_t) %s\(" % name, code), name
        assert hasattr(L, name), name
        assert name in lib.SYMBOL_NAMES, name
    assert "typedef struct fskhip_xmodem_snapshot_info {" in code
    assert lib.lib().fskhip_abi_version() == 8
    # the three sentences stay, and say where the state is carried now
    assert hdr.count("kept with this handle and NOT in the processor") == 3
    import webaudio_modem_amd as wm
    for cls in (wm.XModemReceiverBatch, wm.XModemSenderBatch, wm.XModemFileReceiverBatch):
        for meth in ("remapped", "snapshot", "from_snapshot"):
            assert callable(getattr(cls, meth)), (cls, meth)
    assert callable(wm.xmodem_snapshot_info)
    addon = open(os.path.join(ROOT, "napi", "fsk_addon_next.cc")).read()
    js = open(os.path.join(ROOT, "napi", "xmodem.js")).read()
    dts = open(os.path.join(ROOT, "napi", "xmodem.d.ts")).read()
    for kind, cap in (("rx", "Rx"), ("tx", "Tx"), ("recv", "Recv")):
        assert "XM_LIFECYCLE(%s," % cap in addon
        for f in ("Remap", "Snapshot", "Restore"):
            assert '"xmodem%s%s"' % (cap, f) in addon and "addon.xmodem%s%s" % (cap, f) in js, (cap, f)
    for call in ("fskhip_xmodem_##kind##_remap(", "fskhip_xmodem_##kind##_snapshot(", "fskhip_xmodem_##kind##_restore(", "fskhip_xmodem_snapshot_info_get(",
                 '"xmodemSnapshotInfo"'):
        assert call in addon, call
    assert "addon.xmodemSnapshotInfo(" in js and "xmodemSnapshotInfo," in js
    assert dts.count("remap(processor: object, map: ArrayLike<number>)") == 3 and dts.count("snapshot(streams?: ArrayLike<number> | null): Buffer;") == 3
    assert dts.count("static fromSnapshot(processor: object, buf: Uint8Array") == 3 and "export declare function xmodemSnapshotInfo(" in dts


def test_hand_made_images_of_each_kind_are_read_on_the_host(lib):
    for blob, want in ((rx_image(), (RX, 3, 0, 0, 0)), (tx_image(), (TX, 6, 16, 10, sum(LENS))), (recv_image(), (RECV, 5, 17, 5, sum(LENS))),
                       (_image(RX, []), (RX, 0, 0, 0, 0)), (tx_image(lens=[]), (TX, 1, 16, 10, 0)), (_image(TX, [], param0=128, param1=3), (TX, 0, 128, 3, 0)),
                       (_image(RECV, [], param0=0, param1=0), (RECV, 0, 0, 0, 0)),
                       # has_file 1 and file_len 0 in WAIT_NAK: the empty file that is one fragment
                       (_image(TX, [(1, 1, 0, 0, 0, 0, 0, 1)], param0=128), (TX, 1, 128, 0, 0)),
                       (tx_image(lens=[600, 0, 129], p0=7), (TX, 4, 7, 10, 729)), (recv_image(lens=[600, 600, 0], cap=600), (RECV, 3, 600, 5, 1200))):
        rc, msg, info = _info(lib, blob)
        assert rc == 0, msg
        assert (info.kind, info.n_streams, info.param0, info.param1, info.file_bytes) == want
        assert len(blob) == HEADER + 4 * want[1] * WORDS[want[0]] + (want[4] + 15) // 16 * 16
    # an unaligned copy reads the same
    blob = tx_image()
    raw = bytearray(1 + len(blob))
    raw[1:] = blob
    arr = (C.c_char * len(raw)).from_buffer(raw)
    info = lib.XModemSnapshotInfo()
    assert lib.lib().fskhip_xmodem_snapshot_info_get(C.addressof(arr) + 1, len(blob), C.byref(info)) == 0 and info.n_streams == 6
    import webaudio_modem_amd as wm
    assert wm.xmodem_snapshot_info(recv_image()) == dict(kind=RECV, n_streams=5, param0=17, param1=5, file_bytes=49)
    with pytest.raises(wm.FskHipError, match="checksum"):
        wm.xmodem_snapshot_info(_flip(recv_image(), HEADER + 3))


def _tx1(*rec, p0=16, data=b""):
    return _image(TX, [rec], [data], param0=p0)


def _recv1(*rec, cap=16, data=b""):
    return _image(RECV, [rec], [data], param0=cap)


TABLE_TX = HEADER + 6 * 32
BAD = [
    ("null", None, None, "null snapshot"),
    ("short", "tx", lambda: tx_image()[:HEADER - 8], "fewer than an XModem snapshot header"),
    ("magic", "tx", lambda: tx_image(magic=0x504B5346), "magic"),
    ("format", "rx", lambda: rx_image(format=2), "format 2"),
    ("header-bytes", "rx", lambda: rx_image(header_bytes=64), "header_bytes 64"),
    ("kind-0", "rx", lambda: rx_image(header_kind=0), "kind 0"),
    ("kind-4", "rx", lambda: rx_image(header_kind=4), "kind 4"),
    ("record-words", "rx", lambda: _image(RX, [(1, 0, 0, 0, 0, 0, 0, 0)], record_words=8), "record_words 8"),
    ("record-words-tx", "tx", lambda: _image(TX, [(0, 1, 0, 0)], record_words=4, param0=16), "record_words 4"),
    ("record-count", "rx", lambda: rx_image(n=4), "do not match the layout"),
    ("truncated", "tx", lambda: tx_image()[:-16], "do not match the layout"),
    ("overlong", "recv", lambda: recv_image() + b"\0" * 16, "do not match the layout"),
    ("file-bytes-huge", "recv", lambda: recv_image(file_bytes=1 << 62), "do not match the layout"),
    ("flipped-word", "tx", lambda: _flip(tx_image(), HEADER + 5), "checksum"),
    ("flipped-file-byte", "tx", lambda: _flip(tx_image(), TABLE_TX + 20), "checksum"),
    ("flipped-header-byte", "recv", lambda: _flip(recv_image(), 29), "checksum"),
    ("file-len-sum", "recv", lambda: recv_image(file_bytes=sum(LENS) + 1), "file_len sum to 49, file_bytes is 50"),
    ("file-len-sum-tx", "tx", lambda: _image(TX, [(0, 1, 0, 0, 0, 0, 5, 1)], [b"abcdefgh"], param0=16), "file_len sum to 5, file_bytes is 8"),
    ("padding", "recv", lambda: recv_image(pad=b"\0" * 14 + b"\1"), "padding byte 14"),
    ("rx-params", "rx", lambda: rx_image(param1=3), "reserved header words"),
    ("rx-reserved-word", "rx", lambda: _image(RX, [(1, 0, 0, 0), (1, 0, 0, 9)]), "record 1: reserved word 3"),
    ("recv-reserved-word", "recv", lambda: _recv1(0, 1, 0, 0, 0, 0, 0, 1), "record 0: reserved word 7"),
    ("rx-expected-0", "rx", lambda: _image(RX, [(0, 0, 0, 0)]), "record 0: expected 0"),
    ("rx-expected-256", "rx", lambda: _image(RX, [(1, 0, 0, 0), (256, 0, 0, 0)]), "record 1: expected 256"),
    ("tx-param0-0", "tx", lambda: _image(TX, [], param0=0), "param0 (max_payload_size) 0"),
    ("tx-param0-256", "tx", lambda: _image(TX, [], param0=256), "param0 (max_payload_size) 256"),
    ("tx-state", "tx", lambda: _tx1(4, 1, 0, 0, 0, 0, 0, 0), "record 0: state 4"),
    ("tx-sequence-0", "tx", lambda: _tx1(0, 0, 0, 0, 0, 0, 0, 0), "record 0: sequence 0"),
    ("tx-sequence-256", "tx", lambda: _tx1(0, 256, 0, 0, 0, 0, 0, 0), "record 0: sequence 256"),
    ("tx-has-file-2", "tx", lambda: _tx1(0, 1, 0, 0, 0, 0, 0, 2), "record 0: has_file 2"),
    ("tx-len-without-file", "tx", lambda: _tx1(0, 1, 0, 0, 0, 0, 3, 0, data=b"abc"), "record 0: file_len 3 without a file"),
    ("tx-waiting-without-file", "tx", lambda: _tx1(1, 1, 0, 0, 0, 0, 0, 0), "no file is held"),
    ("tx-fragment-index", "tx", lambda: _tx1(2, 1, 2, 0, 0, 0, 17, 1, data=bytes(17)), "record 0: fragment_index 2 of 2 fragments"),
    ("tx-fragment-index-empty", "tx", lambda: _tx1(1, 1, 1, 0, 0, 0, 0, 1), "record 0: fragment_index 1 of 1 fragments"),
    ("recv-state", "recv", lambda: _recv1(4, 1, 0, 0, 0, 0, 0, 0), "record 0: state 4"),
    ("recv-expected-0", "recv", lambda: _recv1(0, 0, 0, 0, 0, 0, 0, 0), "record 0: expected 0"),
    ("recv-expected-256", "recv", lambda: _recv1(2, 256, 0, 0, 0, 0, 0, 0), "record 0: expected 256"),
    ("recv-file-len", "recv", lambda: _recv1(2, 1, 0, 17, 0, 0, 0, 0, data=bytes(17)), "record 0: file_len 17 exceeds file_capacity 16"),
]


def test_fragment_index_is_free_outside_the_two_waits(lib):
    """IDLE and WAIT_FINAL_ACK carry whatever index the transfer ended with"""
    for state in (0, 3):
        rc, msg, _ = _info(lib, _tx1(state, 1, 9, 0, 0, 0, 0, 0))
        assert rc == 0, msg


@pytest.mark.parametrize("name,kind,make,pattern", BAD, ids=[b[0] for b in BAD])
def test_damaged_images_are_refused_with_a_telling_message(lib, name, kind, make, pattern):
    blob = make() if make else None
    calls = [("fskhip_xmodem_snapshot_info_get", lambda: _info(lib, blob)[:2])]
    for k in KINDS if kind is None else (kind,):
        calls.append(("fskhip_xmodem_%s_restore" % k, lambda k=k: _restore(lib, k, blob, [0])))
    for fn, call in calls:
        rc, msg = call()
        assert rc == lib.E_INVALID, (fn, rc, msg)
        assert pattern in msg and fn in msg, (fn, msg)


def test_restore_and_remap_refuse_before_any_device_call(lib):
    L = lib.lib()
    images = {"rx": rx_image(), "tx": tx_image(), "recv": recv_image()}
    for kind in KINDS:
        remap, snap, size = (getattr(L, "fskhip_xmodem_%s_%s" % (kind, f)) for f in ("remap", "snapshot", "snapshot_bytes"))
        assert remap(None, None, None, 0) == lib.E_INVALID and "null handle" in L.fskhip_last_error().decode()
        w = C.c_size_t(0)
        assert snap(None, None, 0, (C.c_char * 64)(), 64, C.byref(w)) == lib.E_INVALID and "null handle" in L.fskhip_last_error().decode()
        assert size(None, None, 4) == 0
        good = images[kind]
        rc, msg = _restore(lib, kind, good, [0, 1, 2])
        assert rc == lib.E_INVALID and "null handle" in msg
        # the map against itself and against the image: a null map that should hold entries, an entry below -1, an entry past the records
        assert getattr(L, "fskhip_xmodem_%s_restore" % kind)(None, _buf(good), len(good), None, 4) == lib.E_INVALID
        assert "null map" in L.fskhip_last_error().decode()
        rc, msg = _restore(lib, kind, good, [0, 1, -2, -3])
        assert rc == lib.E_INVALID and "map[2] = -2" in msg
        n = lib.XModemSnapshotInfo()
        assert L.fskhip_xmodem_snapshot_info_get(_buf(good), len(good), C.byref(n)) == 0
        rc, msg = _restore(lib, kind, good, [0, n.n_streams, 1])
        assert rc == lib.E_INVALID and "map[1] = %d, the snapshot has %d records" % (n.n_streams, n.n_streams) in msg
        # an image of another kind
        for other in KINDS:
            if other != kind:
                rc, msg = _restore(lib, kind, images[other], [0])
                assert rc == lib.E_INVALID and "the snapshot is of kind" in msg and "(%s)" % other in msg and "(%s)" % kind in msg, msg
    assert L.fskhip_xmodem_snapshot_info_get(_buf(images["rx"]), len(images["rx"]), None) == lib.E_INVALID
    assert "null info" in L.fskhip_last_error().decode()
    import webaudio_modem_amd as wm
    with pytest.raises(ValueError, match="kind 'rx'"):
        wm.XModemSenderBatch.from_snapshot(None, images["rx"])


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("xs") / "xmodem_snapshot_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "webaudio_modem_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "xmodem_snapshot_check.cpp")],
                   check=True)
    return exe


def test_the_validator_walks_the_same_images_as_a_host_program(lib, program):
    good = [rx_image(), tx_image(), recv_image(), _image(RX, []), tx_image(lens=[600, 0, 129], p0=7), recv_image(lens=[600, 600, 0], cap=600),
            _image(TX, [(1, 1, 0, 0, 0, 0, 0, 1)], param0=128)]
    bad = [(make(), pattern) for _, _, make, pattern in BAD if make]
    blobs = good + [b for b, _ in bad]
    text = "".join((b.hex() or "-") + "\n" for b in blobs)
    r = subprocess.run([program], input=text, capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == len(blobs) + 1 and lines[-1] == "-1 null snapshot"
    for blob, line in zip(blobs, lines):
        rc, msg, info = _info(lib, blob)
        if rc == 0:
            n_table = 4 * info.n_streams * WORDS[info.kind]
            files = blob[HEADER + n_table:HEADER + n_table + info.file_bytes]
            assert line == "0 %d %d %d %d %d %d" % (info.kind, info.n_streams, info.param0, info.param1, info.file_bytes, sum(files)), line
        else:
            assert line.startswith("-1 ") and msg == "fskhip_xmodem_snapshot_info_get: " + line[3:], (line, msg)
    assert [ln[0] for ln in lines[:len(good)]] == ["0"] * len(good)
    for (_, pattern), line in zip(bad, lines[len(good):]):
        assert line.startswith("-1 ") and pattern in line, (pattern, line)


def test_node_addon_binds_xmodem_snapshots():
    node = shutil.which("node")
    addon = os.path.join(ROOT, "napi", "fsk_addon.node")
    import __graft_entry__ as ge
    ge.build()
    if node is None or not os.path.exists(addon):
        pytest.skip("node / the N-API addon not available")
    blob = tx_image()
    names = ["xmodem%s%s" % (k, f) for k in ("Rx", "Tx", "Recv") for f in ("Remap", "Snapshot", "Restore")] + ["xmodemSnapshotInfo"]
    script = ("const a = require(%r); const b = Buffer.from(%r, 'hex');"
              "console.log(%s.map((n) => typeof a[n]).join(' '));"
              "const i = a.xmodemSnapshotInfo(b); console.log(i.kind, i.nStreams, i.param0, i.param1, i.fileBytes);"
              "try { a.xmodemTxRestore(null, b, [0]); } catch (e) { console.log(/null handle/.test(e.message) ? 'null-handle' : e.message); }"
              "try { a.xmodemRxRestore(null, b, [0]); } catch (e) { console.log(/of kind 2/.test(e.message) ? 'kind' : e.message); }"
              "b[%d] ^= 1; try { a.xmodemSnapshotInfo(b); } catch (e) { console.log(/checksum/.test(e.message) ? 'checksum' : e.message); }"
              % (addon, blob.hex(), names, HEADER + 3))
    out = subprocess.run([node, "-e", script], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["function"] * 10 + ["2", "6", "16", "10", "49", "null-handle", "kind", "checksum"]
