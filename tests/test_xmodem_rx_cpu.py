"""The resident XModem receiver (include/fskhip_next.h: fskhip_xmodem_rx_*) without a device: every refusal the calls make before
they touch one, held to its code and to the whole fskhip_last_error() string, in the header's order; the numpy expectation of a
poll (tests/xmodem_rx_ref.py) on states small enough to read; and the grammar's shared state machine
(webaudio_modem_amd/csrc/fsk_xmodem_scan.h) compiled as a host program under AddressSanitizer and UBSan -- the 50 golden scans of the
real XModemTransport in burst mode, and generated streams in streaming mode against the expectation the GPU tests use."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import drain_ref
import xmodem_rx_ref as ref
from conftest import ROOT, golden_next
from oracle import next_oracle as no

OK, E_INVALID = 0, -1
HOST, DEVICE = "fskhip_xmodem_rx_poll_host", "fskhip_xmodem_rx_poll_device"
NAMES = ["fskhip_xmodem_rx_create", "fskhip_xmodem_rx_destroy", "fskhip_xmodem_rx_reset", "fskhip_xmodem_rx_state_get", "fskhip_xmodem_rx_state_set",
         HOST, DEVICE]


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from webaudio_modem_amd import _lib
    return _lib.lib()


def refused(L, rc, code, text):
    assert (rc, L.fskhip_last_error().decode()) == (code, text)


def test_create_and_state_refusals(L):
    out = C.c_void_p(0x77)
    refused(L, L.fskhip_xmodem_rx_create(None, C.byref(out)), E_INVALID, "fskhip_xmodem_rx_create: null argument")
    refused(L, L.fskhip_xmodem_rx_create(0x1000, None), E_INVALID, "fskhip_xmodem_rx_create: null argument")   # (a refused call follows no pointer)
    assert out.value == 0x77
    words = np.full(4, 300, np.uint32)   # out-of-range sequences: the receiver is missed first, they are not looked at
    refused(L, L.fskhip_xmodem_rx_state_set(None, words.ctypes.data, None, None), E_INVALID, "null receiver")
    refused(L, L.fskhip_xmodem_rx_state_get(None, words.ctypes.data, None, None), E_INVALID, "null receiver")
    refused(L, L.fskhip_xmodem_rx_reset(None, -1), E_INVALID, "null receiver")
    assert L.fskhip_xmodem_rx_destroy(None) == OK
    assert (words == 300).all()


def test_host_form_refusals_in_order(L):
    call = L.fskhip_xmodem_rx_poll_host
    streams, offsets, data = np.zeros(4, np.uint32), np.zeros(5, np.uint32), np.zeros(64, np.uint8)
    results = np.zeros(4, ref.RESULT_DTYPE)
    ST, RE, OF, DA = streams.ctypes.data, results.ctypes.data, offsets.ctypes.data, data.ctypes.data
    ne, nb = C.c_uint32(7), C.c_uint32(7)
    NE, NB = C.addressof(ne), C.addressof(nb)
    for a, b in ((None, NB), (NE, None), (None, None)):
        refused(L, call(None, None, ST, RE, OF, 4, DA, 64, a, b), E_INVALID, HOST + ": null n_events or n_bytes")
    for st, re_, of in ((None, RE, OF), (ST, None, OF), (ST, RE, None), (None, None, None)):
        refused(L, call(None, None, st, re_, of, 4, DA, 64, NE, NB), E_INVALID, HOST + ": null streams, results or offsets with cap_streams 4")
    refused(L, call(None, None, ST, RE, OF, 4, None, 64, NE, NB), E_INVALID, HOST + ": null data with cap_bytes 64")
    refused(L, call(None, None, None, None, None, 0, None, 3, NE, NB), E_INVALID, HOST + ": null data with cap_bytes 3")
    refused(L, call(None, None, ST, RE, OF, 4, DA, 64, NE, NB), E_INVALID, "null receiver")
    refused(L, call(None, None, None, None, None, 0, None, 0, NE, NB), E_INVALID, "null receiver")   # as the size query would be made
    assert (ne.value, nb.value) == (7, 7) and not streams.any() and not offsets.any() and not data.any()   # a refused call writes nothing


def test_device_form_refusals_in_order(L):
    call = L.fskhip_xmodem_rx_poll_device
    ST, RE, OF, DA, TOT = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000   # (device pointers; a refused call never follows one)
    refused(L, call(None, None, ST, RE, OF, 4, DA, 64, None, None), E_INVALID, DEVICE + ": null d_totals")
    for st, re_, of in ((None, RE, OF), (ST, None, OF), (ST, RE, None)):
        refused(L, call(None, None, st, re_, of, 9, DA, 64, TOT, None), E_INVALID, DEVICE + ": null streams, results or offsets with cap_streams 9")
    refused(L, call(None, None, ST, RE, OF, 9, None, 1, TOT, None), E_INVALID, DEVICE + ": null data with cap_bytes 1")
    refused(L, call(None, None, ST, RE, OF, 9, DA, 64, TOT, None), E_INVALID, "null receiver")
    refused(L, call(None, None, None, None, None, 0, None, 0, TOT, 0x6000), E_INVALID, "null receiver")


def test_symbols_are_in_the_python_table(L):
    import webaudio_modem_amd as wm
    from webaudio_modem_amd import _lib
    assert all(n in _lib.SYMBOL_NAMES and hasattr(L, n) for n in NAMES)
    cls = wm.XModemReceiverBatch
    assert all(callable(getattr(cls, m)) for m in ("poll", "poll_active", "reset", "state", "set_state", "close"))
    assert wm.xmodem.RESULT_DTYPE == ref.RESULT_DTYPE and wm.xmodem.RESULT_DTYPE.itemsize == C.sizeof(_lib.XModemResult) == 40


# ---- the expectation itself, on states small enough to read --------------------------------------------------------------------
def ring_of(cap, r, data):
    ring = np.full((1, cap), 0xEE, np.uint8)
    ring[0, (r + np.arange(len(data))) % cap] = np.frombuffer(bytes(data), np.uint8)
    return drain_ref.Rings([r], [len(data)], ring)


def test_poll_ref_a_packet_split_across_two_polls():
    pkt = ref.packet(1, b"hey")                       # 9 bytes
    first, rest = bytes([0x55, 0x66]) + pkt[:5], pkt[5:]
    rings = ring_of(16, 14, first)                    # the span wraps: 14, 15, 0 ..
    streams, results, offsets, data, after, state = ref.poll_ref(rings, [1])
    # only the two noise bytes leave; nothing is listed, nothing is charged; the packet's head waits at the ring's front
    assert len(streams) == 0 and list(offsets) == [0] and len(data) == 0
    assert (after.r[0], after.n[0]) == (0, 5) and after.stream_bytes(0) == pkt[:5]
    assert {k: int(v[0]) for k, v in state.items()} == {"expected": 1, "packets": 0, "dropped": 0}
    # the demodulator appends the rest; the second poll takes the whole packet
    ring = after.ring.copy()
    ring[0, 5:9] = np.frombuffer(rest, np.uint8)
    streams, results, offsets, data, after, state = ref.poll_ref(drain_ref.Rings(after.r, [9], ring), state["expected"], None, state["packets"], state["dropped"])
    assert list(streams) == [0] and list(offsets) == [0, 3] and bytes(data) == b"hey"
    assert results[0].tolist() == (no.XM_NEED_MORE, 2, 1, 0, 9, 3, -1, -1, -1, -1)
    assert (after.r[0], after.n[0]) == (9, 0)
    assert {k: int(v[0]) for k, v in state.items()} == {"expected": 2, "packets": 1, "dropped": 0}


def test_poll_ref_an_error_clears_the_ring():
    good, bad = ref.packet(7, b"ok"), ref.packet(8, b"no", bad_crc=True)
    line = good + bad + b"\x99" + ref.packet(9, b"zz")[:4]          # bytes behind the error, a packet's head among them
    rings = ring_of(40, 3, line)
    streams, results, offsets, data, after, state = ref.poll_ref(rings, [7], packets=[10], dropped=[2])
    crc = no.crc16(b"no")
    assert list(streams) == [0] and bytes(data) == b"ok" and list(offsets) == [0, 2]
    assert results[0].tolist() == (no.XM_INVALID_CRC, 8, 2, 1, 16, 2, 8, 2, crc ^ 0x0100, crc)    # consumed: the end of the offending step
    assert (after.r[0], after.n[0]) == ((3 + len(line)) % 40, 0)                                      # everything left the ring
    assert {k: int(v[0]) for k, v in state.items()} == {"expected": 8, "packets": 12, "dropped": 3}


def test_poll_ref_eot_with_bytes_behind_it_and_the_mask():
    line = b"\x20" + ref.packet(255, b"") + bytes([no.EOT]) + b"\x31\x32"
    rings = drain_ref.Rings([0, 0], [len(line)] * 2, np.tile(np.frombuffer(line + b"\0" * 6, np.uint8), (2, 1)))
    streams, results, offsets, data, after, state = ref.poll_ref(rings, [255, 255], mask=[0, 1])
    assert list(streams) == [1] and list(offsets) == [0, 0]
    assert results[0].tolist() == (no.XM_EOT, 1, 1, 0, 8, 0, -1, -1, -1, -1)      # 255 -> 1; an empty payload is a packet
    assert list(after.r) == [0, 8] and list(after.n) == [len(line), 2] and after.stream_bytes(1) == b"\x31\x32"
    assert list(state["expected"]) == [255, 1] and list(state["packets"]) == [0, 1]


# ---- the shared state machine as a host program ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grammar(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("xm") / "xmodem_rx_grammar_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "webaudio_modem_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "xmodem_rx_grammar_check.cpp")],
                   check=True)

    def run(cases):
        text = "".join("%s %d %s\n" % (mode, e, bytes(b).hex() or "-") for mode, e, b in cases)
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stderr
        rows = [line.split() for line in r.stdout.splitlines()]
        assert len(rows) == len(cases)
        return [([int(x) for x in row[:10]], int(row[10]), b"" if row[11] == "-" else bytes.fromhex(row[11])) for row in rows]
    return run


def test_grammar_program_matches_the_golden_scans(grammar):
    g = golden_next()
    sc = g.manifest["scans"]
    bursts, datas = g.ragged(sc["bytes"]), g.ragged(sc["data"])
    assert len(sc["cases"]) == len(bursts) == 50
    got = grammar([("B", c["expected"], b) for c, b in zip(sc["cases"], bursts)])
    status = {v: k for k, v in no.XM_NAMES.items()}
    for (words, removed, data), c, want in zip(got, sc["cases"], datas):
        assert words == [status[c["status"]], c["expected_after"], c["packets"], c["dropped"], c["consumed"], len(want), c["err_seq"], c["err_len"],
                         c["crc_rx"], c["crc_calc"]], c["name"]
        assert data == want and removed == 0, c["name"]


def test_grammar_program_matches_poll_ref_on_generated_streams(grammar):
    rng = np.random.default_rng(0x58D)
    cases, rings_by_cap = [], []
    for cap, n_streams in ((1, 40), (16, 500), (100, 700), (1024, 900)):
        expected = ref.start_sequences(rng, n_streams)
        rings, strings = ref.traffic_rings(rng, n_streams, cap, expected, idle=0.05)
        rings_by_cap.append((rings, expected, len(cases)))
        cases += [("S", int(e), rings.stream_bytes(s)) for s, e in enumerate(expected)]
    assert len(cases) >= 2000
    got = grammar(cases)
    seen = set()
    for rings, expected, first in rings_by_cap:
        streams, results, offsets, data, after, state = ref.poll_ref(rings, expected)
        at = {int(s): i for i, s in enumerate(streams)}
        for s in range(rings.n_streams):
            words, removed, payload = got[first + s]
            assert removed == rings.n[s] - after.n[s] and words[1] == state["expected"][s] and words[2] == state["packets"][s] and words[3] == state["dropped"][s]
            assert (s in at) == (words[0] != no.XM_NEED_MORE or words[2] + words[3] > 0)
            if s in at:
                i = at[s]
                assert tuple(words) == results[i].tolist() and payload == bytes(data[offsets[i]:offsets[i + 1]])
                seen.add(words[0])
            else:
                assert words[5] == 0 and words[0] == no.XM_NEED_MORE
    assert seen == {no.XM_NEED_MORE, no.XM_EOT, no.XM_INVALID_SEQUENCE, no.XM_INVALID_CRC, no.XM_UNEXPECTED_SEQUENCE}   # never TRUNCATED
