"""The resident XModem file receiver without a GPU: the golden set (the real XModemTransport.receiveData() under Node,
tools/xmodem_recv_golden/) holds the scenarios the contract rests on; every recorded run replays through step_ref
(tests/xmodem_recv_ref.py) -- each reply planted into a ring, polls until nothing is listed, pending modulations cleared between
polls -- with every modulate() call, its place among the replies, the outcome, the file and the counters as recorded; and the
kernel's own transition (csrc/fsk_xmodem_recv_step.h with the one-reply scan mode) runs as a host program under ASan + UBSan over the
goldens and generated rings and agrees with step_ref."""
import os
import subprocess

import numpy as np
import pytest

import xmodem_recv_ref as ref
from conftest import ROOT
from drain_ref import Rings
from oracle import next_oracle as no

NEEDED = ["one_packet", "two_packets", "five_packets", "empty_file", "eot_with_no_packet", "two_packets_and_eot_in_one_reply",
          "packet_split_across_three_replies", "noise_before_soh_and_between_packets", "duplicate", "duplicate_does_not_reset_retries",
          "invalid_crc_then_good", "invalid_sequence_then_good", "unexpected_sequence_then_good", "errors_up_to_max_retries",
          "errors_beyond_max_retries", "retries_reset_by_an_accepted_packet", "sequence_wraps", "timeout_in_first_byte_wait",
          "timeout_in_header_wait", "timeout_in_payload_wait", "timeouts_beyond_max_retries", "bytes_behind_the_eot", "external_abort"]


def test_the_golden_set_holds_the_scenarios_the_contract_rests_on():
    g = ref.golden_recv()
    names = [c["name"] for c in g.cases]
    assert len(set(names)) == len(names) and set(NEEDED) <= set(names)
    by = {c["name"]: c for c in g.cases}
    assert [len(by[k]["sent"]) - 2 for k in ("one_packet", "two_packets", "five_packets")] == [1, 2, 5]
    assert by["empty_file"]["result"] == b"" and by["eot_with_no_packet"]["result"] == b"" and by["eot_with_no_packet"]["sent"] == [(0, b"\x15"), (1, b"\x06")]
    one = by["two_packets_and_eot_in_one_reply"]   # the reference ACKs each without asking for more
    assert len(one["replies"]) == 1 and one["sent"] == [(0, b"\x15")] + [(1, b"\x06")] * 3
    assert len(by["packet_split_across_three_replies"]["replies"]) == 4
    dup = by["duplicate"]
    assert dup["statistics"]["packetsDropped"] == 1 and dup["statistics"]["packetsReceived"] == 2 and [b for _, b in dup["sent"]] == [b"\x15"] + [b"\x06"] * 4
    assert by["duplicate_does_not_reset_retries"]["outcome"].startswith("Receive failed after max retries")
    assert by["retries_reset_by_an_accepted_packet"]["outcome"] is None
    for k in ("invalid_crc_then_good", "invalid_sequence_then_good", "unexpected_sequence_then_good"):
        assert by[k]["outcome"] is None and [b for _, b in by[k]["sent"]] == [b"\x15", b"\x15", b"\x06", b"\x06"]
    assert by["errors_up_to_max_retries"]["outcome"] is None and by["errors_beyond_max_retries"]["outcome"].startswith("Receive failed after max retries")
    assert by["sequence_wraps"]["expectedSequence"] == 3 and len(by["sequence_wraps"]["result"]) == 257
    for k in ("timeout_in_first_byte_wait", "timeout_in_header_wait", "timeout_in_payload_wait"):
        assert None in by[k]["replies"] and by[k]["outcome"] is None
    assert by["timeouts_beyond_max_retries"]["replies"] == [None] * 3 and by["timeouts_beyond_max_retries"]["outcome"].startswith("Receive failed after max retries")
    assert by["external_abort"]["outcome"] == "Operation aborted" and by["external_abort"]["abort"] == 1
    assert all(c["state"] == "IDLE" for c in g.cases)
    assert g.busy == {name: "Transport busy: receiveData cannot start while in %s state" % name for name in list(ref.STATE_NAMES.values())[1:]}


def check_replay(case, sent, status, words, data):
    name = case["name"]
    assert sent == case["sent"], name
    st = {k: int(v[0]) for k, v in words.items()}
    assert st["packets_received"] == case["statistics"]["packetsReceived"] and st["dropped"] == case["statistics"]["packetsDropped"], name
    assert st["packets_sent"] == len(case["sent"]) and st["expected"] == case["expectedSequence"] and st["state"] == ref.IDLE, name
    if case["result"] is not None:
        assert status == ref.DONE and data == case["result"] and st["file_len"] == len(data), name
    elif case["abort"]:
        assert status == ref.ABORTED and case["outcome"] == "Operation aborted", name
    else:
        assert status == ref.MAX_RETRIES and case["outcome"].startswith("Receive failed after max retries"), name
        assert st["retries"] == case["maxRetries"] + 1 == case["retries"], name


@pytest.mark.parametrize("cap,r0", [(1024, 0), (272, 259), (300, 297)])
def test_step_ref_reproduces_the_recorded_reference(cap, r0):
    """ring placements: from index 0, and two that wrap"""
    for case in ref.golden_recv().cases:
        state = {"words": ref.started_words(ref.fresh_words(1)), "files": [b""]}

        def poll(rings, timeout, abort, case=case, state=state):
            streams, events, after, state["words"], state["files"], sent = ref.step_ref(rings, state["words"], state["files"], 4096, case["maxRetries"],
                                                                                        timeout=[timeout], abort=[abort])
            return {int(s): e for s, e in zip(streams, events)}, after, list(sent.values())
        sent, status = ref.replay(case, poll, cap, r0)
        check_replay(case, sent, status, state["words"], state["files"][0])


# ---- the kernel's transition as a host program -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("xr") / "xmodem_recv_step_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "webaudio_modem_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "xmodem_recv_step_check.cpp")],
                   check=True)

    def run(cases):
        """cases: (words dict of ints, abort, pending, timeout, max_retries, file_capacity, ring bytes) -> per case (event dict,
        touched, listed, removed, span, appended, and the increases of packets_received, dropped, packets_sent)"""
        text = "".join("%d %d %d %d %d %d %d %d %d %s\n" % (w["state"], w["expected"], w["retries"], w["file_len"], ab, pe, to, mr, fc, bytes(buf).hex() or "-")
                       for w, ab, pe, to, mr, fc, buf in cases)
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stderr
        rows = [[int(x) for x in line.split()] for line in r.stdout.splitlines()]
        assert len(rows) == len(cases)
        return [(dict(zip(ref.FIELDS, row[:12])),) + tuple(row[12:]) for row in rows]
    return run


def program_poll(program, rings, words, files, file_capacity, max_retries, timeout=None, abort=None, pending=None):
    """step_ref's return value, computed by the host program: the ring, the words and the files moved as the commit kernel moves them"""
    S = rings.n_streams
    flag = lambda a, s: int(a is not None and bool(a[s]))   # noqa: E731
    live = [s for s in range(S) if words["state"][s] != ref.IDLE]
    got = program([({k: int(words[k][s]) for k in ref.WORDS}, flag(abort, s), flag(pending, s), flag(timeout, s), max_retries, file_capacity,
                    rings.stream_bytes(s)) for s in live])
    after = {k: np.array(v, np.int64) for k, v in words.items()}
    r, n, files_after, streams, events, sent = rings.r.copy(), rings.n.copy(), list(files), [], [], {}
    for s, (ev, touched, listed, removed, span, appended, d_pkt, d_drop, d_sent) in zip(live, got):
        if not touched:
            assert not listed and not removed and not appended and not (d_pkt or d_drop or d_sent)
            continue
        buf = rings.stream_bytes(s)
        if appended:
            assert ev["file_len"] - ev["accepted_len"] == len(files[s])
            files_after[s] = files[s] + buf[span:span + ev["accepted_len"]]
        r[s], n[s] = (r[s] + removed) % rings.cap, n[s] - removed
        for k, v in (("state", ev["state_after"]), ("expected", ev["expected"]), ("retries", ev["retries"]), ("file_len", ev["file_len"])):
            after[k][s] = v
        after["packets_received"][s] += d_pkt
        after["dropped"][s] += d_drop
        after["packets_sent"][s] += d_sent
        assert d_sent == (ev["control"] != -1)
        if d_sent:
            sent[s] = bytes([ev["control"]])
        if listed:
            streams.append(s)
            events.append(tuple(ev[k] for k in ref.FIELDS))
    return (np.array(streams, np.uint32), np.array(events, ref.EVENT_DTYPE), Rings(r, n, rings.ring), {k: v.astype(np.uint32) for k, v in after.items()},
            files_after, sent)


def test_step_program_reproduces_the_recorded_reference(program):
    for case in ref.golden_recv().cases:
        state = {"words": ref.started_words(ref.fresh_words(1)), "files": [b""]}

        def poll(rings, timeout, abort, case=case, state=state):
            streams, events, after, state["words"], state["files"], sent = program_poll(program, rings, state["words"], state["files"], 4096, case["maxRetries"],
                                                                                        timeout=[timeout], abort=[abort])
            return {int(s): e for s, e in zip(streams, events)}, after, list(sent.values())
        sent, status = ref.replay(case, poll, 600, 590)
        check_replay(case, sent, status, state["words"], state["files"][0])


def test_step_program_matches_step_ref_on_generated_rings(program):
    rng = np.random.default_rng(0x4EC7)
    total, seen = 0, set()
    for cap, n_streams, max_payload, max_retries, file_capacity in ((16, 800, 5, 2, 12), (100, 900, 40, 0, 100), (1024, 900, 255, 10, 600), (300, 600, 16, 3, 0)):
        rings, words, files = ref.random_case(rng, n_streams, cap, max_payload, max_retries, file_capacity, idle=0.05)
        abort, pending, timeout = rng.random(n_streams) < 0.1, rng.random(n_streams) < 0.15, rng.random(n_streams) < 0.3
        want = ref.step_ref(rings, words, files, file_capacity, max_retries, timeout=timeout, abort=abort, pending=pending)
        got = program_poll(program, rings, words, files, file_capacity, max_retries, timeout=timeout, abort=abort, pending=pending)
        assert np.array_equal(got[0], want[0]) and got[1].tolist() == want[1].tolist()
        assert np.array_equal(got[2].r, want[2].r) and np.array_equal(got[2].n, want[2].n)
        assert all(np.array_equal(got[3][k], want[3][k]) for k in ref.WORDS) and got[4] == want[4] and got[5] == want[5]
        seen |= {(int(e["status"]), int(e["step"]), int(e["control"])) for e in want[1]}
        total += n_streams
    assert total >= 3000
    assert {st for st, _, _ in seen} == {ref.PROGRESS, ref.DONE, ref.MAX_RETRIES, ref.ABORTED, ref.FILE_FULL}
    assert {k for _, k, _ in seen} >= set(ref.ERRORS) | {no.XM_EOT, no.XM_NEED_MORE} and {c for _, _, c in seen} == {-1, ref.ACK, ref.NAK}


def test_python_surface():
    import ctypes as C
    import __graft_entry__ as ge
    ge.build()
    import webaudio_modem_amd as wm
    from webaudio_modem_amd import _lib
    L = _lib.lib()
    names = ["fskhip_xmodem_recv_" + n for n in ("create", "destroy", "start_host", "poll_host", "poll_device", "state_get", "state_set", "reset", "files_host",
                                                 "files_set_host")]
    assert all(n in _lib.SYMBOL_NAMES and hasattr(L, n) for n in names)
    cls = wm.XModemFileReceiverBatch
    assert all(callable(getattr(cls, m)) for m in ("start", "poll", "poll_active", "files", "set_files", "reset", "state", "set_state", "close"))
    assert wm.xmodem.RECV_EVENT_DTYPE == ref.EVENT_DTYPE and wm.xmodem.RECV_EVENT_DTYPE.itemsize == C.sizeof(_lib.XModemRecvEvent) == 48
    assert wm.xmodem.RECV_WORDS == ref.WORDS and wm.xmodem.RECV_STATE_NAMES == ref.STATE_NAMES
    assert (_lib.XR_IDLE, _lib.XR_SEND_NAK, _lib.XR_WAIT_BLOCK, _lib.XR_SEND_ACK) == (ref.IDLE, ref.SEND_NAK, ref.WAIT_BLOCK, ref.SEND_ACK)
    assert (_lib.XR_PROGRESS, _lib.XR_DONE, _lib.XR_MAX_RETRIES, _lib.XR_ABORTED, _lib.XR_FILE_FULL) == (ref.PROGRESS, ref.DONE, ref.MAX_RETRIES, ref.ABORTED, ref.FILE_FULL)
