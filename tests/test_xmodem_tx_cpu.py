"""The resident XModem sender (include/fskhip_next.h: fskhip_xmodem_tx_*) without a device: the recorded behaviour of the real
XModemTransport.sendData() (tests/golden/golden_xmodem_tx.npz, from tools/xmodem_tx_golden/) replayed through step_ref
(tests/xmodem_tx_ref.py), one demodulate() reply per poll -- every modulate() call, its place among the replies, the outcome and
the counters must come out as recorded --, and the transition the kernel runs (webaudio_modem_amd/csrc/fsk_xmodem_tx_step.h)
compiled as a host program under AddressSanitizer and UBSan, fed the same goldens and generated replies, against step_ref."""
import os
import subprocess

import numpy as np
import pytest

import drain_ref
import xmodem_tx_ref as ref
from conftest import ROOT

OUTCOMES = {ref.DONE: None, ref.MAX_RETRIES: "Timeout - max retries exceeded", ref.ABORTED: "Operation aborted"}


def one_ring(cap, r, data):
    ring = np.full((1, cap), 0xEE, np.uint8)
    ring[0, (r + np.arange(len(data))) % cap] = np.frombuffer(bytes(data), np.uint8)
    return drain_ref.Rings([r], [len(data)], ring)


def replay(case, poll):
    """one golden scenario, a poll per reply through `poll(words, reply, abort) -> (event or None, tx bytes or None, words)`.
    Returns (modulate calls as (replies before, bytes), final status, whether it ended in the first wait, polls made, words)."""
    words = ref.sent_words(ref.fresh_words(1))
    sent, status, first_wait, polls = [], None, False, 0
    for i, reply in enumerate(case["replies"]):
        was = int(words["state"][0])
        ev, tx, words = poll(words, b"" if reply is None else reply, reply is None)
        polls += 1
        if tx is not None:
            sent.append((i + 1, tx))
        if ev is not None and ev["status"] != ref.PROGRESS:
            status, first_wait = ev["status"], was == ref.WAIT_NAK
            break
    return sent, status, first_wait, polls, words


def check_replay(case, sent, status, first_wait, polls, words):
    name = case["name"]
    assert sent == case["sent"], name
    assert status is not None, name                      # every recorded sendData() ended
    want = "Operation aborted at sendData" if status == ref.ABORTED and first_wait else OUTCOMES[status]
    assert want == case["outcome"], name
    assert polls == case["replies_taken"], name          # (replies behind the end of the transfer were never asked for)
    assert int(words["state"][0]) == ref.IDLE and case["after"]["state"] == "IDLE", name
    assert (int(words["packets_sent"][0]), int(words["retransmitted"][0])) == (case["stats"]["packetsSent"], case["stats"]["packetsRetransmitted"]), name
    assert (int(words["sequence"][0]), int(words["fragment_index"][0])) == (case["after"]["sequence"], case["after"]["fragmentIndex"]), name
    assert len(ref.fragments(case["data"], case["maxPayloadSize"])) == case["after"]["fragments"], name


def test_the_golden_set_holds_the_scenarios_the_contract_rests_on():
    g = ref.golden_tx()
    by = {c["name"]: c for c in g.cases}
    assert len(by) == len(g.cases) >= 29
    assert [by[n]["after"]["fragments"] for n in ("one_fragment", "two_fragments", "five_fragments", "empty_file", "exact_multiple")] == [1, 2, 5, 1, 4]
    assert len(by["empty_file"]["data"]) == 0 and by["empty_file"]["sent"][0][1][:4] == bytes([1, 1, 254, 0])
    wrap = by["sequence_wraps"]
    assert wrap["maxPayloadSize"] == 1 and len(wrap["data"]) == 300
    assert [m[1][1] for m in wrap["sent"][253:257]] == [254, 255, 1, 2]                 # 255 -> 1, never 0
    assert by["nak_answered_once"]["stats"]["packetsRetransmitted"] == 2                # an answered NAK counts twice
    assert by["naks_up_to_max_retries"]["outcome"] is None and by["naks_beyond_max_retries"]["outcome"] == "Timeout - max retries exceeded"
    assert by["naks_beyond_max_retries"]["stats"]["packetsRetransmitted"] == 2 * 3 + 1  # the unanswered one counts once
    assert by["retries_are_per_fragment"]["outcome"] is None                            # 6 NAKs with maxRetries 2: the counter restarts per fragment
    assert by["second_control_is_lost"]["replies"][0] == bytes([ref.NAK, ref.ACK]) and by["second_control_is_lost"]["sent"][1][0] == 2
    assert [by[n]["outcome"] for n in ("timeout_in_first_wait", "timeout_in_ack_wait", "timeout_in_final_wait")] == \
        ["Operation aborted at sendData", "Operation aborted", "Operation aborted"]
    assert by["timeout_in_final_wait"]["sent"][-1][1] == bytes([ref.EOT]) and len(by["timeout_in_final_wait"]["sent"]) == 2   # no EOT retransmission
    for need in ("control_behind_noise", "eot_while_waiting_for_ack", "ack_and_eot_before_first_nak", "own_eot_echo_before_final_ack", "empty_reply"):
        assert by[need]["outcome"] is None
    assert g.busy == {k: "Transport busy: sendData cannot start while in %s state" % k for k in ("SENDING_WAIT_NAK", "SENDING_WAIT_ACK", "SENDING_WAIT_FINAL_ACK")}
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "golden_xmodem_tx.npz")) < 1 << 20


@pytest.mark.parametrize("cap,r", [(1024, 0), (16, 13)])
def test_step_ref_reproduces_the_recorded_reference(cap, r):
    for case in ref.golden_tx().cases:
        if max(len(x or b"") for x in case["replies"]) > cap:
            continue

        def poll(words, reply, abort, case=case):
            streams, events, after, words, sent = ref.step_ref(one_ring(cap, r, reply), words, [case["data"]], case["maxPayloadSize"], case["maxRetries"],
                                                               abort=[abort])
            assert after.n[0] == (len(reply) if abort else 0) and after.r[0] == ((r if abort else r + len(reply)) % cap)
            ev = {k: int(events[0][k]) for k in ref.FIELDS} if len(streams) else None
            return ev, sent.get(0), words
        check_replay(case, *replay(case, poll))


def test_step_ref_mask_pending_and_idle_streams_keep_every_word():
    rng = np.random.default_rng(5)
    rings, words, files = ref.random_case(rng, 200, 100, 16, 3)
    mask, pending = rng.random(200) < 0.5, rng.random(200) < 0.3
    streams, events, after, w2, sent = ref.step_ref(rings, words, files, 16, 3, mask=mask, pending=pending)
    still = ~mask | pending | (words["state"] == ref.IDLE)
    assert still.sum() > 50 and (~still).sum() > 30
    assert np.array_equal(after.n[still], rings.n[still]) and np.array_equal(after.r[still], rings.r[still]) and not after.n[~still].any()
    assert all(np.array_equal(w2[k][still], words[k][still]) for k in ref.WORDS)
    assert not set(streams.tolist()) & set(np.flatnonzero(still).tolist()) and set(sent) <= set(streams.tolist())


# ---- the kernel's transition as a host program -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("xt") / "xmodem_tx_step_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "webaudio_modem_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "xmodem_tx_step_check.cpp")],
                   check=True)

    def run(cases):
        """cases: (words dict of ints, abort, pending, max_retries, file_len, max_payload, skew, reply) -> per case (event dict, send,
        touched, drained, listed, packets_sent increase, retransmitted increase)"""
        text = "".join("%d %d %d %d %d %d %d %d %d %d %s\n" % (w["state"], w["sequence"], w["fragment_index"], w["retries"], ab, pe, mr, fl, mp, skew,
                                                            bytes(reply).hex() or "-") for w, ab, pe, mr, fl, mp, skew, reply in cases)
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stderr
        rows = [[int(x) for x in line.split()] for line in r.stdout.splitlines()]
        assert len(rows) == len(cases)
        return [(dict(zip(ref.FIELDS, row[:8])),) + tuple(row[8:]) for row in rows]
    return run


def test_step_program_reproduces_the_recorded_reference(program):
    for skew in (16, 0, 13):
        for case in ref.golden_tx().cases:
            frags = ref.fragments(case["data"], case["maxPayloadSize"])

            def poll(words, reply, abort, case=case, frags=frags):
                w = {k: int(v[0]) for k, v in words.items()}
                ev, send, touched, drained, listed, d_sent, d_retx = program([(w, abort, 0, case["maxRetries"], len(case["data"]), case["maxPayloadSize"], skew, reply)])[0]
                tx = None
                if send == 1:
                    tx = ref.packet(ev["sequence"], frags[ev["fragment_index"]])
                    assert ev["sent_len"] == len(tx)
                elif send == 2:
                    tx = bytes([ref.EOT])
                assert (d_sent == 1) == (tx is not None) and drained == (0 if abort else 1) and touched == 1
                after = {"state": ev["state_after"], "sequence": ev["sequence"], "fragment_index": ev["fragment_index"], "retries": ev["retries"],
                         "packets_sent": w["packets_sent"] + d_sent, "retransmitted": w["retransmitted"] + d_retx}
                return (ev if listed else None), tx, {k: np.array([v], np.uint32) for k, v in after.items()}
            check_replay(case, *replay(case, poll))


def test_step_program_matches_step_ref_on_generated_replies(program):
    rng = np.random.default_rng(0x7E57)
    total, seen = 0, set()
    for cap, n_streams, max_payload, max_retries in ((16, 600, 5, 2), (100, 900, 16, 0), (1024, 900, 128, 10), (1, 100, 255, 1), (300, 700, 1, 3)):
        rings, words, files = ref.random_case(rng, n_streams, cap, max_payload, max_retries, idle=0.0)
        abort, pending = rng.random(n_streams) < 0.1, rng.random(n_streams) < 0.15
        skews = np.where(rng.random(n_streams) < 0.3, 16, rings.r % 16)
        cases = [({k: int(words[k][s]) for k in ref.WORDS}, int(abort[s]), int(pending[s]), max_retries, len(files[s]), max_payload, int(skews[s]),
                  rings.stream_bytes(s)) for s in range(n_streams)]
        got = program(cases)
        streams, events, after, w2, sent = ref.step_ref(rings, words, files, max_payload, max_retries, abort=abort, pending=pending)
        at = {int(s): i for i, s in enumerate(streams)}
        for s, (ev, send, touched, drained, listed, d_sent, d_retx) in enumerate(got):
            assert (s in at) == bool(listed), s
            if s in at:
                assert tuple(ev[k] for k in ref.FIELDS) == events[at[s]].tolist(), s
                seen.add((int(words["state"][s]), ev["status"], ev["control"]))
            assert (ev["state_after"], ev["sequence"], ev["fragment_index"], ev["retries"]) == tuple(int(w2[k][s]) for k in ref.WORDS[:4]), s
            assert (int(words["packets_sent"][s]) + d_sent, int(words["retransmitted"][s]) + d_retx) == (int(w2["packets_sent"][s]), int(w2["retransmitted"][s])), s
            assert bool(drained) == (after.n[s] == 0 and not (abort[s] or pending[s])), s
            assert {0: None, 1: ev["sent_len"], 2: 1}[send] == (len(sent[s]) if s in sent else None), s
            assert bool(touched) == (not pending[s] or bool(abort[s])), s
        total += n_streams
    assert total >= 3000
    # every wait met every control byte it can return, and each of the three ways a transfer ends
    for state in (ref.WAIT_NAK, ref.WAIT_ACK):
        assert {c for st, status, c in seen if st == state and status == ref.PROGRESS} >= {ref.ACK, ref.NAK, ref.EOT}
    assert {status for _, status, _ in seen} == {ref.PROGRESS, ref.DONE, ref.MAX_RETRIES, ref.ABORTED}


def test_python_surface():
    import ctypes as C
    import __graft_entry__ as ge
    ge.build()
    import webaudio_modem_amd as wm
    from webaudio_modem_amd import _lib
    L = _lib.lib()
    names = ["fskhip_xmodem_tx_" + n for n in ("create", "destroy", "send_host", "poll_host", "poll_device", "state_get", "state_set", "reset")]
    assert all(n in _lib.SYMBOL_NAMES and hasattr(L, n) for n in names)
    cls = wm.XModemSenderBatch
    assert all(callable(getattr(cls, m)) for m in ("send", "poll", "poll_active", "reset", "state", "set_state", "close"))
    assert wm.xmodem.TX_EVENT_DTYPE == ref.EVENT_DTYPE and wm.xmodem.TX_EVENT_DTYPE.itemsize == C.sizeof(_lib.XModemTxEvent) == 32
    assert wm.xmodem.TX_WORDS == ref.WORDS and wm.xmodem.TX_STATE_NAMES == ref.STATE_NAMES
    assert (_lib.XT_IDLE, _lib.XT_WAIT_NAK, _lib.XT_WAIT_ACK, _lib.XT_WAIT_FINAL_ACK) == (ref.IDLE, ref.WAIT_NAK, ref.WAIT_ACK, ref.WAIT_FINAL_ACK)
    assert (_lib.XT_PROGRESS, _lib.XT_DONE, _lib.XT_MAX_RETRIES, _lib.XT_ABORTED) == (ref.PROGRESS, ref.DONE, ref.MAX_RETRIES, ref.ABORTED)
