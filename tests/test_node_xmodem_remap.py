"""remap / snapshot / fromSnapshot of the three resident XModem classes of napi/xmodem.js (-> N-API -> fskhip_xmodem_*_remap, _snapshot,
_restore): tests/js/xmodem_remap_test.js -- the surface and the device-free refusals without a GPU; on the GPU, for each class at 70
streams, the image of the remapped object and of a snapshot round trip under the same map against the digest of what the Python
binding produces from the same state (formulas shared with the script, no random numbers)."""
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NODE = shutil.which("node")
JS = os.path.join(ROOT, "tests", "js", "xmodem_remap_test.js")
S = 70
LENGTHS = [0, 1, 15, 16, 17, 127, 128, 129, 600]
MAP = [-1 if i % 9 == 4 else (i * 37 + 11) % S for i in range(64)]


def _build():
    import __graft_entry__ as ge
    ge.build()
    if not os.path.exists(os.path.join(ROOT, "napi", "fsk_addon.node")):
        pytest.skip("N-API addon not built (no node headers)")


def _file(s):
    return bytes((s * 31 + k * 7 + 1) & 0xFF for k in range(LENGTHS[s % 9]))


def _u32(f):
    return np.array([f(s) for s in range(S)], np.uint32)


def _python_digests():
    """the script's three cases through the Python binding: sha256 of the remapped object's image"""
    import webaudio_modem_amd as wm

    def batch(n):
        return wm.FSKProcessorBatch(wm.FSKEngine(n, {}, precision=wm.PRECISION_F32), rx_capacity=300)

    def rx(p):
        h = wm.XModemReceiverBatch(p)
        h.set_state(expected=_u32(lambda s: 1 + s * 13 % 255), packets=_u32(lambda s: s * 3), dropped=_u32(lambda s: s % 7))
        return h

    def tx(p):
        h = wm.XModemSenderBatch(p, 128, 3)
        has = [s % 5 != 0 for s in range(S)]
        h.send([_file(s) for s in range(S)], mask=has)
        frags = lambda s: max(1, -(-LENGTHS[s % 9] // 128))   # noqa: E731
        h.set_state(state=_u32(lambda s: s % 4 if has[s] else 0), sequence=_u32(lambda s: 1 + s * 17 % 255),
                    fragment_index=_u32(lambda s: s % frags(s) if has[s] and s % 4 in (1, 2) else 0), retries=_u32(lambda s: s % 3),
                    packets_sent=_u32(lambda s: s * 5), retransmitted=_u32(lambda s: s % 11))
        return h

    def recv(p):
        h = wm.XModemFileReceiverBatch(p, 600, 3)
        h.set_files([_file(s + 3) for s in range(S)])
        h.set_state(state=_u32(lambda s: s % 4), expected=_u32(lambda s: 1 + s * 19 % 255), retries=_u32(lambda s: s % 4),
                    packets_received=_u32(lambda s: s * 2), dropped=_u32(lambda s: s % 5), packets_sent=_u32(lambda s: s + 1))
        return h

    out = []
    for make in (rx, tx, recv):
        src, dst = batch(S), batch(len(MAP))
        h = make(src)
        nxt = h.remapped(dst, MAP)
        out.append(hashlib.sha256(nxt.snapshot()).hexdigest())
        for x in (nxt, h, dst, dst.engine, src, src.engine):
            x.close()
    return out


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_xmodem_remap_surface_and_refusals():
    _build()
    out = subprocess.run([NODE, JS, "cpu"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "js xmodem remap cpu tests ok" in out.stdout


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_xmodem_remap_and_snapshot_round_trip_match_the_python_digests():
    _build()
    digests = _python_digests()
    out = subprocess.run([NODE, JS, "gpu"] + digests, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "js xmodem remap gpu tests ok" in out.stdout
