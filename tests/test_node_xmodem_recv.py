"""XModemFileReceiverBatch of napi/xmodem.js (-> N-API -> fskhip_xmodem_recv_*): tests/js/xmodem_recv_test.js -- its argument checks without
a device, and on the GPU one planted poll held to values computed in the test, a files() round trip and the busy text."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

NODE = shutil.which("node")
JS = os.path.join(ROOT, "tests", "js", "xmodem_recv_test.js")


def _build():
    import __graft_entry__ as ge
    ge.build()
    if not os.path.exists(os.path.join(ROOT, "napi", "fsk_addon.node")):
        pytest.skip("N-API addon not built (no node headers)")


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_xmodem_recv_argument_checks():
    _build()
    out = subprocess.run([NODE, JS, "cpu"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "js xmodem recv cpu tests ok" in out.stdout


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_xmodem_recv_planted_poll_files_and_busy_text():
    _build()
    out = subprocess.run([NODE, JS, "gpu"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "js xmodem recv gpu tests ok" in out.stdout
