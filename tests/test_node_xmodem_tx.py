"""XModemSenderBatch of napi/xmodem.js (-> N-API -> fskhip_xmodem_tx_*): tests/js/xmodem_tx_test.js -- its argument checks without
a device, and on the GPU the closed loop of three streams against XModemReceiverBatch: samples from one processor into the other."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

NODE = shutil.which("node")
JS = os.path.join(ROOT, "tests", "js", "xmodem_tx_test.js")


def _build():
    import __graft_entry__ as ge
    ge.build()
    if not os.path.exists(os.path.join(ROOT, "napi", "fsk_addon.node")):
        pytest.skip("N-API addon not built (no node headers)")


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_xmodem_tx_argument_checks():
    _build()
    out = subprocess.run([NODE, JS, "cpu"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "js xmodem tx cpu tests ok" in out.stdout


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_xmodem_tx_closed_loop_with_the_resident_receiver():
    _build()
    out = subprocess.run([NODE, JS, "gpu"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "js xmodem tx gpu tests ok" in out.stdout
