"""XModemTimers of napi/xmodem.js (-> N-API -> fskhip_xmodem_timer_*, fskhip_xmodem_*_poll_timed_host): tests/js/xmodem_timer_test.js -- its
argument checks without a device, and on the GPU the twin of tests/test_gpu_xmodem_timer.py at 70 streams: the class against the plain
polls driven by a model of the contract, word for word after every quantum."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

NODE = shutil.which("node")
JS = os.path.join(ROOT, "tests", "js", "xmodem_timer_test.js")


def _build():
    import __graft_entry__ as ge
    ge.build()
    if not os.path.exists(os.path.join(ROOT, "napi", "fsk_addon.node")):
        pytest.skip("N-API addon not built (no node headers)")


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_xmodem_timer_argument_checks():
    _build()
    out = subprocess.run([NODE, JS, "cpu"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "js xmodem timer cpu tests ok" in out.stdout


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_xmodem_timer_against_a_twin():
    _build()
    out = subprocess.run([NODE, JS, "gpu"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "js xmodem timer gpu tests ok" in out.stdout
