"""XModemTimers.remap / snapshot / fromSnapshot and xmodemTimerSnapshotInfo of napi/xmodem.js (-> N-API -> fskhip_xmodem_timer_remap,
_snapshot, _restore, _snapshot_info_get): tests/js/xmodem_timer_remap_test.js -- the surface and the image validator without a device,
and on the GPU the words through every map at 70 streams, both ways, for both kinds, with the kind-mismatch TypeError."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

NODE = shutil.which("node")
JS = os.path.join(ROOT, "tests", "js", "xmodem_timer_remap_test.js")


def _build():
    import __graft_entry__ as ge
    ge.build()
    if not os.path.exists(os.path.join(ROOT, "napi", "fsk_addon.node")):
        pytest.skip("N-API addon not built (no node headers)")


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_xmodem_timer_remap_surface_and_images():
    _build()
    out = subprocess.run([NODE, JS, "cpu"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "js xmodem timer remap cpu tests ok" in out.stdout


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_xmodem_timer_words_through_every_map():
    _build()
    out = subprocess.run([NODE, JS, "gpu"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "js xmodem timer remap gpu tests ok" in out.stdout
