"""CaptureConverter / PlaybackConverter of napi/filters.js through remap, snapshot and fromSnapshot (-> N-API -> fskhip_ratecvt_remap,
_snapshot, _restore, _snapshot_info_get): tests/js/ratecvt_remap_test.js -- the surface and the device-free refusals without a GPU; on
the GPU both converters at 5 and 65 streams carried by remap and by both snapshot routes against the by-hand carry (state / setState /
setPosition), byte for byte over two further calls, and the refusals."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

NODE = shutil.which("node")
JS = os.path.join(ROOT, "tests", "js", "ratecvt_remap_test.js")


def _build():
    import __graft_entry__ as ge
    ge.build()
    if not os.path.exists(os.path.join(ROOT, "napi", "fsk_addon.node")):
        pytest.skip("N-API addon not built (no node headers)")


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_ratecvt_remap_surface_and_refusals():
    _build()
    out = subprocess.run([NODE, JS, "cpu"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "js ratecvt remap cpu tests ok" in out.stdout


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_remap_and_snapshots_equal_the_by_hand_carry():
    _build()
    out = subprocess.run([NODE, JS, "gpu"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "js ratecvt remap gpu tests ok" in out.stdout
