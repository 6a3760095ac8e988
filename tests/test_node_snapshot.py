"""FSKBatch.snapshot / fromSnapshot and FSKBatchSharded.remap (napi/fsk-core.js -> N-API -> fskhip_snapshot_streams /
fskhip_restore_streams) on the GPU: tests/js/snapshot_test.js."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

NODE = shutil.which("node")
JS = os.path.join(ROOT, "tests", "js", "snapshot_test.js")


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_batch_snapshot_round_trip_and_sharded_remap():
    import __graft_entry__ as ge
    ge.build()
    if not os.path.exists(os.path.join(ROOT, "napi", "fsk_addon.node")):
        pytest.skip("N-API addon not built (no node headers)")
    out = subprocess.run([NODE, JS, "gpu"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "js snapshot gpu tests ok" in out.stdout
