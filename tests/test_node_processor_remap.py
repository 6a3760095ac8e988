"""FSKProcessorBatch.remap / snapshot / fromSnapshot (napi/fsk-processor.js -> N-API -> fskhip_processor_remap / _snapshot /
_restore) on the GPU: tests/js/processor_remap_test.js."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

NODE = shutil.which("node")
JS = os.path.join(ROOT, "tests", "js", "processor_remap_test.js")


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_processor_batch_remap_and_snapshot_continue_streams():
    import __graft_entry__ as ge
    ge.build()
    if not os.path.exists(os.path.join(ROOT, "napi", "fsk_addon.node")):
        pytest.skip("N-API addon not built (no node headers)")
    out = subprocess.run([NODE, JS, "gpu"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "js processor remap gpu tests ok" in out.stdout
