"""FSKBatch.modulateSamples (napi/fsk-core.js -> N-API -> fskhip_modulate_host_fmt) on the GPU: tests/js/egress_test.js."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

NODE = shutil.which("node")
JS = os.path.join(ROOT, "tests", "js", "egress_test.js")


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_modulate_samples_equals_encoded_float_call():
    import __graft_entry__ as ge
    ge.build()
    if not os.path.exists(os.path.join(ROOT, "napi", "fsk_addon.node")):
        pytest.skip("N-API addon not built (no node headers)")
    out = subprocess.run([NODE, JS, "gpu"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "js egress gpu tests ok" in out.stdout
