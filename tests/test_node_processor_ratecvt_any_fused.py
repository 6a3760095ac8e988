"""FSKProcessorBatch.lastTxKernel through the N-API addon (include/fskhip_next.h: fskhip_processor_last_tx_kernel):
tests/js/processor_ratecvt_any_fused_test.js -- the surface without a GPU; on the GPU processSamplesAtAny stream-major and as
frames over the host forms, against a twin sent through the two launches."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

NODE = shutil.which("node")
JS = os.path.join(ROOT, "tests", "js", "processor_ratecvt_any_fused_test.js")


def _build():
    import __graft_entry__ as ge
    ge.build()
    if not os.path.exists(os.path.join(ROOT, "napi", "fsk_addon.node")):
        pytest.skip("N-API addon not built (no node headers)")


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_last_tx_kernel_surface():
    _build()
    out = subprocess.run([NODE, JS, "cpu"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "js processor ratecvt any fused cpu tests ok" in out.stdout


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_last_tx_kernel_names_the_path_of_every_form():
    _build()
    out = subprocess.run([NODE, JS, "gpu"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "js processor ratecvt any fused gpu tests ok" in out.stdout
