"""FSKProcessorBatch.processSamplesAt (napi/fsk-processor.js -> N-API -> fskhip_processor_process_rate_host): tests/js/processor_rate_test.js,
its argument checks without a device and its TX / RX equality with the chain Upsampler -> process() -> Downsampler on a twin on the GPU."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

NODE = shutil.which("node")
JS = os.path.join(ROOT, "tests", "js", "processor_rate_test.js")


def run(mode, marker):
    import __graft_entry__ as ge
    ge.build()
    if not os.path.exists(os.path.join(ROOT, "napi", "fsk_addon.node")):
        pytest.skip("N-API addon not built (no node headers)")
    out = subprocess.run([NODE, JS, mode], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert marker in out.stdout


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_process_samples_at_argument_checks():
    run("cpu", "js processor rate cpu tests ok")


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_process_samples_at_equals_the_chain_on_a_twin():
    run("gpu", "js processor rate gpu tests ok")
