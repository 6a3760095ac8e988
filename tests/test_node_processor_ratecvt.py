"""FSKProcessorBatch.processSamplesAt with converters (napi/fsk-processor.js -> N-API -> fskhip_processor_process_ratecvt_host):
tests/js/processor_ratecvt_test.js, its argument checks without a device, and on the GPU its quanta against the chain on a twin and,
for the last of them, against what the Python host gets for the same calls."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NODE = shutil.which("node")
JS = os.path.join(ROOT, "tests", "js", "processor_ratecvt_test.js")


def run(marker, *args):
    import __graft_entry__ as ge
    ge.build()
    if not os.path.exists(os.path.join(ROOT, "napi", "fsk_addon.node")):
        pytest.skip("N-API addon not built (no node headers)")
    out = subprocess.run([NODE, JS, *args], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert marker in out.stdout


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_process_samples_at_takes_converters():
    run("js processor ratecvt cpu tests ok", "cpu")


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_quantum_at_44100_equals_the_python_host(tmp_path):
    import __graft_entry__ as ge
    ge.build()
    import webaudio_modem_amd as wm
    S, Q, quanta = 66, 441, 3
    payloads = [[(s * 29 + 11 * i + 3) & 0xFF for i in range(1 + s % 3)] for s in range(S)]
    engs = [wm.FSKEngine(S, {}) for _ in range(2)]
    tx, rx = (wm.FSKProcessorBatch(e) for e in engs)
    play, cap = wm.PlaybackConverter(48000, 44100, S), wm.CaptureConverter(44100, 48000, S)
    tx.modulate([bytes(p) for p in payloads])
    for _ in range(quanta):
        frames = tx.process_samples_at(None, n_out=Q, downsampler=play)
        assert rx.process_samples_at(frames, upsampler=cap) is None
    assert frames.shape == (Q, S) and frames.dtype == np.uint8 and (frames != 0xFF).any()
    want = dict(streams=S, quantum=Q, quanta=quanta, payloads=payloads, frames=frames.tobytes().hex(), play_state=play.state().tobytes().hex(),
                cap_state=cap.state().tobytes().hex(), rx_processor=rx.snapshot().processor.hex())
    for x in (play, cap, tx, rx, *engs):
        x.close()
    expected = tmp_path / "expected.json"
    expected.write_text(json.dumps(want))
    run("js processor ratecvt gpu tests ok", "gpu", str(expected))
