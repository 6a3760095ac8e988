"""The rate converters' calls of any length through napi/filters.js and napi/fsk-processor.js (-> N-API -> fskhip_ratecvt_*_any_host,
fskhip_processor_process_ratecvt_any_host): tests/js/ratecvt_any_test.js -- the surface without a GPU; on the GPU processAny over
cuts against one call, whose digest (samples, history rows, position) is the Python binding's for the same inputs (formulas shared
with the script, no random numbers), position / setPosition, and processSamplesAtAny in 128-frame quanta against the chain on twins."""
import hashlib
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NODE = shutil.which("node")
JS = os.path.join(ROOT, "tests", "js", "ratecvt_any_test.js")
S = 66
N = 128 + 1 + 129 + 128 + 146 + 1 + 148 + 128


def _build():
    import __graft_entry__ as ge
    ge.build()
    if not os.path.exists(os.path.join(ROOT, "napi", "fsk_addon.node")):
        pytest.skip("N-API addon not built (no node headers)")


def _python_digests():
    import webaudio_modem_amd as wm
    s = np.arange(S, dtype=np.int64)[None, :]
    m = np.arange(N, dtype=np.int64)[:, None]
    frames = ((s * 37 + m * 11 + (m * m) % 7) & 0xFF).astype(np.uint8)
    cap = wm.CaptureConverter(44100, 48000, S)
    h = hashlib.sha256()
    h.update(cap.process_any(frames, "mulaw", "sample").tobytes())
    h.update(cap.state().tobytes())
    h.update(struct.pack("<I", cap.position))
    cap.close()
    t = np.arange(N, dtype=np.int64)[None, :]
    x = (((s.T * 131 + t * 29) % 2001 - 1000) / 1000).astype(np.float32)
    play = wm.PlaybackConverter(48000, 44100, S)
    g = hashlib.sha256()
    g.update(play.process_any(x, "s16", "stream").tobytes())
    g.update(play.state().tobytes())
    g.update(struct.pack("<I", play.position))
    play.close()
    return [h.hexdigest(), g.hexdigest()]


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_ratecvt_any_surface():
    _build()
    out = subprocess.run([NODE, JS, "cpu"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "js ratecvt any cpu tests ok" in out.stdout


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_any_length_calls_match_the_python_digests_and_the_chain():
    _build()
    out = subprocess.run([NODE, JS, "gpu"] + _python_digests(), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "js ratecvt any gpu tests ok" in out.stdout
