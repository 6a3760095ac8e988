"""CaptureConverter / PlaybackConverter of napi/filters.js (-> N-API -> fskhip_ratecvt_*): tests/js/ratecvt_test.js -- the surface, the
ratio, the default design and the device-free refusals without a GPU; on the GPU one case per direction against the digest of what
the Python binding returns for the same inputs (formulas shared with the script, no random numbers), then state / setState, reset
and the refusal of a bad nIn."""
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NODE = shutil.which("node")
JS = os.path.join(ROOT, "tests", "js", "ratecvt_test.js")
S = 66


def _build():
    import __graft_entry__ as ge
    ge.build()
    if not os.path.exists(os.path.join(ROOT, "napi", "fsk_addon.node")):
        pytest.skip("N-API addon not built (no node headers)")


def _python_digests():
    import webaudio_modem_amd as wm
    s = np.arange(S, dtype=np.int64)[None, :]

    def frames(m0, n):
        m = m0 + np.arange(n, dtype=np.int64)[:, None]
        return ((s * 37 + m * 11 + (m * m) % 7) & 0xFF).astype(np.uint8)

    cap = wm.CaptureConverter(44100, 48000, S)
    h = hashlib.sha256()
    for m0, n in ((0, 294), (294, 147)):
        h.update(cap.process(frames(m0, n), "mulaw", "sample").tobytes())
    h.update(cap.state().tobytes())
    cap.close()
    t = np.arange(640, dtype=np.int64)[None, :]
    x = (((s.T * 131 + t * 29) % 2001 - 1000) / 1000).astype(np.float32)
    lens = ((np.arange(S) * 53) % 700).astype(np.uint32)
    play = wm.PlaybackConverter(48000, 44100, S)
    g = hashlib.sha256()
    g.update(play.process(x, "s16", "stream", lens=lens).tobytes())
    g.update(play.state().tobytes())
    play.close()
    return [h.hexdigest(), g.hexdigest()]


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_ratecvt_surface_and_refusals():
    _build()
    out = subprocess.run([NODE, JS, "cpu"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "js ratecvt cpu tests ok" in out.stdout


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_converters_match_the_python_digests():
    _build()
    out = subprocess.run([NODE, JS, "gpu"] + _python_digests(), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "js ratecvt gpu tests ok" in out.stdout
