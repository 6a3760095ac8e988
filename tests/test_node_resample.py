"""Upsampler / Downsampler of napi/filters.js (-> N-API -> fskhip_resampler_*): tests/js/resample_test.js -- the surface and the
device-free refusals without a GPU; on the GPU one case per direction against the digest of what the Python binding returns for the
same inputs (formulas shared with the script, no random numbers)."""
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NODE = shutil.which("node")
JS = os.path.join(ROOT, "tests", "js", "resample_test.js")
S, L = 66, 6


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

    up = wm.Upsampler(L, S)
    h = hashlib.sha256()
    for m0, n in ((0, 60), (60, 40)):
        h.update(up.process(frames(m0, n), "mulaw", "sample").tobytes())
    h.update(up.state().tobytes())
    up.close()
    t = np.arange(600, dtype=np.int64)[None, :]
    x = (((s.T * 131 + t * 29) % 2001 - 1000) / 1000).astype(np.float32)
    lens = ((np.arange(S) * 53) % 700).astype(np.uint32)
    down = wm.Downsampler(L, S)
    g = hashlib.sha256()
    g.update(down.process(x, "s16", "stream", lens=lens).tobytes())
    g.update(down.state().tobytes())
    down.close()
    return [h.hexdigest(), g.hexdigest()]


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_resample_surface_and_refusals():
    _build()
    out = subprocess.run([NODE, JS, "cpu"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "js resample cpu tests ok" in out.stdout


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_resamplers_match_the_python_digests():
    _build()
    out = subprocess.run([NODE, JS, "gpu"] + _python_digests(), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "js resample gpu tests ok" in out.stdout
