"""Upsampler / Downsampler of napi/filters.js through remap, snapshot and fromSnapshot (-> N-API -> fskhip_resampler_remap, _snapshot,
_restore): tests/js/resample_remap_test.js -- the surface and the device-free refusals without a GPU; on the GPU an interpolator
and a decimator carried by remap and by both snapshot routes against the digest of what the Python binding's remapped() gives for
the same inputs (formulas shared with the script, no random numbers)."""
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NODE = shutil.which("node")
JS = os.path.join(ROOT, "tests", "js", "resample_remap_test.js")
S, L = 66, 6
MAP = [-1 if i % 9 == 4 else (i * 29 + 3) % S for i in range(S + 5)]


def _build():
    import __graft_entry__ as ge
    ge.build()
    if not os.path.exists(os.path.join(ROOT, "napi", "fsk_addon.node")):
        pytest.skip("N-API addon not built (no node headers)")


def _mulaw(m0, n, streams):
    s = np.arange(streams, dtype=np.int64)[:, None]
    m = m0 + np.arange(n, dtype=np.int64)[None, :]
    return ((s * 37 + m * 11 + (m * m) % 7) & 0xFF).astype(np.uint8)


def _floats(t0, n, streams):
    s = np.arange(streams, dtype=np.int64)[:, None]
    t = t0 + np.arange(n, dtype=np.int64)[None, :]
    return (((s * 131 + t * 29) % 2001 - 1000) / 1000).astype(np.float32)


def _python_digests():
    import webaudio_modem_amd as wm
    out = []
    up = wm.Upsampler(L, S)
    up.process(_mulaw(0, 60, S), "mulaw")
    down = wm.Downsampler(L, S)
    down.process(_floats(0, 600, S), "s16")
    for src, step in ((up, lambda h: h.process(_mulaw(60, 37, h.n_streams), "mulaw")), (down, lambda h: h.process(_floats(600, 37 * L, h.n_streams), "s16"))):
        r = src.remapped(MAP)
        d = hashlib.sha256()
        d.update(r.state().tobytes())
        d.update(step(r).tobytes())
        d.update(r.state().tobytes())
        out.append(d.hexdigest())
        r.close()
        src.close()
    return out


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_resample_remap_surface_and_refusals():
    _build()
    out = subprocess.run([NODE, JS, "cpu"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "js resample remap cpu tests ok" in out.stdout


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_remap_and_snapshots_match_the_python_digests():
    _build()
    out = subprocess.run([NODE, JS, "gpu"] + _python_digests(), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "js resample remap gpu tests ok" in out.stdout
