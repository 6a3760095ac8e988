"""fskhip_remap_streams without a GPU: declared, exported, bound on both hosts, and loud on every bad argument it can judge
without an engine (include/fskhip.h)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from webaudio_modem_amd import _lib
    return _lib


def test_remap_is_declared_exported_and_bound(lib):
    hdr = open(os.path.join(ROOT, "include", "fskhip.h")).read()
    assert re.search(r"int fskhip_remap_streams\(fskhip_engine \*dst, const fskhip_engine \*src, const int64_t \*map, uint32_t n_map\);", hdr)
    assert hasattr(C.CDLL(lib.LIB_PATH), "fskhip_remap_streams")
    assert "fskhip_remap_streams" in lib.SYMBOL_NAMES
    import webaudio_modem_amd as wm
    assert callable(wm.FSKEngine.remap_from) and callable(wm.FSKEngine.remapped)
    addon = open(os.path.join(ROOT, "napi", "fsk_addon.cc")).read()
    assert "fskhip_remap_streams(" in addon and '"remapStreams"' in addon
    js = open(os.path.join(ROOT, "napi", "fsk-core.js")).read()
    assert "addon.remapStreams(" in js and re.search(r"\n  remap\(map, configs\)", js)
    assert "remap(map: ArrayLike<number>" in open(os.path.join(ROOT, "napi", "fsk-core.d.ts")).read()


def test_abi_version_is_still_8(lib):
    assert lib.lib().fskhip_abi_version() == 8


def _call(lib, m, n_map=None, dst=None, src=None):
    L = lib.lib()
    if m is None:
        rc = L.fskhip_remap_streams(dst, src, None, n_map)
    else:
        a = np.ascontiguousarray(m, np.int64)
        rc = L.fskhip_remap_streams(dst, src, a.ctypes.data, len(a) if n_map is None else n_map)
    return rc, L.fskhip_last_error().decode()


def test_remap_fails_loudly_without_engines(lib):
    rc, msg = _call(lib, [0, 1, -1])
    assert rc == lib.E_INVALID and "null engine" in msg
    rc, msg = _call(lib, [0, 1, -2, 3])
    assert rc == lib.E_INVALID and "map[2] = -2" in msg          # the first offending index
    rc, msg = _call(lib, None, n_map=4)
    assert rc == lib.E_INVALID and "null map" in msg
    rc, msg = _call(lib, [], n_map=0)
    assert rc == lib.E_INVALID and "null engine" in msg


def test_node_addon_binds_remap():
    node = shutil.which("node")
    addon = os.path.join(ROOT, "napi", "fsk_addon.node")
    import __graft_entry__ as ge
    ge.build()
    if node is None or not os.path.exists(addon):
        pytest.skip("node / the N-API addon not available")
    out = subprocess.run([node, "-e", "const a = require(%r); console.log(typeof a.remapStreams);"
                          "try { a.remapStreams(null, null, [0]); } catch (e) { console.log('threw'); }" % addon],
                         capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["function", "threw"]
