"""FSKProcessorBatchSharded through Node (napi/fsk-processor.js over the N-API addon): tests/js/processor_sharded_test.js repeats the
quantum parity, image and rebalancing checks of tests/test_gpu_processor_sharded.py at 70 streams; without a GPU it checks the
shard arithmetic and the surface, and processorSnapshotConcat against the Python binding on hand-made images."""
import os
import subprocess

import pytest

from conftest import ROOT
from test_node_host import NODE, _build, _announce
from test_processor_snapshot_cpu import _image, _record

JS = os.path.join(ROOT, "tests", "js", "processor_sharded_test.js")


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_processor_sharded_cpu_side():
    _build()
    out = subprocess.run([NODE, JS, "cpu"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "js processor sharded cpu tests ok" in out.stdout
    _announce("tests/js/processor_sharded_test.js cpu side (no compute calls)")


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_processor_snapshot_concat_is_the_librarys():
    _build()
    import webaudio_modem_amd as wm
    a, b = _image(), _image([_record(48, 0, ring=b"zz", read=47)], pay_cap=0)
    script = ("const p = require(%r); const out = p.processorSnapshotConcat([Buffer.from(%r, 'hex'), Buffer.from(%r, 'hex')]);"
              "console.log(Buffer.from(out.buffer, out.byteOffset, out.byteLength).toString('hex'));"
              "try { p.processorSnapshotConcat([Buffer.from(%r, 'hex'), Buffer.from(%r, 'hex')]); } catch (e) { console.log(/rx_capacity/.test(e.message) ? 'refused' : e.message); }"
              % (os.path.join(ROOT, "napi", "fsk-processor.js"), a.hex(), b.hex(), a.hex(), _image([], rx_cap=64, pay_cap=0).hex()))
    r = subprocess.run([NODE, "-e", script], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split()
    assert bytes.fromhex(lines[0]) == wm.processor_snapshot_concat([a, b]) and lines[1] == "refused"


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_processor_sharded_gpu():
    _build()
    out = subprocess.run([NODE, JS, "gpu"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "js processor sharded gpu tests ok" in out.stdout
    _announce("tests/js/processor_sharded_test.js gpu: FSKProcessorBatchSharded through the addon on the GPU")
