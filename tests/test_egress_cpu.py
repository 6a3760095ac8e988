"""The encode direction of the capture formats without a GPU (include/fskhip.h: fskhip_egress_device, fskhip_modulate_host_fmt): the
numpy reference the GPU tests use (tests/samples_ref.py) against Python's audioop for every 16-bit value, the fixed point through the
decoders for every code, the s16 rule at its edges, the staging geometry of the host call (csrc/fsk_plan.h: egress_stage, compiled
here with g++), the Python argument checks and -- with no device -- the loud failure of the compute entry points."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import samples_ref as er
import samples_ref as ir

from conftest import ROOT

S16 = np.arange(-32768, 32768, dtype=np.int32)


def test_encode_reference_is_audioop_for_every_value():
    audioop = pytest.importorskip("audioop")
    raw = S16.astype("<i2").tobytes()
    for fmt, fn, ref in (("mulaw", audioop.lin2ulaw, er.linear_to_mulaw), ("alaw", audioop.lin2alaw, er.linear_to_alaw)):
        want = np.frombuffer(fn(raw, 2), dtype=np.uint8)
        got = ref(S16)
        assert got.dtype == np.uint8 and np.array_equal(got, want), fmt
        # ... and through the floats: every value k / 32768 is its own 16-bit value
        assert np.array_equal(er.encode(S16.astype(np.float32) / np.float32(32768), fmt), want), fmt
    assert np.array_equal(er.encode(S16.astype(np.float32) / np.float32(32768), "s16"), S16.astype(np.int16))


def test_it_is_the_standard_encoder_not_the_nearest_table_entry():
    x = S16.astype(np.float32) / np.float32(32768)
    for fmt, differ in (("mulaw", 1016), ("alaw", 747)):       # (by decoded value: the two codes of mu-law's zero are one value)
        assert int((ir.decode(er.encode(x, fmt), fmt) != ir.decode(ir.quantise(x, fmt), fmt)).sum()) == differ, fmt
    assert np.array_equal(er.encode(x, "s16"), ir.quantise(x, "s16"))


def test_every_code_is_a_fixed_point_through_the_decoders():
    codes = np.arange(256, dtype=np.uint8)
    for fmt in ("mulaw", "alaw"):
        dec = ir.decode(codes, fmt)
        again = er.encode(dec, fmt)
        assert np.array_equal(ir.decode(again, fmt), dec), fmt
        moved = np.flatnonzero(again != codes).tolist()
        assert moved == ([127] if fmt == "mulaw" else []), (fmt, moved)
    assert er.encode(ir.decode(np.uint8(127), "mulaw"), "mulaw") == 0xFF    # negative zero re-encodes as zero


def test_silence_is_what_zero_encodes_to():
    for fmt in ("f32", "s16", "mulaw", "alaw"):
        z = er.encode(np.zeros(1, np.float32), fmt)
        assert z.dtype == er.DTYPES[fmt] and z[0] == er.silence(fmt) and np.dtype(type(er.silence(fmt))) == z.dtype
    assert (er.silence("s16"), er.silence("mulaw"), er.silence("alaw"), er.silence("f32")) == (0, 0xFF, 0xD5, 0.0)


def test_s16_rule_at_its_edges():
    k = np.arange(-40000, 40000, dtype=np.int64)
    ties = ((k + 0.5) / 32768.0).astype(np.float32)                  # exact in float32: k + 0.5 has at most 17 bits
    assert np.array_equal(ties.astype(np.float64) * 32768.0, k + 0.5)
    want = np.clip(np.where(k % 2 == 0, k, k + 1), -32768, 32767)    # ties to even: k + 0.5 -> the even one of k, k + 1
    assert np.array_equal(er.to_s16(ties), want)
    edge = np.array([1.0, -1.0, np.inf, -np.inf, np.nan, -0.0, 1.0 + 2.0 ** -23, -(1.0 + 2.0 ** -23), 1e-45, 3.4e38, -3.4e38,
                     32767.0 / 32768, 32766.5 / 32768, 32767.5 / 32768, -32768.5 / 32768], np.float32)
    assert er.to_s16(edge).tolist() == [32767, -32768, 32767, -32768, 0, 0, 32767, -32768, 0, 32767, -32768, 32767, 32766, 32767, -32768]
    assert er.encode(edge, "s16").dtype == np.int16
    # f32 is the same bits, NaN payloads and the sign of zero included
    bits = np.array([0x7FC5E417, 0x80000000, 0xFF800001, 0x00000001], np.uint32)
    assert np.array_equal(er.encode(bits.view(np.float32), "f32").view(np.uint32), bits)


@pytest.fixture(scope="module")
def stage(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not installed")
    d = tmp_path_factory.mktemp("egress_stage")
    (d / "t.cc").write_text(r'''
#include <cstdio>
#include <cstdlib>
#include "fsk_plan.h"
int main(int argc, char **argv) {
  for (int i = 1; i + 3 < argc; i += 4) {
    const fsk::EgressStage g = fsk::egress_stage(strtoull(argv[i], 0, 10), strtoull(argv[i + 1], 0, 10), strtoull(argv[i + 2], 0, 10), atoi(argv[i + 3]) != 0);
    printf("%zu %zu %zu %zu %zu\n", g.fpitch, g.npitch, g.bytes, g.rows, g.row_bytes);
  }
  return 0;
}
''')
    exe = str(d / "t")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "webaudio_modem_amd", "csrc"), "-o", exe, str(d / "t.cc")], check=True)

    def run(*cases):
        args = [str(v) for c in cases for v in c]
        out = subprocess.run([exe] + args, check=True, capture_output=True, text=True).stdout.splitlines()
        return [tuple(int(v) for v in line.split()) for line in out]
    return run


def test_host_call_staging_geometry(stage):
    """fskhip_modulate_host_fmt's buffers and its one 2-D copy: float rows at a multiple of four floats, narrow stream-major rows on
    16-byte boundaries, packed frames; the copy never reads past the staging and takes exactly the elements (s < S, t < n)."""
    cases = [(S, n, esz, fr) for S in (1, 63, 65, 130) for n in (0, 1, 5, 15, 16, 17, 8199, 48000) for esz in (4, 2, 1) for fr in (0, 1)]
    for (S, n, esz, fr), (fpitch, npitch, nbytes, rows, row_bytes) in zip(cases, stage(*cases)):
        assert fpitch % 4 == 0 and n <= fpitch < n + 4
        if fr:
            assert (npitch, rows, row_bytes) == (S, n, S * esz)
        else:
            assert (npitch * esz) % 16 == 0 and n <= npitch < n + 16 // esz and (rows, row_bytes) == (S, n * esz)
        assert nbytes == rows * npitch * esz and row_bytes <= npitch * esz
        assert rows * row_bytes == S * n * esz
    # sizes of a full-scale call stay exact in 64 bits
    assert stage((1 << 20, 1 << 24, 4, 0)) == [(1 << 24, 1 << 24, 1 << 46, 1 << 20, 1 << 26)]


def test_python_argument_checks():
    from webaudio_modem_amd.engine import samples_out, payload_args
    out, code, lay, pitch = samples_out("s16", "stream", 3, 7)
    assert (out.shape, out.dtype, code, lay, pitch) == ((3, 7), np.int16, 1, 0, 7)
    out, code, lay, pitch = samples_out("alaw", "sample", 3, 7)
    assert (out.shape, out.dtype, code, lay, pitch) == ((7, 3), np.uint8, 3, 1, 3)
    wide = np.zeros((7, 10), np.uint8)
    view, _, _, pitch = samples_out("mulaw", "sample", 3, 7, wide[:, 4:7])     # a shard's column block: the full frame pitch
    assert view.ctypes.data == wide.ctypes.data + 4 and pitch == 10
    rows = np.zeros((9, 7), np.float32)
    view, _, _, pitch = samples_out("f32", "stream", 3, 7, rows[2:5])          # ... and its row block
    assert view.ctypes.data == rows[2:].ctypes.data and pitch == 7
    with pytest.raises(ValueError, match="format"):
        samples_out("pcm24", "stream", 3, 7)
    with pytest.raises(ValueError, match="layout"):
        samples_out("s16", "planar", 3, 7)
    with pytest.raises(ValueError, match="int16 array of shape"):
        samples_out("s16", "stream", 3, 7, np.zeros((3, 7), np.uint8))
    with pytest.raises(ValueError, match="shape"):
        samples_out("s16", "sample", 3, 7, np.zeros((3, 7), np.int16))
    with pytest.raises(ValueError, match="contiguous rows"):
        samples_out("s16", "stream", 3, 7, np.zeros((7, 3), np.int16).T)
    pay, lens, ppitch = payload_args([b"abc", b"", bytearray(b"xy")])
    assert pay.tolist() == [[97, 98, 99], [0, 0, 0], [120, 121, 0]] and lens.tolist() == [3, 0, 2] and ppitch == 3
    assert payload_args([b""])[2] == 1


def test_compute_entry_points_fail_loudly_without_gpu():
    import __graft_entry__ as ge
    ge.build()
    import webaudio_modem_amd as wm
    from webaudio_modem_amd import _lib
    L = _lib.lib()
    if L.fskhip_device_count() > 0:
        pytest.skip("a GPU is present")
    src, dst = np.zeros(64, np.float32), np.zeros(64, np.int16)
    with pytest.raises(wm.FskHipError) as ei:
        wm.egress_device(src.ctypes.data, 8, None, 2, 8, "s16", "stream", dst.ctypes.data, 8)
    assert ei.value.code == _lib.E_NO_DEVICE and "no CPU fallback" in str(ei.value)
    assert not dst.any()
    with pytest.raises(wm.FskHipError) as ei:
        wm.FSKEngine(1, {}).modulate_samples([b"x"], "mulaw")
    assert ei.value.code == _lib.E_NO_DEVICE
