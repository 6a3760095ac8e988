"""Which kernel a fskhip_demodulate_device call runs on (csrc/fsk_plan.h), through the C ABI on the GPU (-m gpu): the names
fskhip_last_kernel reports over a grid of batch sizes, call sequences and "kernel" spellings, typed in.  The shapes are the
smallest at which a rule can flip; tests/test_plan_cpu.py checks the rules themselves without a GPU."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BELL = dict(baudRate=1200, markFrequency=1200, spaceFrequency=2200)      # dsSPB = 20
PITCH = 256
B4 = "fsk::demod_blk_kernel<false, true, false>"                         # <write-back, uniform, time-sliced>
B4R = "fsk::demod_blk_kernel_r<false, false>"                            # <write-back, time-sliced>
PIPE, FUSED, TAIL = "fsk::demod_pipe_kernel<false, true>", "fsk::demod_fused_kernel<false, true>", "fsk::demod_tail_kernel"
F64, F64_TWO = "fsk::demod_kernel<double, ...>", "fsk::demod_kernel<double, ..., two waves>"


def _compute_units(wm):
    """the device's CU count as the engine sees it: groups of 8 streams are the engine's choice while each has a CU to itself"""
    lo, hi = 1, 4096
    while lo < hi:
        mid = (lo + hi + 1) // 2
        eng = wm.FSKEngine(8 * mid, BELL)
        lo, hi = (mid, hi) if eng.blk_lanes() == 8 else (lo, mid - 1)
        eng.close()
    return lo


def test_kernel_choice_is_unchanged():
    import webaudio_modem_amd as wm
    cus = _compute_units(wm)
    gen = wm.FSKEngine(65600, BELL)
    d_x = gen.device_malloc((65600 * PITCH + 4) * 4)
    gen.h2d(d_x, np.zeros(65600 * PITCH + 4, np.float32))
    out_pitch = gen.max_bytes(PITCH)
    d_out, d_cnt, d_eod = gen.device_malloc(65600 * out_pitch), gen.device_malloc(65600 * 4), gen.device_malloc(65600 * 4)

    def run(S, calls, options=None, precision=wm.PRECISION_F32, trace=False, names=None):
        """calls: (n, pitch, pointer offset in floats) or n -> the kernel names, one engine; names(eng): the expected ones"""
        eng = wm.FSKEngine(S, BELL, precision=precision, options=dict({"blk_resets": 0}, **(options or {})))
        if trace:
            eng.trace_enable(0, 256)
        got = []
        for c in calls:
            n, pitch, off = c if isinstance(c, tuple) else (c, PITCH, 0)
            eng.demodulate_device(d_x + 4 * off, n, pitch, d_out, out_pitch, d_cnt, d_eod)
            got.append(eng.last_kernel())
        eng.synchronize()
        want = names(eng) if callable(names) else names
        eng.close()
        assert got == want, (S, calls, options, got, want)

    b6 = lambda eng: "fsk::demod_blk6_kernel<false, %d>" % eng.blk_lanes()
    # seven waves: up to one workgroup per compute unit, calls of at least eight tiles (112 against 128 samples)
    run(2048, [16, 112, 128], names=lambda e: [B4, B4, b6(e)])
    run(64 * cus, [16, 112, 128], names=[B4, B4, "fsk::demod_blk6_kernel<false, 64>"])
    run(64 * cus + 64, [16, 112, 128], names=[B4, B4, B4])
    # one round of resident workgroups (1 024 on 256 compute units) and one group beyond it: a call too short for two time slices
    # is round 2's -- one wave per group, since five 36 432-byte tiles do not fit a compute unit's LDS
    run(65536, [16, 112, 128, 256], names=[B4] * 4)
    run(65600, [16, 112, 128, 256], names=[FUSED] * 4)
    # an odd-length call, then the heads that close the pair and reach the amplitude ring's quad grid: 7 (121 samples left: seven
    # tiles), 7, no tiles at all, 6 (ring at 1: 127 left), 1 (ring at 3 with the pair open: 128 left)
    run(2048, [129, 128, 135, 2, 133, 129], names=lambda e: [b6(e), B4, b6(e), TAIL, B4, b6(e)])
    # rows off the 16-byte grid are sample by sample; a pointer that is only dword-aligned is not
    run(2048, [(128, 129, 0), (128, PITCH, 1), (128, PITCH, 0)], names=lambda e: [TAIL, b6(e), b6(e)])
    run(2048, [128], trace=True, names=[TAIL])
    run(2048, [128, 63], precision=wm.PRECISION_F64, options={"exact_waves": 1}, names=[F64, F64])
    run(2048, [128, 63], precision=wm.PRECISION_F64, options={"exact_waves": 2}, names=[F64_TWO, F64_TWO])
    # every spelling of "kernel"; a pinned kernel takes the short call too
    for spelling, names in (("auto", lambda e: [B4, b6(e)]), ("auto-r04", [B4, B4]), ("auto-r02", [PIPE, PIPE]), ("seven-wave", lambda e: [b6(e), b6(e)]),
                            ("six-wave", lambda e: [b6(e), b6(e)]), ("four-wave", [B4, B4]), ("two-wave", [PIPE, PIPE]), ("one-wave", [FUSED, FUSED])):
        run(2048, [16, 128], options={"kernel": spelling}, names=names)
    run(2048, [128], options={"kernel": "four-wave", "blk_resets": 1}, names=[B4R])
    for p in (d_x, d_out, d_cnt, d_eod):
        gen.device_free(p)
    gen.close()
