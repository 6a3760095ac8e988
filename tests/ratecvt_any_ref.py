"""The model of the rate converter's calls of any length (include/fskhip_next.h: "Rate conversion in calls of any length"), on top
of ratecvt_ref.py: the whole signal zero-padded to whole periods goes through ratecvt_ref.convert, and the first ceil(N L / M)
outputs are the signal's -- the filter is causal, so the padding cannot reach them.  A call from position pos with history hist
is the same with pos inputs in front of it, of which the last H are the history (the ones before are never read by the call's
outputs).  The counts are in integers.  Not a test; test_ratecvt_any_cpu.py holds it against itself under cuts and the oracle,
test_gpu_ratecvt_any.py the kernels against it."""
import numpy as np

import ratecvt_ref as rc
import samples_ref as sr


def first_output(L, M, pos):
    """ceil(pos L / M): the first output of the period grid whose newest input is at or behind grid input pos"""
    return -(-(pos * L) // M)


def out_count_any(L, M, pos, n):
    return first_output(L, M, pos + n) - first_output(L, M, pos)


def in_count_any(L, M, pos, n_out):
    """the smallest n with out_count_any(L, M, pos, n) >= n_out"""
    return (first_output(L, M, pos) + n_out - 1) * M // L + 1 - pos if n_out else 0


def convert_whole(x, taps, L, M):
    """float32 [S, N], any N, from a fresh handle -> float32 [S, ceil(N L / M)]"""
    x = np.atleast_2d(np.asarray(x, np.float32))
    S, N = x.shape
    pad = np.zeros((S, -(-N // M) * M), np.float32)
    pad[:, :N] = x
    return rc.convert(pad, taps, L, M)[0][:, :first_output(L, M, N)]


def convert_any(x, taps, L, M, pos=0, hist=None):
    """one call: float32 [S, n] from position pos behind history hist (None: zeros) -> (float32 [S, out_count_any(pos, n)], the
    history the call leaves, the position it leaves)"""
    x = np.atleast_2d(np.asarray(x, np.float32))
    S, n = x.shape
    H = rc.history(L, np.asarray(taps).size)
    hist = np.zeros((S, H), np.float32) if hist is None else np.asarray(hist, np.float32).reshape(S, H)
    # the grid from the period boundary: inputs -H .. pos - 1 of it are pos zeros (older than the history: no output of the call
    # reads them) and the history; the first H of them are convert()'s own history, the rest lie in front of the call
    pre = np.concatenate([np.zeros((S, pos), np.float32), hist], axis=1)
    front, lead = pre[:, :H], pre[:, H:]
    grid = np.concatenate([lead, x], axis=1)
    pad = np.zeros((S, -(-grid.shape[1] // M) * M), np.float32)
    pad[:, :grid.shape[1]] = grid
    y = rc.convert(pad, taps, L, M, front)[0] if pad.shape[1] else np.zeros((S, 0), np.float32)
    q0, q1 = first_output(L, M, pos), first_output(L, M, pos + n)
    xx = np.concatenate([hist, x], axis=1)
    return y[:, q0:q1], xx[:, xx.shape[1] - H:].copy(), (pos + n) % M


def capture_any(x, fmt, taps, L, M, pos=0, hist=None):
    return convert_any(sr.decode(np.atleast_2d(np.asarray(x)), fmt), taps, L, M, pos, hist)


def playback_any(x, taps, L, M, fmt, lens=None, pos=0, hist=None):
    """lens: row s reads as 0.0 from lens[s] on, counted from the call's first input"""
    x = np.atleast_2d(np.asarray(x, np.float32))
    if lens is not None:
        x = np.where(np.arange(x.shape[1])[None, :] < np.asarray(lens, np.int64)[:, None], x, np.float32(0.0))
    y, h, p = convert_any(x, taps, L, M, pos, hist)
    return sr.encode(y, fmt), h, p
