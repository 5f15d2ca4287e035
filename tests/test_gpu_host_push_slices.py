"""A host push of MORE than one slice (iqgpu_env_push / iqgpu_lag_push: 2^22 frames a slice; iqgpu_sgram_push: 2^20): the loop that
stages a slice, pushes it, copies its rows back and advances the planes (push_host_slices, accum_core.hpp) against the same bytes
pushed in pieces that are each shorter than a slice.  Piecewise pushes are held to the float64 models by the split tests of
test_gpu_env, test_gpu_lag and test_gpu_sgram, so equality with them is what is asked here: every plane and the open row, bit for bit.

Shapes: one slice, three rows (env, lag) or 96 segments (sgram) and 17 frames more, so that the second slice is short, begins
inside a row and leaves a row open; pieces of a quarter slice and 5 frames, so that no piece's seam falls on the one push's."""
import numpy as np
import pytest

from iq_tool_amd import synth

pytestmark = pytest.mark.gpu
ENV_SLICE, SGRAM_SLICE = 1 << 22, 1 << 20
B = 4096


def pushed(acc, raw, piece):
    """the planes of `raw` (cu8: two bytes a frame) pushed in host pushes of `piece` frames, each plane as bytes; the open row"""
    parts = [acc.push(raw[2 * lo:2 * (lo + piece)]) for lo in range(0, raw.size // 2, piece)]
    planes = tuple(b"".join(np.ascontiguousarray(p[i]).tobytes() for p in parts) for i in range(len(parts[0])))
    return planes, acc.read_open()


def same(a, b):
    """equal bit for bit: arrays by their bytes, floats by their bits, the rest by =="""
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.tobytes() == b.tobytes()
    if isinstance(a, float):
        return np.float64(a).tobytes() == np.float64(b).tobytes()
    return a == b


def check(make, n, slice_frames, piece, row_bytes):
    raw = synth.hash_stream(n, 31, "cu8")
    assert n > slice_frames > piece
    one, one_open = pushed(make(), raw, n)
    many, many_open = pushed(make(), raw, piece)
    assert [len(p) for p in one] == row_bytes and all(len(p) > 0 for p in one)
    for i, (a, b) in enumerate(zip(one, many)):
        assert a == b, "plane %d" % i
    assert same(one_open, many_open), (one_open, many_open)


def test_env_push_of_two_slices_equals_pieces(gpu):
    n = ENV_SLICE + 3 * B + 17
    check(lambda: gpu.Env("cu8", B), n, ENV_SLICE, (1 << 20) + 5, [4 * (n // B)] * 3)


def test_lag_push_of_two_slices_equals_pieces(gpu):
    # a near partner (out of LDS) and a far one (a second load): both reach across the slice seam, into the history
    n = ENV_SLICE + 3 * B + 17
    check(lambda: gpu.Lag("cu8", B, (1, 1500)), n, ENV_SLICE, (1 << 20) + 5, [16 * (n // B), 4 * (n // B)])


def test_sgram_push_of_two_slices_equals_pieces(gpu):
    n = SGRAM_SLICE + 3 * 16384 + 17
    rows = ((n - 1024) // 512 + 1) // 32
    check(lambda: gpu.Sgram("cu8", 1024, 512, row_segments=32), n, SGRAM_SLICE, (1 << 18) + 5, [4 * 1024 * rows] * 2)
