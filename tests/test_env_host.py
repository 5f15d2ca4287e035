"""The parts of the envelope accumulator that need no device (include/iqgpu.h "envelope"): the row arithmetic and the option checks,
the struct layouts, the float64 model's order against math.fsum, and the burst finder and the floor against the Python restatement in
env_model.py -- hand-made row vectors for each rule, then seeded random ones."""
import ctypes as C
import math

import numpy as np
import pytest

import env_model
from iq_tool_amd import _lib, env

B = 64


def rc_of(fn, *args):
    return getattr(_lib.load(), fn)(*args)


def rowsum(means, b=B):
    """row_sum of rows with these mean powers (small integers: exact in float)"""
    return np.asarray(means, np.float32) * np.float32(b)


def test_rows_arithmetic_and_option_validation():
    assert env.env_opts().block_frames == 4096
    for b in (64, 1024, 4096, 1 << 24):
        for frames in (0, 1, b - 1, b, b + 1, 5 * b + 17, (1 << 40) + 3):
            assert env.rows(frames, b) == frames // b
    n = C.c_uint64(7)
    for bad in (0, 32, 96, 100, 4095, 1 << 25, (1 << 24) + 1):
        o = _lib.EnvOpts(bad)
        assert rc_of("iqgpu_env_rows", C.byref(o), 1000, C.byref(n)) == -1, bad
        h = C.c_void_p()
        assert rc_of("iqgpu_env_create", 0, 3, C.byref(o), C.byref(h)) == -1 and not h.value, bad     # refused before any device is looked for
    assert rc_of("iqgpu_env_rows", None, 1000, C.byref(n)) == -1
    assert rc_of("iqgpu_env_rows", C.byref(_lib.EnvOpts(64)), 1000, None) == -1
    assert rc_of("iqgpu_env_max_rows", None, 1000) == 0


def test_struct_layouts():
    u32, u64, f64 = C.sizeof(C.c_uint32), C.sizeof(C.c_uint64), C.sizeof(C.c_double)
    assert C.sizeof(_lib.EnvOpts) == u32
    assert C.sizeof(_lib.EnvInfo) == 3 * u64 + 2 * u32 and _lib.EnvInfo.open_frames.offset == 24 and _lib.EnvInfo.block_frames.offset == 28
    assert C.sizeof(_lib.EnvBurstOpts) == 4 * u32 + 2 * f64 and _lib.EnvBurstOpts.on.offset == 16 and _lib.EnvBurstOpts.off.offset == 24
    assert C.sizeof(_lib.EnvBurst) == 3 * u64 + f64 and _lib.EnvBurst.peak_mean.offset == 24
    # the library writes the fields where the mirrors read them
    o = _lib.EnvOpts(0)
    _lib.load().iqgpu_env_opts_init(C.byref(o))
    assert o.block_frames == 4096
    got = env.bursts(rowsum([0, 9, 7, 0]), B, on=5, off=5)
    assert got == [dict(first_frame=B, frames=2 * B, peak_row=1, peak_mean=9.0)]


class _FakeOracle:
    """cf32 only: the unpack at gain 1 is the identity"""
    @staticmethod
    def to_cf32(raw, fmt, gain):
        assert fmt == "cf32" and gain == 1.0
        return np.ascontiguousarray(raw).view(np.complex64).copy()


@pytest.mark.parametrize("b", (64, 1024, 2048, 65536, 131072))
def test_the_models_order_matters_only_in_the_last_bits(b):
    rng = np.random.default_rng(b)
    n = 2 * b + 17
    x = (rng.standard_normal((n, 2)) * 0.3).astype(np.float32)
    s, k, r, open_row, nonfinite = env_model.model(x, "cf32", b, _FakeOracle)
    p = x.astype(np.float64)[:, 0] ** 2 + x.astype(np.float64)[:, 1] ** 2
    assert s.size == 2 and nonfinite == 0
    for i in range(2):
        exact = math.fsum(p[i * b:(i + 1) * b])
        # b - 1 additions of non-negative terms in any order: |model - exact| <= b 2^-53 exact before the rounding to float
        assert abs(float(s[i]) - exact) <= (b * 2.0 ** -53 + 2.0 ** -24) * exact
        assert k[i] == np.float32(p[i * b:(i + 1) * b].max())
    assert abs(open_row[0] - math.fsum(p[2 * b:])) <= 17 * 2.0 ** -53 * math.fsum(p[2 * b:]) and open_row[1] == p[2 * b:].max()
    # B <= 1024: the balanced adjacent-pair tree over the row's terms
    if b <= 1024:
        assert s[0] == np.float32(env_model.tree(p[:b]))


# ---- the burst finder: one hand-made vector per rule ----
def both(means, **kw):
    kw = dict(dict(on=10.0, off=5.0, min_rows=1, hang_rows=0, pad_rows=0), **kw)
    v = rowsum(means)
    got, want = env.bursts(v, B, **kw), env_model.bursts(v, B, **kw)
    assert got == want, (means, kw, got, want)
    return [(g["first_frame"] // B, g["frames"] // B) for g in got]


def test_burst_opens_at_on_and_closes_below_off():
    assert both([0, 0, 12, 12, 0, 0]) == [(2, 2)]
    assert both([0, 9, 12, 7, 6, 4, 12]) == [(2, 3), (6, 1)]      # 9 < on does not open; 7 and 6 >= off stay in; 4 closes
    assert both([10, 5, 4.5]) == [(0, 2)]                          # the comparisons are >= on and < off
    assert both([0, 0, 0]) == [] and both([]) == []


def test_a_dip_of_hang_rows_stays_and_one_more_closes():
    assert both([12, 0, 0, 12, 0], hang_rows=2) == [(0, 5)]        # (the last dip is no run of more than hang_rows: it lasts to the end)
    assert both([12, 0, 0, 0, 12, 0, 0, 0, 0], hang_rows=2) == [(0, 1), (4, 1)]
    assert both([12, 0, 12, 0, 0, 12], hang_rows=1) == [(0, 3), (5, 1)]


def test_min_rows_drops_short_bursts():
    assert both([12, 0, 12, 12, 0, 12, 12, 12, 0], min_rows=2) == [(2, 2), (5, 3)]
    assert both([12, 0, 12, 12, 0], min_rows=3) == []


def test_padding_joins_and_is_clipped_at_both_ends():
    assert both([12, 0, 0, 0, 0, 12, 0, 0, 0, 12], pad_rows=1) == [(0, 2), (4, 3), (8, 2)]
    assert both([0, 12, 0, 0, 12, 0, 0], pad_rows=1) == [(0, 6)]   # [0, 3) and [3, 6) touch: joined
    assert both([0, 0, 12, 0, 0, 0, 12, 0], pad_rows=5) == [(0, 8)]
    assert both([12, 0, 0, 0, 0, 0, 0, 12], pad_rows=2) == [(0, 3), (5, 3)]


def test_nan_rows_tie_for_the_peak_and_capacity():
    nan = float("nan")
    assert both([12, nan, 12, nan, nan, 12], hang_rows=1) == [(0, 3), (5, 1)]     # a NaN mean is below off
    assert both([nan, nan]) == []
    got = env.bursts(rowsum([0, 11, 15, 15, 11, 0]), B, on=10, off=5)
    assert got[0]["peak_row"] == 2 and got[0]["peak_mean"] == 15.0                 # the first of equal peaks
    v, n = rowsum([12, 0, 12, 0, 12]), C.c_size_t(0)
    o = _lib.EnvBurstOpts(B, 1, 0, 0, 10.0, 5.0)
    out = (_lib.EnvBurst * 2)()
    assert rc_of("iqgpu_env_bursts", v.ctypes.data_as(C.c_void_p), v.size, C.byref(o), C.cast(out, C.c_void_p), 2, C.byref(n)) == -8
    assert n.value == 3 and out[1].first_frame == 2 * B
    assert rc_of("iqgpu_env_bursts", v.ctypes.data_as(C.c_void_p), v.size, C.byref(o), None, 0, C.byref(n)) == -8 and n.value == 3
    assert rc_of("iqgpu_env_bursts", v.ctypes.data_as(C.c_void_p), v.size, C.byref(_lib.EnvBurstOpts(B, 1, 0, 0, 5.0, 10.0)), None, 0, C.byref(n)) == -1
    assert rc_of("iqgpu_env_bursts", v.ctypes.data_as(C.c_void_p), v.size, C.byref(_lib.EnvBurstOpts(100, 1, 0, 0, 10.0, 5.0)), None, 0, C.byref(n)) == -1


def test_bursts_and_floor_on_random_vectors():
    rng = np.random.default_rng(2024)
    for trial in range(300):
        rows = int(rng.integers(1, 60))
        v = (rng.integers(0, 20, rows).astype(np.float32) * B)
        if trial % 7 == 0:
            v[rng.integers(0, rows)] = np.nan
        off = float(rng.integers(1, 12))
        kw = dict(on=off + float(rng.integers(0, 6)), off=off, min_rows=int(rng.integers(0, 4)), hang_rows=int(rng.integers(0, 4)),
                  pad_rows=int(rng.integers(0, 3)))
        assert env.bursts(v, B, **kw) == env_model.bursts(v, B, **kw), (trial, v.tolist(), kw)
        f = float(rng.random())
        assert env.floor(v, B, f) == env_model.floor(v, B, f) or (math.isnan(env.floor(v, B, f)) and math.isnan(env_model.floor(v, B, f))), (trial, f)


def test_floor_ranks_and_refusals():
    v = rowsum([7, 1, 5, 3, 9])
    assert [env.floor(v, B, f) for f in (0.0, 0.1, 0.25, 0.5, 1.0)] == [1.0, 1.0, 3.0, 5.0, 9.0]
    assert v.tolist() == rowsum([7, 1, 5, 3, 9]).tolist()                          # selected on a copy
    m = C.c_double(0)
    for args in ((v.ctypes.data_as(C.c_void_p), 0, B, 0.1), (v.ctypes.data_as(C.c_void_p), 5, B, 1.5), (v.ctypes.data_as(C.c_void_p), 5, 100, 0.1),
                 (None, 5, B, 0.1)):
        assert rc_of("iqgpu_env_floor", *args, C.byref(m)) == -1, args
