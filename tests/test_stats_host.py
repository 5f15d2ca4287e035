"""The capture-statistics accumulator, host side (include/iqgpu.h "capture statistics"; no GPU call): the layout of the two structs
against the ctypes mirror, iqgpu_stats_merge on hand-built results (identity, both groupings of three pieces, the tie rule, the
peak_frame offset), iqgpu_stats_derive against the header's formulas restated in numpy float64 (1e-12 relative: both sides evaluate one
written-down formula on the same doubles, so only libm's last bits differ), and every refusal that needs no device."""
import ctypes as C
import os
import subprocess
import textwrap

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENODEV, EFORMAT = -1, -2, -5
EXACT = ("frames", "nonfinite_frames", "rail_lo", "rail_hi", "hist", "min", "max", "peak_power", "peak_frame")


@pytest.fixture(scope="module")
def lib():
    import iq_tool_amd
    return iq_tool_amd.load()


def test_stats_struct_layouts_match_ctypes(tmp_path):
    from iq_tool_amd import _lib
    rfields = [n for n, _ in _lib.StatsResult._fields_]
    dfields = [n for n, _ in _lib.StatsDerived._fields_]
    assert rfields == ["frames", "nonfinite_frames", "rail_lo", "rail_hi", "hist", "min", "max", "peak_power", "peak_frame", "sum", "sum_sq", "sum_iq"]
    assert dfields == ["n", "mean_i", "mean_q", "power", "rms_dbfs", "peak_dbfs", "crest_db", "var_i", "var_q", "iq_gain_ratio", "iq_phase_rad",
                       "clip_fraction", "bins_used"]
    lines = ['printf("%zu %zu ", sizeof(iqgpu_stats_result), sizeof(iqgpu_stats_derived));']
    lines += ['printf("%%zu ", offsetof(iqgpu_stats_result, %s));' % n for n in rfields]
    lines += ['printf("%%zu ", offsetof(iqgpu_stats_derived, %s));' % n for n in dfields]
    prog = textwrap.dedent("""
        #include <stdio.h>
        #include <stddef.h>
        #include "iqgpu.h"
        int main(void) {
            %s
            return 0;
        }""") % "\n    ".join(lines)
    src = tmp_path / "layout.c"
    src.write_text(prog)
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    R, D = _lib.StatsResult, _lib.StatsDerived
    want = [C.sizeof(R), C.sizeof(D)] + [getattr(R, n).offset for n in rfields] + [getattr(D, n).offset for n in dfields]
    assert got == want
    assert (C.sizeof(R), C.sizeof(D)) == (8 * 6 + 8 * 512 + 16 + 16 + 40, 8 + 88 + 8)


def piece(seed, frames, nonfinite=0, peak=None, peak_frame=None):
    """a hand-built, self-consistent result of `frames` frames, `nonfinite` of them non-finite"""
    from iq_tool_amd import _lib, stats
    rng = np.random.default_rng(seed)
    r = _lib.StatsResult()
    r.frames, r.nonfinite_frames = frames, nonfinite
    n = frames - nonfinite
    if n:
        for c in range(2):
            stats.view(r, "hist")[c] = rng.multinomial(n, np.full(256, 1 / 256))
            stats.view(r, "rail_lo")[c], stats.view(r, "rail_hi")[c] = rng.integers(0, n + 1, 2)
            stats.view(r, "min")[c], stats.view(r, "max")[c] = np.sort(rng.uniform(-1, 1, 2).astype(np.float32))
            stats.view(r, "sum")[c], stats.view(r, "sum_sq")[c] = rng.uniform(-n, n), rng.uniform(0, n)
        r.peak_power = float(rng.uniform(0.1, 2.0)) if peak is None else peak
        r.peak_frame = int(rng.integers(0, frames)) if peak_frame is None else peak_frame
        r.sum_iq = rng.uniform(-n, n)
    return r


def exact(r):
    from iq_tool_amd import stats
    d = stats.as_dict(r)
    return {k: d[k] for k in EXACT}


def test_merge_identity_and_sides_without_finite_frames():
    from iq_tool_amd import _lib, stats
    a = piece(1, 1000)
    for empty in (_lib.StatsResult(), piece(2, 7, nonfinite=7)):
        left = stats.merge(stats.copy(empty), a)                      # empty in front: a, its peak moved behind the empty frames
        want = stats.as_dict(a)
        want["frames"] += empty.frames; want["nonfinite_frames"] += empty.nonfinite_frames; want["peak_frame"] += empty.frames
        assert stats.as_dict(left) == want
        right = stats.merge(stats.copy(a), empty)                     # empty behind: a
        want = stats.as_dict(a)
        want["frames"] += empty.frames; want["nonfinite_frames"] += empty.nonfinite_frames
        assert stats.as_dict(right) == want
    both = stats.merge(_lib.StatsResult(), _lib.StatsResult())
    assert bytes(both) == bytes(C.sizeof(_lib.StatsResult))


@pytest.mark.parametrize("seeds", [(3, 4, 5), (6, 7, 8), (9, 10, 11)])
def test_merge_is_associative_in_every_exact_field(seeds):
    from iq_tool_amd import stats
    a, b, c = piece(seeds[0], 1000, nonfinite=3), piece(seeds[1], 77), piece(seeds[2], 50_000, nonfinite=1)
    left = stats.merge(stats.merge(stats.copy(a), b), c)
    right = stats.merge(stats.copy(a), stats.merge(stats.copy(b), c))
    assert exact(left) == exact(right)
    h = [stats.view(x, "hist").astype(object) for x in (a, b, c)]
    assert (stats.view(left, "hist") == h[0] + h[1] + h[2]).all()
    assert left.frames == 51_077 and left.nonfinite_frames == 4
    assert [left.min[0], left.max[1]] == [min(x.min[0] for x in (a, b, c)), max(x.max[1] for x in (a, b, c))]
    assert left.sum_iq == (a.sum_iq + b.sum_iq) + c.sum_iq and left.sum[1] == (a.sum[1] + b.sum[1]) + c.sum[1]
    # the peak: the largest, at its place in the concatenation
    off = [0, a.frames, a.frames + b.frames]
    k = int(np.argmax([x.peak_power for x in (a, b, c)]))
    assert (left.peak_power, left.peak_frame) == ((a, b, c)[k].peak_power, off[k] + (a, b, c)[k].peak_frame)


def test_merge_tie_keeps_the_earlier_frame_and_offsets_the_later():
    from iq_tool_amd import stats
    a, b, c = piece(20, 100, peak=1.5, peak_frame=40), piece(21, 200, peak=1.5, peak_frame=0), piece(22, 300, peak=1.5, peak_frame=299)
    for grouped in (stats.merge(stats.merge(stats.copy(a), b), c), stats.merge(stats.copy(a), stats.merge(stats.copy(b), c))):
        assert (grouped.peak_power, grouped.peak_frame) == (1.5, 40)
    lower = piece(23, 100, peak=1.25, peak_frame=7)
    for grouped in (stats.merge(stats.merge(stats.copy(lower), b), c), stats.merge(stats.copy(lower), stats.merge(stats.copy(b), c))):
        assert (grouped.peak_power, grouped.peak_frame) == (1.5, 100)
    assert stats.merge(stats.copy(lower), c).peak_frame == 100 + 299


def derive_model(r):
    """the header's formulas, in its operation order, in numpy float64"""
    f = np.float64
    n = r.frames - r.nonfinite_frames
    out = dict(n=n, mean_i=0.0, mean_q=0.0, power=0.0, rms_dbfs=0.0, peak_dbfs=0.0, crest_db=0.0, var_i=0.0, var_q=0.0, iq_gain_ratio=0.0,
               iq_phase_rad=0.0, clip_fraction=0.0)
    from iq_tool_amd import stats
    out["bins_used"] = [int(np.count_nonzero(stats.view(r, "hist")[c])) for c in range(2)]
    if n == 0:
        return out
    nn = f(n)
    mi, mq = f(r.sum[0]) / nn, f(r.sum[1]) / nn
    power = (f(r.sum_sq[0]) + f(r.sum_sq[1])) / nn
    rms = f(10.0) * np.log10(power) if power > 0 else f(0)
    pk = f(10.0) * np.log10(f(r.peak_power)) if r.peak_power > 0 else f(0)
    vi, vq = f(r.sum_sq[0]) / nn - mi * mi, f(r.sum_sq[1]) / nn - mq * mq
    out.update(mean_i=mi, mean_q=mq, power=power, rms_dbfs=rms, peak_dbfs=pk, crest_db=pk - rms if power > 0 and r.peak_power > 0 else f(0),
               var_i=vi, var_q=vq)
    if vq > 0 and vi >= 0:
        out["iq_gain_ratio"] = np.sqrt(vi / vq)
    if vi > 0 and vq > 0:
        out["iq_phase_rad"] = np.arcsin(np.clip((f(r.sum_iq) / nn - mi * mq) / np.sqrt(vi * vq), -1.0, 1.0))
    out["clip_fraction"] = f(int(r.rail_lo[0]) + int(r.rail_lo[1]) + int(r.rail_hi[0]) + int(r.rail_hi[1])) / (f(2.0) * nn)
    return out


def stream_result(x, nonfinite=0):
    """the result of a complex128 stream with values in (-1, 1), as a cf32 accumulator would report it (built on the host)"""
    from iq_tool_amd import _lib, stats
    x = np.asarray(x, np.complex64)
    r = _lib.StatsResult()
    r.frames, r.nonfinite_frames = x.size + nonfinite, nonfinite
    for c, v in enumerate((x.real, x.imag)):
        stats.view(r, "hist")[c] = np.bincount(np.clip(np.floor(v * 128).astype(int) + 128, 0, 255), minlength=256)
        stats.view(r, "min")[c], stats.view(r, "max")[c] = v.min(), v.max()
        stats.view(r, "sum")[c], stats.view(r, "sum_sq")[c] = v.astype(np.float64).sum(), (v.astype(np.float64) ** 2).sum()
    p = x.real.astype(np.float64) ** 2 + x.imag.astype(np.float64) ** 2
    r.peak_power, r.peak_frame = p.max(), int(p.argmax())
    r.sum_iq = (x.real.astype(np.float64) * x.imag.astype(np.float64)).sum()
    return r


def test_derive_equals_the_written_formulas():
    from iq_tool_amd import _lib, stats
    rng = np.random.default_rng(40)
    n = 20_000
    i = rng.standard_normal(n) * 0.2
    cases = [stream_result(np.clip(i + 0.05, -0.99, 0.99) + 1j * np.clip(0.8 * (i * 0.1 + rng.standard_normal(n) * 0.2) - 0.02, -0.99, 0.99), nonfinite=5),
             stream_result(np.full(100, 0.25 - 0.5j)),                 # no variance: the ratio and the phase are 0
             stream_result(np.zeros(64, np.complex64)),                # digital silence: no power, no logarithm
             stream_result(0.5 * np.exp(2j * np.pi * 0.01 * np.arange(5000))),
             piece(41, 1000, nonfinite=10), _lib.StatsResult(), piece(42, 9, nonfinite=9)]
    cases[0].rail_hi[0], cases[0].rail_lo[1] = 17, 3
    for r in cases:
        d, want = stats.as_dict(stats.derive(r)), derive_model(r)
        assert d["n"] == want["n"] and d["bins_used"] == want["bins_used"]
        for k, w in want.items():
            if k not in ("n", "bins_used"):
                # crest_db is the difference of two logarithms that are each held to 1e-12 relative: its bar is 1e-12 of their magnitudes
                scale = abs(float(want["peak_dbfs"])) + abs(float(want["rms_dbfs"])) if k == "crest_db" else abs(float(w))
                assert abs(d[k] - float(w)) <= 1e-12 * scale, (k, d[k], w)
    d = stats.derive(cases[0])
    assert d.n == n and 0.04 < d.mean_i < 0.06 and 1.0 < d.iq_gain_ratio < 1.6 and d.iq_phase_rad > 0 and d.clip_fraction == 20 / (2.0 * n)
    assert d.crest_db > 3 and d.bins_used[0] > 50
    tone = stats.derive(cases[3])
    assert abs(tone.rms_dbfs - 20 * np.log10(0.5)) < 1e-3 and abs(tone.crest_db) < 1e-3 and abs(tone.iq_gain_ratio - 1) < 1e-2
    z = stats.as_dict(stats.derive(cases[2]))
    assert z["n"] == 64 and z["bins_used"] == [1, 1] and all(z[k] == 0 for k in z if k not in ("n", "bins_used"))


def test_refusals_that_need_no_device(lib):
    from iq_tool_amd import _lib, stats
    h, r, d = C.c_void_p(), _lib.StatsResult(), _lib.StatsDerived()
    x = (C.c_float * 16)()
    assert stats.geometry() >= 1024
    lib.iqgpu_stats_geometry(None)             # tolerated
    assert lib.iqgpu_stats_create(0, _lib.FMT["cs16"], None) == EINVAL
    assert lib.iqgpu_last_error()
    for fmt in (0, 7, 17, -1):
        assert lib.iqgpu_stats_create(0, fmt, C.byref(h)) == EFORMAT and not h.value
    assert lib.iqgpu_stats_reset(None) == EINVAL
    assert lib.iqgpu_stats_push(None, x, 8) == EINVAL
    assert lib.iqgpu_stats_push_device(None, x, 8, None) == EINVAL
    assert lib.iqgpu_stats_read(None, C.byref(r)) == EINVAL
    assert lib.iqgpu_stats_merge(None, C.byref(r)) == EINVAL and lib.iqgpu_stats_merge(C.byref(r), None) == EINVAL
    assert lib.iqgpu_stats_derive(None, C.byref(d)) == EINVAL and lib.iqgpu_stats_derive(C.byref(r), None) == EINVAL
    lib.iqgpu_stats_destroy(None)              # tolerated
    with pytest.raises(KeyError):
        stats.Stats("cs12")


def test_create_without_a_device_answers_enodev(lib):
    from iq_tool_amd import _lib
    if lib.iqgpu_device_count() > 0:
        pytest.skip("a device is visible")
    h = C.c_void_p()
    assert lib.iqgpu_stats_create(0, _lib.FMT["cs16"], C.byref(h)) == ENODEV and not h.value
    with pytest.raises(_lib.IqgpuError) as e:
        import iq_tool_amd
        iq_tool_amd.Stats("cs16")
    assert e.value.code == ENODEV
