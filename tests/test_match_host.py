"""The template-correlation accumulator, host side (include/iqgpu.h "template correlation"; no GPU call): the defaults, the row count
against the model's around every boundary, every refusal of the options and the templates that needs no device, the shift bank against
numpy, the detections on hand-made rows with the capacity answer, and the layout of the structs against the ctypes mirror."""
import ctypes as C
import os
import subprocess
import textwrap

import numpy as np
import pytest

import match_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENODEV, EFORMAT, ECAPACITY = -1, -2, -5, -8


@pytest.fixture(scope="module")
def lib():
    import iq_tool_amd
    return iq_tool_amd.load()


def test_opts_init_sets_the_documented_defaults(lib):
    from iq_tool_amd import _lib
    o = _lib.MatchOpts(7, 7, 7, 7)
    lib.iqgpu_match_opts_init(C.byref(o))
    assert (o.nfft, o.block_frames, o.n_templates, o.template_frames) == (0, 4096, 1, 0)
    lib.iqgpu_match_opts_init(None)        # tolerated


@pytest.mark.parametrize("nfft", (1024, 2048, 4096))
def test_rows_equal_the_models_count(lib, nfft):
    from iq_tool_amd import match
    V = nfft // 2
    for B in (V, 2 * V, 64 * V, 1 << 24):
        row_end = nfft + (B // V - 1) * V                    # the frame count that finishes row 0
        sweep = {0, 1, 5 * nfft + 3, 70_000, (1 << 31) + 5, 1 << 39}
        for centre in (nfft, row_end, row_end + B, row_end + 2 * B):
            sweep |= {centre - 1, centre, centre + 1, centre + V - 1, centre + V}
        for frames in sorted(sweep):
            assert match.rows(frames, 16, 3, B, nfft) == match_model.rows_of(frames, nfft, B), (nfft, B, frames)
        assert match.rows(row_end - 1, 16, 1, B, nfft) == 0 and match.rows(row_end, 16, 1, B, nfft) == 1


def test_nfft_zero_is_the_smallest_size_that_holds_the_template(lib):
    from iq_tool_amd import match
    for L, nfft in ((2, 1024), (513, 1024), (514, 2048), (1025, 2048), (1026, 4096), (2049, 4096)):
        assert match_model.nfft_of(0, L) == nfft
        for frames in (nfft - 1, nfft, nfft + nfft // 2 - 1, nfft + nfft // 2):
            assert match.rows(frames, L, 1, nfft // 2) == match_model.rows_of(frames, nfft, nfft // 2), (L, frames)
        assert match.rows(1 << 20, L, 1, 4096) == match_model.rows_of(1 << 20, nfft, 4096)


def test_refusals_that_need_no_device(lib):
    from iq_tool_amd import _lib
    from iq_tool_amd.match import match_opts
    n64, h = C.c_uint64(0), C.c_void_p()
    taps = np.ones(2 * 8 * 2049, np.float32)
    tp = taps.ctypes.data_as(C.c_void_p)
    bad = [match_opts(1, 1, 1024, 1024), match_opts(0, 1, 1024, 1024), match_opts(514, 1, 1024, 1024), match_opts(1026, 1, 1024, 2048),
           match_opts(2050, 1, 4096, 4096), match_opts(2050, 1, 4096, 0), match_opts(16, 1, 256, 1024), match_opts(16, 1, 1024, 4096),
           match_opts(16, 1, 1536, 1024), match_opts(16, 1, 1000, 1024), match_opts(16, 1, 1 << 25, 1024), match_opts(16, 1, 0, 1024),
           match_opts(16, 0, 1024, 1024), match_opts(16, 9, 1024, 1024), match_opts(16, 1, 1024, 512), match_opts(16, 1, 8192, 8192),
           match_opts(16, 1, 1024, 1000)]
    for o in bad:
        what = (o.template_frames, o.n_templates, o.block_frames, o.nfft)
        assert lib.iqgpu_match_rows(C.byref(o), 1 << 20, C.byref(n64)) == EINVAL, what
        assert lib.iqgpu_match_create(0, _lib.FMT["cs16"], C.byref(o), tp, C.byref(h)) == EINVAL and not h.value, what
        assert lib.iqgpu_last_error()
    for o in (match_opts(2, 1, 512, 1024), match_opts(513, 8, 1 << 24, 1024), match_opts(2049, 8, 2048, 4096), match_opts(2049, 1, 2048, 0)):
        assert lib.iqgpu_match_rows(C.byref(o), 1 << 20, C.byref(n64)) == 0
    good = match_opts(16, 2, 1024, 1024)
    # the templates: a NaN or Inf tap anywhere, a template without energy (the second of two)
    for at, v in ((0, np.nan), (63, np.inf), (33, -np.inf)):
        t = np.ones(64, np.float32)
        t[at] = v
        assert lib.iqgpu_match_create(0, _lib.FMT["cs16"], C.byref(good), t.ctypes.data_as(C.c_void_p), C.byref(h)) == EINVAL and not h.value
        assert b"finite" in lib.iqgpu_last_error()
    t = np.ones(64, np.float32)
    t[32:] = 0.0
    assert lib.iqgpu_match_create(0, _lib.FMT["cs16"], C.byref(good), t.ctypes.data_as(C.c_void_p), C.byref(h)) == EINVAL and not h.value
    assert b"energy" in lib.iqgpu_last_error()
    x = (C.c_float * 16)()
    got = C.c_size_t(5)
    # NULL arguments
    assert lib.iqgpu_match_rows(None, 4096, C.byref(n64)) == EINVAL
    assert lib.iqgpu_match_rows(C.byref(good), 4096, None) == EINVAL
    assert lib.iqgpu_match_create(0, _lib.FMT["cs16"], None, tp, C.byref(h)) == EINVAL
    assert lib.iqgpu_match_create(0, _lib.FMT["cs16"], C.byref(good), None, C.byref(h)) == EINVAL
    assert lib.iqgpu_match_create(0, _lib.FMT["cs16"], C.byref(good), tp, None) == EINVAL
    assert lib.iqgpu_match_reset(None) == EINVAL
    assert lib.iqgpu_match_push(None, x, 16, None, None, None, 0, C.byref(got)) == EINVAL and got.value == 0
    got.value = 5
    assert lib.iqgpu_match_push_device(None, x, 16, None, None, None, 0, C.byref(got), None) == EINVAL and got.value == 0
    assert lib.iqgpu_match_read_open(None, None, None, None, None) == EINVAL
    assert lib.iqgpu_match_max_rows(None, 1 << 20) == 0
    lib.iqgpu_match_destroy(None)          # tolerated
    # an unknown format, with good options and templates
    for fmt in (0, 7, 17, -1):
        assert lib.iqgpu_match_create(0, fmt, C.byref(good), tp, C.byref(h)) == EFORMAT and not h.value


def test_create_without_a_device_answers_enodev(lib):
    from iq_tool_amd import _lib
    if lib.iqgpu_device_count() > 0:
        return                             # (on a machine with a device tests/test_gpu_match.py creates handles)
    import iq_tool_amd
    with pytest.raises(_lib.IqgpuError) as e:
        iq_tool_amd.Match("cs16", np.ones(16, np.complex64), 1024)
    assert e.value.code == ENODEV


def ulps(a, b):
    """the distance of two float32 arrays in units of the last place of b"""
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.abs(b).astype(np.float32)).astype(np.float64)


def test_shift_bank_against_numpy_to_one_ulp(lib):
    from iq_tool_amd import match
    rate, hz = 2.4e6, [-37500.0, -1234.5, 0.0, 999.75, 600e3]
    tmpl = match_model.templates(1, 513, 3)[0] * np.float32(0.7)
    got = match.shift_bank(tmpl, hz, rate)
    assert got.shape == (5, 513) and got.dtype == np.complex64
    k = np.arange(513)
    for i, f in enumerate(hz):
        want = tmpl.astype(np.complex128) * np.exp(2j * np.pi * f * k / rate)
        w32 = want.astype(np.complex64)
        assert ulps(got[i].real, w32.real).max() <= 1 and ulps(got[i].imag, w32.imag).max() <= 1, i
        # ... and the error against the unrounded value is that of one rounding of a component, up to numpy's own last bits
        assert np.abs(got[i] - want).max() <= 2.0 ** -24
    assert got[2].tobytes() == tmpl.tobytes()                                  # hz = 0: the template itself
    # refusals
    out = np.zeros(16, np.complex64)
    t, f = tmpl[:16].copy(), np.array([1.0, np.nan])
    args = lambda tp, fp, n, fs, op: lib.iqgpu_match_shift_bank(tp, 16, fp, n, fs, op)          # noqa: E731
    tp, fp, op = t.ctypes.data_as(C.c_void_p), f.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    assert args(tp, fp, 1, 2.4e6, op) == 0
    assert args(None, fp, 1, 2.4e6, op) == args(tp, None, 1, 2.4e6, op) == args(tp, fp, 1, 2.4e6, None) == EINVAL
    assert args(tp, fp, 0, 2.4e6, op) == args(tp, fp, 1, 0.0, op) == args(tp, fp, 1, float("nan"), op) == args(tp, fp, 2, 2.4e6, op) == EINVAL


def test_peaks_on_hand_made_rows(lib):
    from iq_tool_amd import _lib, match
    B, L = 1024, 16
    # rows x 2 templates.  The mean of the other positions is (sum - peak) / 1023
    pk = np.array([[50.0, 1.0], [0.0, 9.0], [4.0, np.nan], [10.0, 10.0]], np.float32)
    at = np.array([[7, 3], [0, 1023], [5, 5], [0, 512]], np.uint32)
    sm = np.array([[50.0 + 1023.0, 1.0 + 1023.0], [0.0, 9.0], [4.0 + 1023.0 * 0.5, np.nan], [10.0 + 1023.0, 10.0 + 1023.0 * 1.25]], np.float32)
    got = match.peaks(pk, at, sm, B, L, 8.0)
    assert got == [dict(first_frame=7, template=0, peak=50.0, ratio=50.0), dict(first_frame=B + 1023, template=1, peak=9.0, ratio=float("inf")),
                   dict(first_frame=2 * B + 5, template=0, peak=4.0, ratio=8.0), dict(first_frame=3 * B, template=0, peak=10.0, ratio=10.0),
                   dict(first_frame=3 * B + 512, template=1, peak=10.0, ratio=8.0)]
    # the bar is >=: a hair above the ratio of row 2 drops it; an all-zero row and a NaN row are never detections
    assert [d["first_frame"] for d in match.peaks(pk, at, sm, B, L, 8.000001)] == [7, B + 1023, 3 * B]
    assert len(match.peaks(pk, at, sm, B, L, 0.0)) == 6
    assert match.peaks(pk[:0], at[:0], sm[:0], B, L, 8.0) == []
    # capacity: the count needed comes back with IQGPU_ECAPACITY, the first `cap` are written
    o, n = match.match_opts(L, 2, B, 1024), C.c_size_t(0)
    out = (_lib.MatchPeak * 2)()
    ptr = [a.ctypes.data_as(C.c_void_p) for a in (pk, at, sm)]
    assert lib.iqgpu_match_peaks(*ptr, 4, C.byref(o), 8.0, out, 2, C.byref(n)) == ECAPACITY and n.value == 5
    assert (out[0].first_frame, out[1].first_frame, out[1].template_index) == (7, B + 1023, 1)
    assert lib.iqgpu_match_peaks(*ptr, 4, C.byref(o), 8.0, None, 0, C.byref(n)) == ECAPACITY and n.value == 5
    with pytest.raises(_lib.IqgpuError) as e:
        match.peaks(pk, at, sm, B, L, 8.0, cap=4)
    assert e.value.code == ECAPACITY
    # refusals
    assert lib.iqgpu_match_peaks(*ptr, 4, C.byref(o), 8.0, out, 2, None) == EINVAL
    assert lib.iqgpu_match_peaks(None, ptr[1], ptr[2], 4, C.byref(o), 8.0, out, 2, C.byref(n)) == EINVAL
    assert lib.iqgpu_match_peaks(*ptr, 4, None, 8.0, out, 2, C.byref(n)) == EINVAL
    for ratio in (-1.0, float("nan"), float("inf")):
        assert lib.iqgpu_match_peaks(*ptr, 4, C.byref(o), ratio, out, 2, C.byref(n)) == EINVAL


def test_match_struct_layouts_match_ctypes(tmp_path):
    from iq_tool_amd import _lib
    names = dict(iqgpu_match_opts=_lib.MatchOpts, iqgpu_match_info=_lib.MatchInfo, iqgpu_match_peak=_lib.MatchPeak)
    assert [n for n, _ in _lib.MatchOpts._fields_] == ["nfft", "block_frames", "n_templates", "template_frames"]
    assert [n for n, _ in _lib.MatchInfo._fields_] == ["frames", "segments", "rows", "open_segments", "nfft", "block_frames", "n_templates",
                                                      "template_frames", "reserved", "template_energy"]
    assert [n for n, _ in _lib.MatchPeak._fields_] == ["first_frame", "template_index", "peak", "ratio"]
    lines, want = [], []
    for cname, T in names.items():
        lines.append('printf("%%zu ", sizeof(%s));' % cname)
        want.append(C.sizeof(T))
        for n, _ in T._fields_:
            lines.append('printf("%%zu ", offsetof(%s, %s));' % (cname, n))
            want.append(getattr(T, n).offset)
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
    assert got == want
    assert [C.sizeof(T) for T in names.values()] == [16, 112, 24]
