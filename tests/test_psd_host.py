"""The power-spectrum accumulator, host side (include/iqgpu.h "power spectrum"; no GPU call): the defaults, the window tables against
the numpy float64 formulas bit for bit, the segment count against its closed form, every refusal that needs no device, the answer of
create where no device is visible, and the layout of the two structs against the ctypes mirror."""
import ctypes as C
import os
import subprocess
import textwrap

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENODEV, EFORMAT = -1, -2, -5
WINDOWS = ("rect", "hann", "hamming", "blackman_harris")
SIZES = (1024, 2048, 4096)


@pytest.fixture(scope="module")
def lib():
    import iq_tool_amd
    return iq_tool_amd.load()


def formula(window, n):
    """the periodic windows of the header, in float64"""
    i = np.arange(n, dtype=np.float64)
    if window == "rect":
        return np.ones(n)
    if window == "hann":
        return 0.5 - 0.5 * np.cos(2 * np.pi * i / n)
    if window == "hamming":
        return 0.54 - 0.46 * np.cos(2 * np.pi * i / n)
    return 0.35875 - 0.48829 * np.cos(2 * np.pi * i / n) + 0.14128 * np.cos(4 * np.pi * i / n) - 0.01168 * np.cos(6 * np.pi * i / n)


def test_opts_init_sets_the_documented_defaults(lib):
    from iq_tool_amd import _lib
    o = _lib.PsdOpts(7, 7, 7, 7.0)
    lib.iqgpu_psd_opts_init(C.byref(o))
    assert (o.nfft, o.hop, o.window, o.gain) == (1024, 512, _lib.PSD_WINDOW["hann"], 1.0)
    assert _lib.PSD_WINDOW == dict(rect=0, hann=1, hamming=2, blackman_harris=3)
    lib.iqgpu_psd_opts_init(None)          # tolerated


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("window", WINDOWS)
def test_window_is_the_float64_formula_rounded_once(lib, window, n):
    from iq_tool_amd import psd
    w, s, q = psd.window(n, window)
    want = formula(window, n).astype(np.float32)
    assert w.dtype == np.float32 and w.tobytes() == want.tobytes()
    w64 = w.astype(np.float64)
    assert abs(s - w64.sum()) <= 1e-12 * w64.sum()
    assert abs(q - (w64 * w64).sum()) <= 1e-12 * (w64 * w64).sum()


@pytest.mark.parametrize("n", SIZES)
def test_segments_equal_the_closed_form(lib, n):
    from iq_tool_amd import psd
    for hop in (n, n // 2, n // 4):
        sweep = [0, 1, n - 1, n, n + 1, n + hop - 1, n + hop, n + hop + 1, 5 * n + 3, 70_000, (1 << 31) + 5, 1 << 39]
        for frames in sweep:
            assert psd.segments(frames, n, hop) == (0 if frames < n else (frames - n) // hop + 1), (n, hop, frames)


def test_refusals_that_need_no_device(lib):
    from iq_tool_amd import _lib
    from iq_tool_amd.psd import psd_opts
    w = np.empty(4096, np.float32)
    wp = w.ctypes.data_as(C.c_void_p)
    n64, h = C.c_uint64(0), C.c_void_p()
    s = C.c_double(0)
    bad = [psd_opts(nfft=512, hop=256), psd_opts(nfft=8192, hop=4096), psd_opts(nfft=1000, hop=500), psd_opts(nfft=1024, hop=128),
           psd_opts(nfft=1024, hop=0), psd_opts(nfft=1024, hop=2048), psd_opts(nfft=2048, hop=768), psd_opts(window=4), psd_opts(window=-1),
           psd_opts(gain=float("nan")), psd_opts(gain=float("inf")), psd_opts(gain=float("-inf"))]
    for o in bad:
        assert lib.iqgpu_psd_window(C.byref(o), wp, w.size, C.byref(s), C.byref(s)) == EINVAL
        assert lib.iqgpu_psd_segments(C.byref(o), 4096, C.byref(n64)) == EINVAL
        assert lib.iqgpu_psd_create(0, _lib.FMT["cs16"], C.byref(o), C.byref(h)) == EINVAL and not h.value
        assert lib.iqgpu_last_error()
    good = psd_opts()
    # NULL arguments
    assert lib.iqgpu_psd_window(None, wp, w.size, None, None) == EINVAL
    assert lib.iqgpu_psd_window(C.byref(good), None, w.size, None, None) == EINVAL
    assert lib.iqgpu_psd_segments(None, 4096, C.byref(n64)) == EINVAL
    assert lib.iqgpu_psd_segments(C.byref(good), 4096, None) == EINVAL
    assert lib.iqgpu_psd_create(0, _lib.FMT["cs16"], None, C.byref(h)) == EINVAL
    assert lib.iqgpu_psd_create(0, _lib.FMT["cs16"], C.byref(good), None) == EINVAL
    assert lib.iqgpu_psd_reset(None) == EINVAL
    assert lib.iqgpu_psd_push(None, wp, 16) == EINVAL
    assert lib.iqgpu_psd_push_device(None, wp, 16, None) == EINVAL
    assert lib.iqgpu_psd_read(None, None, None, None) == EINVAL
    lib.iqgpu_psd_destroy(None)            # tolerated
    lib.iqgpu_psd_geometry(None)
    # cap < nfft; the sums are optional
    for n in SIZES:
        o = psd_opts(nfft=n)
        assert lib.iqgpu_psd_window(C.byref(o), wp, n - 1, None, None) == EINVAL
        assert lib.iqgpu_psd_window(C.byref(o), wp, n, None, None) == 0
    # an unknown format, with good options
    for fmt in (0, 7, 17, -1):
        assert lib.iqgpu_psd_create(0, fmt, C.byref(good), C.byref(h)) == EFORMAT and not h.value


def test_geometry_is_in_the_expected_band(lib):
    from iq_tool_amd import psd
    assert 16 <= psd.geometry() <= 64


def test_create_without_a_device_answers_enodev(lib):
    from iq_tool_amd import _lib
    from iq_tool_amd.psd import psd_opts
    if lib.iqgpu_device_count() > 0:
        pytest.skip("a device is visible")
    h = C.c_void_p()
    o = psd_opts()
    assert lib.iqgpu_psd_create(0, _lib.FMT["cs16"], C.byref(o), C.byref(h)) == ENODEV and not h.value
    with pytest.raises(_lib.IqgpuError) as e:
        import iq_tool_amd
        iq_tool_amd.Psd("cs16")
    assert e.value.code == ENODEV


def test_psd_struct_layouts_match_ctypes(tmp_path):
    from iq_tool_amd import _lib
    prog = textwrap.dedent("""
        #include <stdio.h>
        #include <stddef.h>
        #include "iqgpu.h"
        int main(void) {
            printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(iqgpu_psd_opts), offsetof(iqgpu_psd_opts, nfft),
                   offsetof(iqgpu_psd_opts, hop), offsetof(iqgpu_psd_opts, window), offsetof(iqgpu_psd_opts, gain),
                   sizeof(iqgpu_psd_info), offsetof(iqgpu_psd_info, frames), offsetof(iqgpu_psd_info, segments),
                   offsetof(iqgpu_psd_info, nfft), offsetof(iqgpu_psd_info, hop), offsetof(iqgpu_psd_info, window_sum),
                   offsetof(iqgpu_psd_info, window_sum_sq));
            return 0;
        }""")
    src = tmp_path / "layout.c"
    src.write_text(prog)
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    O, I = _lib.PsdOpts, _lib.PsdInfo
    want = [C.sizeof(O), O.nfft.offset, O.hop.offset, O.window.offset, O.gain.offset,
            C.sizeof(I), I.frames.offset, I.segments.offset, I.nfft.offset, I.hop.offset, I.window_sum.offset, I.window_sum_sq.offset]
    assert got == want
    assert (C.sizeof(O), C.sizeof(I)) == (16, 40)
