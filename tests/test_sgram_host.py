"""The row accumulator, host side (include/iqgpu.h "spectrogram"; no GPU call): the defaults, the row count against its closed form
around nfft, a row boundary and a cell boundary, every refusal that needs no device, the answer of create where no device is visible,
and the layout of the two structs against the ctypes mirror."""
import ctypes as C
import os
import subprocess
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENODEV, EFORMAT = -1, -2, -5


@pytest.fixture(scope="module")
def lib():
    import iq_tool_amd
    return iq_tool_amd.load()


def test_opts_init_sets_the_documented_defaults(lib):
    from iq_tool_amd import _lib
    o = _lib.SgramOpts(7, 7, 7, 7.0, 7)
    lib.iqgpu_sgram_opts_init(C.byref(o))
    assert (o.nfft, o.hop, o.window, o.gain, o.row_segments) == (1024, 512, _lib.PSD_WINDOW["hann"], 1.0, 32)
    lib.iqgpu_sgram_opts_init(None)        # tolerated


def closed_form(frames, n, hop, R):
    return (0 if frames < n else (frames - n) // hop + 1) // R


@pytest.mark.parametrize("n", (1024, 2048, 4096))
def test_rows_equal_the_closed_form(lib, n):
    from iq_tool_amd import psd, sgram
    G = psd.geometry()
    for hop in (n, n // 2, n // 4):
        for R in (1, 3, G, G + 1, 70, 1 << 20):
            row_end = n + (R - 1) * hop                      # the frame count that finishes row 0
            cell_end = n + (G - 1) * hop                     # ... the first cell
            sweep = {0, 1, 5 * n + 3, 70_000, (1 << 31) + 5, 1 << 39}
            for centre in (n, row_end, cell_end, row_end + R * hop, row_end + 2 * R * hop):
                sweep |= {centre - 1, centre, centre + 1, centre + hop - 1, centre + hop}
            for frames in sorted(sweep):
                assert sgram.rows(frames, n, hop, R) == closed_form(frames, n, hop, R), (n, hop, R, frames)
            assert sgram.rows(row_end - 1, n, hop, R) == 0 and sgram.rows(row_end, n, hop, R) == 1


def test_refusals_that_need_no_device(lib):
    from iq_tool_amd import _lib
    from iq_tool_amd.sgram import sgram_opts
    n64, h = C.c_uint64(0), C.c_void_p()
    bad = [sgram_opts(row_segments=0), sgram_opts(row_segments=(1 << 20) + 1), sgram_opts(row_segments=0xffffffff),
           sgram_opts(nfft=512, hop=256), sgram_opts(nfft=8192, hop=4096), sgram_opts(nfft=1000, hop=500), sgram_opts(nfft=1024, hop=128),
           sgram_opts(nfft=1024, hop=0), sgram_opts(nfft=1024, hop=2048), sgram_opts(nfft=2048, hop=768), sgram_opts(window=4), sgram_opts(window=-1),
           sgram_opts(gain=float("nan")), sgram_opts(gain=float("inf")), sgram_opts(gain=float("-inf"))]
    for o in bad:
        assert lib.iqgpu_sgram_rows(C.byref(o), 1 << 20, C.byref(n64)) == EINVAL
        assert lib.iqgpu_sgram_create(0, _lib.FMT["cs16"], C.byref(o), C.byref(h)) == EINVAL and not h.value
        assert lib.iqgpu_last_error()
    for R in (1, 1 << 20):
        assert lib.iqgpu_sgram_rows(C.byref(sgram_opts(row_segments=R)), 1 << 20, C.byref(n64)) == 0
    good = sgram_opts()
    x = (C.c_float * 16)()
    got = C.c_size_t(5)
    # NULL arguments
    assert lib.iqgpu_sgram_rows(None, 4096, C.byref(n64)) == EINVAL
    assert lib.iqgpu_sgram_rows(C.byref(good), 4096, None) == EINVAL
    assert lib.iqgpu_sgram_create(0, _lib.FMT["cs16"], None, C.byref(h)) == EINVAL
    assert lib.iqgpu_sgram_create(0, _lib.FMT["cs16"], C.byref(good), None) == EINVAL
    assert lib.iqgpu_sgram_reset(None) == EINVAL
    assert lib.iqgpu_sgram_push(None, x, 16, None, None, 0, C.byref(got)) == EINVAL and got.value == 0
    got.value = 5
    assert lib.iqgpu_sgram_push_device(None, x, 16, None, None, 0, C.byref(got), None) == EINVAL and got.value == 0
    assert lib.iqgpu_sgram_read_open(None, None, None, None) == EINVAL
    assert lib.iqgpu_sgram_max_rows(None, 1 << 20) == 0
    lib.iqgpu_sgram_destroy(None)          # tolerated
    # an unknown format, with good options
    for fmt in (0, 7, 17, -1):
        assert lib.iqgpu_sgram_create(0, fmt, C.byref(good), C.byref(h)) == EFORMAT and not h.value


def test_create_without_a_device_answers_enodev(lib):
    from iq_tool_amd import _lib
    from iq_tool_amd.sgram import sgram_opts
    if lib.iqgpu_device_count() > 0:
        pytest.skip("a device is visible")
    h = C.c_void_p()
    o = sgram_opts()
    assert lib.iqgpu_sgram_create(0, _lib.FMT["cs16"], C.byref(o), C.byref(h)) == ENODEV and not h.value
    with pytest.raises(_lib.IqgpuError) as e:
        import iq_tool_amd
        iq_tool_amd.Sgram("cs16")
    assert e.value.code == ENODEV


def test_sgram_struct_layouts_match_ctypes(tmp_path):
    from iq_tool_amd import _lib
    ofields = [n for n, _ in _lib.SgramOpts._fields_]
    ifields = [n for n, _ in _lib.SgramInfo._fields_]
    assert ofields == ["nfft", "hop", "window", "gain", "row_segments"]
    assert ifields == ["frames", "segments", "rows", "open_segments", "nfft", "hop", "row_segments", "window_sum", "window_sum_sq"]
    lines = ['printf("%zu %zu ", sizeof(iqgpu_sgram_opts), sizeof(iqgpu_sgram_info));']
    lines += ['printf("%%zu ", offsetof(iqgpu_sgram_opts, %s));' % n for n in ofields]
    lines += ['printf("%%zu ", offsetof(iqgpu_sgram_info, %s));' % n for n in ifields]
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
    O, I = _lib.SgramOpts, _lib.SgramInfo
    want = [C.sizeof(O), C.sizeof(I)] + [getattr(O, n).offset for n in ofields] + [getattr(I, n).offset for n in ifields]
    assert got == want
    assert (C.sizeof(O), C.sizeof(I)) == (20, 56)
