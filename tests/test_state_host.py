"""Checkpoint / resume, host side (no device): the five entry points and iqgpu_state_info as the header declares them and as ctypes
mirrors them, the blob size of a description without a device, and what iqgpu_state_inspect refuses."""
import ctypes as C
import os
import re
import subprocess
import textwrap

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ERATIO, EFORMAT = -1, -4, -5
ENTRY_POINTS = ("iqgpu_design_state_size", "iqgpu_state_inspect", "iqgpu_chain_tell", "iqgpu_chain_save_state", "iqgpu_chain_load_state")
NRSC5 = dict(in_format="cs16", out_format="cs16", input_rate_hz=2.4e6, target_rate_hz=744187.5, shift_hz=200e3)
TEN_TO_2M4 = dict(in_format="cs16", out_format="cs16", input_rate_hz=10e6, target_rate_hz=2.4e6)
FFT1025 = dict(filters=(("passband", 158.5e3, 113e3),), filter_taps=1024)              # 1025 taps, FFT kind, block 2048


@pytest.fixture(scope="module")
def lib():
    import iq_tool_amd
    return iq_tool_amd.load()


def header():
    with open(os.path.join(ROOT, "include", "iqgpu.h")) as fh:
        return fh.read()


def test_header_declares_the_entry_points_and_the_abi_version_stays(lib):
    from iq_tool_amd import _lib
    hdr = header()
    assert int(re.search(r"#define\s+IQGPU_ABI_VERSION\s+(\d+)", hdr).group(1)) == 9 == lib.iqgpu_abi_version()
    bound = {n for n, _, _ in _lib.SYMBOLS}
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (iqgpu_[a-z0-9_]+)", out))
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in exported and name in bound and getattr(lib, name) is not None
    assert re.search(r"\}\s*iqgpu_state_info\s*;", hdr)
    # ... and the one refusal of save is listed with the others
    assert re.search(r"IQGPU_EUNSUPPORTED = -10.*?iqgpu_chain_save_state: a chain on IQGPU_AGC_CLOCK_WALL", hdr, re.S)


def test_state_info_layout_matches_the_header(tmp_path):
    from iq_tool_amd import _lib
    fields = ["format_version", "reserved", "bytes", "fingerprint", "frames_in", "frames_out"]
    prog = textwrap.dedent("""
        #include <stdio.h>
        #include <stddef.h>
        #include "iqgpu.h"
        int main(void) {
            printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(iqgpu_state_info), offsetof(iqgpu_state_info, format_version),
                   offsetof(iqgpu_state_info, reserved), offsetof(iqgpu_state_info, bytes), offsetof(iqgpu_state_info, fingerprint),
                   offsetof(iqgpu_state_info, frames_in), offsetof(iqgpu_state_info, frames_out));
            return 0;
        }""")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(prog)
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    S = _lib.StateInfo
    assert got == [C.sizeof(S)] + [getattr(S, f).offset for f in fields] == [40, 0, 4, 8, 16, 24, 32]


def test_design_state_size(lib):
    import iq_tool_amd
    from iq_tool_amd.chain import make_desc
    n = iq_tool_amd.design_state_size(**NRSC5)
    assert n > 0 and n % 16 == 0
    assert iq_tool_amd.design_state_size(**NRSC5) == n                     # equal descriptions, equal sizes
    assert iq_tool_amd.design_state_size(**dict(NRSC5, device=3, iq_mag=0.01)) == n
    plain, filt = iq_tool_amd.design_state_size(**TEN_TO_2M4), iq_tool_amd.design_state_size(**dict(TEN_TO_2M4, **FFT1025))
    # the filter front at its maximum: [L-1 history][a whole block pending], cf32
    assert plain % 16 == 0 and filt == plain + (1024 + 2048) * 8
    # what every further stage adds: the r >= 1 resampler's history, the window of the dx / local AGC profiles
    assert iq_tool_amd.design_state_size(**dict(NRSC5, input_rate_hz=2.0e6, target_rate_hz=2.4e6)) > 192
    digital, local = (iq_tool_amd.design_state_size(**dict(NRSC5, agc=True, agc_profile=p)) for p in ("digital", "local"))
    assert digital == n and local > n
    # the error codes of iqgpu_design_probe
    info, got = iq_tool_amd._lib.ChainInfo(), C.c_size_t(7)
    for bad, code in ((dict(NRSC5, target_rate_hz=2.4e6 * 2000), ERATIO), (dict(NRSC5, target_rate_hz=100.0), ERATIO),
                      (dict(NRSC5, out_format=99), EFORMAT), (dict(NRSC5, in_format=3), EFORMAT)):
        d = make_desc(**bad)
        assert lib.iqgpu_design_probe(C.byref(d), C.byref(info), None, 0, None, 0, None, 0) == code
        assert lib.iqgpu_design_state_size(C.byref(d), C.byref(got)) == code and got.value == 0
        assert lib.iqgpu_last_error()
    d = make_desc(**NRSC5)
    assert lib.iqgpu_design_state_size(None, C.byref(got)) == EINVAL and lib.iqgpu_design_state_size(C.byref(d), None) == EINVAL


def test_state_inspect_refuses_what_is_no_saved_state(lib):
    import iq_tool_amd
    from iq_tool_amd import _lib
    n = iq_tool_amd.design_state_size(**NRSC5)
    info = _lib.StateInfo()
    rng = np.random.default_rng(7)
    cases = {"NULL": (None, n), "0 bytes": (b"", 0), "7 bytes": (b"IQGPUST", 7), "zero-filled": (bytes(n), n),
             "random": (rng.integers(0, 256, n, dtype=np.uint8).tobytes(), n),
             "the magic alone": (b"IQGPUST1" + bytes(n - 8), n)}
    for what, (blob, size) in cases.items():
        info.bytes = 99
        assert lib.iqgpu_state_inspect(blob, size, C.byref(info)) == EINVAL, what
        msg = lib.iqgpu_last_error().decode()
        print("%s: %s" % (what, msg))
        assert "iqgpu_state_inspect" in msg and len(msg) > 25, what
        assert info.bytes == 0, what
        if blob is not None:
            with pytest.raises(iq_tool_amd.IqgpuError) as e:
                iq_tool_amd.state_inspect(blob)
            assert e.value.code == EINVAL
    assert lib.iqgpu_state_inspect(bytes(n), n, None) == EINVAL


def test_null_chain_is_einval(lib):
    a, b, n = C.c_uint64(0), C.c_uint64(0), C.c_size_t(0)
    buf = C.create_string_buffer(64)
    assert lib.iqgpu_chain_tell(None, C.byref(a), C.byref(b)) == EINVAL
    assert lib.iqgpu_chain_save_state(None, buf, 64, C.byref(n)) == EINVAL
    assert lib.iqgpu_chain_load_state(None, buf, 64) == EINVAL
    assert b"NULL" in lib.iqgpu_last_error()


def test_the_blob_unit_includes_nothing_of_hip():
    """state_blob.cpp / .hpp compile alone: the stand-alone sanitizer program under tools/ depends on it"""
    for name in ("state_blob.cpp", "state_blob.hpp"):
        with open(os.path.join(ROOT, "iq_tool_amd", "csrc", name)) as fh:
            incs = re.findall(r'#include\s+[<"]([^>"]+)[>"]', fh.read())
        assert incs and not [i for i in incs if "hip" in i or i in ("chain.hpp", "kernels.hpp")], incs
