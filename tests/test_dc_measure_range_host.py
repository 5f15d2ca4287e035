"""The DC measure pass over a whole range in one call (include/iqgpu.h, iqgpu_chain_*_dc_measure_range), host side (no device): the
header, the exports, the ctypes table, the Python methods, the refusals that need no chain, the launch cap's accessor and the
diagnostic switch that sizes the host variants' staging slice.

Not covered here: the per-piece planning (dc_measure_plan, process.cpp).  It plans on a chain object, and a chain exists only behind
iqgpu_chain_create, which needs a device; tests/test_gpu_dc_measure_range.py compares its outcome -- the rows -- with the per-call
form's on the GPU, where both forms plan through it."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
NAMES = ("iqgpu_chain_dc_measure_range", "iqgpu_chain_dc_measure_range_device",
         "iqgpu_chain_dcagc_dc_measure_range", "iqgpu_chain_dcagc_dc_measure_range_device",
         "iqgpu_chain_dcrms_dc_measure_range", "iqgpu_chain_dcrms_dc_measure_range_device")
CAP = "iqgpu_dc_measure_range_launch_entries"


@pytest.fixture(scope="module")
def lib():
    import iq_tool_amd
    return iq_tool_amd.load()


def header():
    return open(os.path.join(ROOT, "include", "iqgpu.h")).read()


def declared(name):
    """(return type, [parameter types]) of `name` as include/iqgpu.h declares it"""
    m = re.search(r"^(\w+)\s+" + name + r"\(([^;]*?)\);", header(), re.M | re.S)
    assert m, name
    params = [" ".join(p.split()) for p in m.group(2).split(",")]
    return m.group(1), [p.rsplit(" ", 1)[0].replace("const ", "") + ("*" if p.rsplit(" ", 1)[1].startswith("*") else "") for p in params]


@pytest.mark.parametrize("name", NAMES)
def test_the_header_declares_the_call_as_the_ctypes_table_binds_it(lib, name):
    from iq_tool_amd import _lib
    res, args = {n: (r, a) for n, r, a in _lib.SYMBOLS}[name]
    ret, params = declared(name)
    print(name, params)
    assert params == ["iqgpu_chain*", "uint64_t", "void*", "size_t", "size_t", "iqgpu_dc_row*", "size_t", "size_t*", "uint32_t*"]
    assert ret == "int" and res is C.c_int and len(args) == len(params)
    by_type = {"uint64_t": (C.c_uint64,), "size_t": (C.c_size_t,), "size_t*": (C.POINTER(C.c_size_t),), "iqgpu_chain*": (C.c_void_p,),
               "void*": (C.c_void_p,), "iqgpu_dc_row*": (C.POINTER(_lib.DcRow), C.c_void_p), "uint32_t*": (C.POINTER(C.c_uint32), C.c_void_p)}
    for got, p in zip(args, params):
        assert got in by_type[p], (name, p)


def test_the_abi_version_is_still_9_and_the_library_exports_the_calls(lib):
    from iq_tool_amd import _lib
    assert int(re.search(r"#define\s+IQGPU_ABI_VERSION\s+(\d+)", header()).group(1)) == 9 == lib.iqgpu_abi_version()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (iqgpu_[a-z0-9_]+)", out))
    assert set(NAMES) <= exported and CAP in exported
    for name in NAMES:
        assert getattr(lib, name) is not None


def test_the_python_methods_exist():
    from iq_tool_amd.chain import Chain
    for m in ("dc_measure_range", "dc_measure_range_device", "dcagc_dc_measure_range", "dcagc_dc_measure_range_device",
              "dcrms_dc_measure_range", "dcrms_dc_measure_range_device"):
        assert callable(getattr(Chain, m)), m


@pytest.mark.parametrize("name", NAMES)
def test_a_null_chain_is_refused_whatever_else_is_null(lib, name):
    from iq_tool_amd import _lib
    fn = getattr(lib, name)
    buf, rows, got, first = (C.c_uint8 * 64)(), (_lib.DcRow * 4)(), C.c_size_t(7), (C.c_uint32 * 4)()
    assert fn(None, 0, buf, 8, 4096, rows, 4, C.byref(got), first) == EINVAL
    msg = lib.iqgpu_last_error()
    # under the new entry point's name (the _device form speaks as its host form, like every family call)
    assert b"NULL chain" in msg and msg.startswith(name.replace("_device", "").encode() + b":")
    assert fn(None, 0, buf, 8, 4096, None, 0, C.byref(got), None) == EINVAL
    assert fn(None, 0, None, 0, 0, None, 0, None, None) == EINVAL


def test_the_launch_cap_has_one_statement_and_an_accessor(lib):
    """the tests take the cap from the accessor; the accessor returns the constant the kernels' launchers check"""
    src = open(os.path.join(ROOT, "iq_tool_amd", "csrc", "kernels.hpp")).read()
    stated = re.findall(r"constexpr\s+int\s+kDcBatchEntries\s*=\s*(\d+)\s*;", src)
    assert len(stated) == 1
    cap = lib.iqgpu_dc_measure_range_launch_entries()
    print("entries per launch:", cap)
    assert cap == int(stated[0]) and 1 <= cap <= 65535                   # (grid.y of k_dc_prefix_batch)


def test_the_slice_switch_is_known_to_the_library_and_to_the_mirror(lib):
    from iq_tool_amd import _lib
    assert "dc_range_slice_frames" in _lib.DEBUG_NAMES
    try:
        assert lib.iqgpu_debug_set(b"dc_range_slice_frames", b"262144") == 0
        assert _lib.debug_switches().get("dc_range_slice_frames") == "262144"
    finally:
        assert lib.iqgpu_debug_set(b"dc_range_slice_frames", None) == 0
    assert "dc_range_slice_frames" not in _lib.debug_switches()
