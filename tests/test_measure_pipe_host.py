"""The pipelined measure pass (iqgpu_chain_measure_submit, ABI v9), host side: the library exports the call, the version is the
header's, and the ctypes signature is the prototype the header declares.  No device is touched."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "iqgpu.h")
NAME = "iqgpu_chain_measure_submit"
EINVAL = -1
# a parameter of the prototype (const and the name dropped, blanks squeezed) -> what the ctypes table binds it to
CTYPE = {"iqgpu_chain *": C.c_void_p, "void *": C.c_void_p, "iqgpu_agc_chunk *": C.c_void_p, "size_t": C.c_size_t,
         "size_t *": C.POINTER(C.c_size_t), "uint64_t": C.c_uint64, "uint64_t *": C.POINTER(C.c_uint64), "int": C.c_int}


@pytest.fixture(scope="module")
def lib():
    import iq_tool_amd
    return iq_tool_amd.load()


def header_without_comments():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def prototype(name):
    """(return type, [parameter types]) of `name` as include/iqgpu.h declares it"""
    m = re.search(r"\b(\w[\w \*]*?)\s+%s\s*\(([^)]*)\)\s*;" % name, header_without_comments())
    assert m, "%s is not declared in iqgpu.h" % name
    params = []
    for p in m.group(2).split(","):
        p = re.sub(r"\bconst\b", "", p).strip()
        base, stars = re.match(r"([\w ]+?)\s*(\**)\s*\w+$", p).groups()
        params.append((" ".join(base.split()) + (" " + stars if stars else "")))
    return m.group(1).strip(), params


def test_library_exports_measure_submit(lib):
    from iq_tool_amd import _lib
    declared = set(re.findall(r"\b(iqgpu_[a-z0-9_]+)\s*\(", header_without_comments()))
    assert NAME in declared
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert NAME in set(re.findall(r" T (iqgpu_[a-z0-9_]+)", out))
    assert NAME in {n for n, _, _ in _lib.SYMBOLS} and getattr(lib, NAME) is not None


def test_abi_version_is_9_and_the_headers(lib):
    version = int(re.search(r"#define\s+IQGPU_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1))
    assert version == 9 and lib.iqgpu_abi_version() == 9


def test_ctypes_signature_is_the_headers_prototype(lib):
    from iq_tool_amd import _lib
    ret, params = prototype(NAME)
    assert ret == "int"
    assert params == ["iqgpu_chain *", "void *", "size_t", "iqgpu_agc_chunk *", "size_t", "size_t *", "uint64_t *"]
    (res, args), = [(r, a) for n, r, a in _lib.SYMBOLS if n == NAME]
    assert res is C.c_int and args == [CTYPE[p] for p in params]
    fn = getattr(lib, NAME)
    assert fn.restype is C.c_int and list(fn.argtypes) == args
    # the rows it fills are collected with the call the ordinary pipeline has: same ticket type
    (_, cargs), = [(r, a) for n, r, a in _lib.SYMBOLS if n == "iqgpu_chain_collect"]
    assert [CTYPE[p] for p in prototype("iqgpu_chain_collect")[1]] == cargs and cargs[1] is C.c_uint64


def test_null_chain_is_einval_without_a_device(lib):
    from iq_tool_amd import _lib
    rows, got, ticket = (_lib.AgcChunk * 4)(), C.c_size_t(5), C.c_uint64(5)
    buf = (C.c_char * 64)()
    assert getattr(lib, NAME)(None, buf, 16, rows, 4, C.byref(got), C.byref(ticket)) == EINVAL
    assert b"NULL" in lib.iqgpu_last_error()
