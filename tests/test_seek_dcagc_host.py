"""Exact sharding of chains with the DC blocker and the digital AGC, host side (no device): the iqgpu_chain_dcagc_* symbols are
exported, declared in the header with the argument lists the ctypes table gives them, refuse a NULL chain before they touch
anything, and the harness plans a `--shards N --seamless-dc-agc` job (--dry-placement covers the seamless modes: no GPU call)."""
import ctypes as C
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
NAMES = ("iqgpu_chain_dcagc_dc_measure", "iqgpu_chain_dcagc_dc_measure_device", "iqgpu_chain_dcagc_dc_advance", "iqgpu_chain_dcagc_seek",
         "iqgpu_chain_dcagc_seek_device", "iqgpu_chain_dcagc_measure", "iqgpu_chain_dcagc_measure_device")
# what a C parameter type is in the ctypes table: pointers to the library's structures by their class, every other pointer void *
CTYPE = {"uint64_t": C.c_uint64, "size_t": C.c_size_t}


@pytest.fixture(scope="module")
def lib():
    import iq_tool_amd
    return iq_tool_amd.load()


def declared(name):
    """(return type, [parameter types]) of `name` as include/iqgpu.h declares it"""
    hdr = open(os.path.join(ROOT, "include", "iqgpu.h")).read()
    m = re.search(r"^(\w+)\s+" + name + r"\(([^;]*?)\);", hdr, re.M | re.S)
    assert m, name
    params = [" ".join(p.split()) for p in m.group(2).split(",")]
    return m.group(1), [p.rsplit(" ", 1)[0].replace("const ", "") + ("*" if p.rsplit(" ", 1)[1].startswith("*") else "") for p in params]


@pytest.mark.parametrize("name", NAMES)
def test_symbols_are_exported_and_declared_as_the_ctypes_table_says(lib, name):
    from iq_tool_amd import _lib
    assert hasattr(lib, name)
    res, args = {n: (r, a) for n, r, a in _lib.SYMBOLS}[name]
    ret, params = declared(name)
    assert ret == "int" and res is C.c_int
    struct_ptr = {"iqgpu_dc_state*": C.POINTER(_lib.DcState), "iqgpu_agc_state*": C.POINTER(_lib.AgcState)}
    print(name, params)
    assert len(args) == len(params)
    for got, p in zip(args, params):
        if p == "size_t*":
            assert got == C.POINTER(C.c_size_t), (name, p)
        elif p in struct_ptr:
            assert got in (struct_ptr[p], C.c_void_p), (name, p)        # (one state by its class, an array of them as void *)
        elif p.endswith("*"):
            assert got is C.c_void_p, (name, p)
        else:
            assert got is CTYPE[p], (name, p)


def test_abi_version_is_unchanged(lib):
    hdr = open(os.path.join(ROOT, "include", "iqgpu.h")).read()
    assert int(re.search(r"#define\s+IQGPU_ABI_VERSION\s+(\d+)", hdr).group(1)) == 9 == lib.iqgpu_abi_version()


def test_null_chain_is_refused(lib):
    from iq_tool_amd import _lib
    buf = (C.c_uint8 * 64)()
    rows = (C.c_uint8 * 64)()
    n = C.c_size_t(7)
    st = _lib.DcState()
    assert lib.iqgpu_chain_dcagc_dc_measure(None, 0, buf, 8, rows, 2, C.byref(n)) == EINVAL
    assert lib.iqgpu_chain_dcagc_dc_measure_device(None, 0, buf, 8, rows, 2, C.byref(n)) == EINVAL
    assert lib.iqgpu_chain_dcagc_dc_advance(None, C.byref(st), rows, 1, None) == EINVAL
    assert lib.iqgpu_chain_dcagc_seek(None, 0, None, 0, 0, None, None) == EINVAL
    assert lib.iqgpu_chain_dcagc_seek_device(None, 0, None, 0, 0, None, None) == EINVAL
    assert lib.iqgpu_chain_dcagc_measure(None, buf, 8, rows, 4, C.byref(n)) == EINVAL
    assert lib.iqgpu_chain_dcagc_measure_device(None, buf, 8, rows, 4, C.byref(n)) == EINVAL
    assert b"NULL chain" in lib.iqgpu_last_error()


def test_python_methods_exist():
    from iq_tool_amd.chain import Chain
    for m in ("dcagc_dc_measure", "dcagc_dc_measure_device", "dcagc_dc_advance", "dcagc_seek", "dcagc_seek_device", "dcagc_measure",
              "dcagc_measure_device"):
        assert callable(getattr(Chain, m))


def _dry(tmp_path, total, *extra, shards=4, chunk=1 << 22):
    from iq_tool_amd.build import HARNESS_BIN
    env = dict(os.environ)
    for k in ("ROCR_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        env.pop(k, None)
    cmd = [HARNESS_BIN, "--synthetic", str(total), "--synthetic-hash", "7", "--raw-file-input-rate", "2400000", "--raw-file-input-sample-format", "cs16",
           "--output-rate", "744187.5", "--output-sample-format", "cs16", "--freq-shift", "200000", "--shards", str(shards), "--devices", "8",
           "--chunk-frames", str(chunk), "--dry-placement", "--no-numa-bind", "--debug", "sysfs_root=" + str(tmp_path), *extra]
    return subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=120)


def test_harness_dry_placement_of_a_seamless_dc_agc_job(lib, tmp_path):
    import iq_tool_amd
    kw = dict(in_format="cs16", out_format="cs16", input_rate_hz=2.4e6, target_rate_hz=744187.5, shift_hz=200e3)
    total, chunk = 4 * 100_000_000 + 12_345, 1 << 22
    p = _dry(tmp_path, total, "--seamless-dc-agc", "--dc-block", "--agc-profile", "digital")
    assert p.returncode == 0, p.stderr
    r = json.loads(p.stdout.strip().splitlines()[-1])
    assert r["dry_placement"] is True and r["seamless_dc_agc"] is True and "seamless_dc" not in r and "seamless_agc" not in r
    pre = -(-iq_tool_amd.design_preroll_frames(**kw) // chunk) * chunk             # the filters' memory in whole calls
    assert pre == chunk
    per, off, end = total // 4, 0, 0
    for s, sh in enumerate(r["per_shard"]):
        assert sh["first_frame"] == s * per // chunk * chunk == end and sh["first_frame"] % 16384 == 0
        end = sh["first_frame"] + sh["frames_in"]
        assert sh["preroll_frames"] == min(sh["first_frame"], pre)
        first, count = iq_tool_amd.design_out_frames_range(sh["first_frame"], sh["frames_in"], **kw)
        assert (sh["out_offset_bytes"], sh["planned_out"]) == (4 * first, count) and sh["out_offset_bytes"] == off
        off += 4 * sh["planned_out"]
        assert sh["dc_rows"] == (-(-sh["frames_in"] // chunk) if s < 3 else 0)
        assert sh["agc_rows"] == (-(-sh["frames_in"] // 16384) if s < 3 else 0)
    assert end == total and off // 4 == r["frames_out"]


def test_harness_refuses_what_the_recipe_does_not_cover(lib, tmp_path):
    both = ("--dc-block", "--agc-profile", "digital")
    for extra, status, word in [(("--seamless-dc-agc", "--agc-profile", "digital"), 1, "--dc-block"),
                                (("--seamless-dc-agc", "--dc-block"), 1, "AGC"),
                                (("--seamless-dc-agc", "--dc-block", "--agc-profile", "dx"), 1, "dx / local"),
                                (("--seamless-dc-agc", "--seamless-dc", *both), 2, "excludes"),
                                (("--seamless-dc-agc", "--seamless-agc", *both), 2, "excludes")]:
        p = _dry(tmp_path, 1 << 26, *extra)
        assert p.returncode == status and word in p.stderr and not p.stdout.strip(), (extra, p.returncode, p.stderr)
    p = _dry(tmp_path, 1 << 26, "--seamless-dc-agc", *both, chunk=16384 * 3 + 4096)       # calls off the AGC's chunk grid
    assert p.returncode == 2 and "multiple of the AGC chunk" in p.stderr
    p = _dry(tmp_path, 1 << 22, "--seamless-dc-agc", *both, shards=4)                      # too few frames for the grid
    assert p.returncode == 1 and "too few" in p.stderr
    # the older modes keep their refusal of such a chain, in their own words
    p = _dry(tmp_path, 1 << 26, "--seamless-dc", *both)
    assert p.returncode == 1 and "AGC" in p.stderr and not p.stdout.strip()
