"""Exact seamless range sharding of DC-blocker chains, host side (no device): the six entry points of the C ABI as the header
declares them and as ctypes / numpy mirror them, the refusals that need no GPU, and the harness's `--shards N --seamless-dc` plan."""
import ctypes as C
import json
import math
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "iq_tool_amd", "lib", "iqgpu_run")
EINVAL, ENODEV = -1, -2
NRSC5_ARGS = ["--raw-file-input-rate", "2.4e6", "--raw-file-input-sample-format", "cs16", "--output-rate", "744187.5",
              "--output-sample-format", "cs16", "--freq-shift", "200e3"]
CONFIG3_ARGS = ["--raw-file-input-rate", "10e6", "--raw-file-input-sample-format", "cs16", "--output-rate", "2.4e6",
                "--output-sample-format", "cs16", "--pass-range", "102000:215000", "--filter-taps", "1024"]
ENTRY_POINTS = ("iqgpu_chain_get_dc_state", "iqgpu_chain_dc_measure", "iqgpu_chain_dc_measure_device", "iqgpu_chain_dc_advance",
                "iqgpu_chain_seek_dc", "iqgpu_chain_seek_dc_device")


@pytest.fixture(scope="module")
def lib():
    import iq_tool_amd
    return iq_tool_amd.load()


def harness(*args):
    return subprocess.run([EXE, *args], capture_output=True, text=True)


def header():
    with open(os.path.join(ROOT, "include", "iqgpu.h")) as fh:
        return fh.read()


def test_header_declares_the_entry_points_and_the_abi_version_stays(lib):
    from iq_tool_amd import _lib
    hdr = header()
    assert int(re.search(r"#define\s+IQGPU_ABI_VERSION\s+(\d+)", hdr).group(1)) == 9 == lib.iqgpu_abi_version()
    bound = {n for n, _, _ in _lib.SYMBOLS}
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(\s*iqgpu_chain\s*\*" % name, hdr), name
        assert name in bound and getattr(lib, name) is not None          # exported by the library, bound by the mirror


def test_struct_layouts_match_the_header(lib):
    from iq_tool_amd import _lib
    from iq_tool_amd.chain import DC_ROW, DC_STATE
    hdr = header()
    # the header's own field lists, in order: every field is 8 bytes wide, so its offset is 8 times its place
    m = re.search(r"typedef\s+struct\s*\{\s*double\s+([\w\s,]+);\s*\}\s*iqgpu_dc_state\s*;", hdr)
    assert m and [f.strip() for f in m.group(1).split(",")] == ["re", "im"]
    m = re.search(r"typedef\s+struct\s*\{\s*double\s+([\w\s,]+);\s*uint64_t\s+(\w+)\s*;\s*\}\s*iqgpu_dc_row\s*;", hdr)
    assert m and [f.strip() for f in m.group(1).split(",")] + [m.group(2)] == ["f", "g_re", "g_im", "frames"]
    assert C.sizeof(_lib.DcState) == 16 == DC_STATE.itemsize and C.sizeof(_lib.DcRow) == 32 == DC_ROW.itemsize
    for i, name in enumerate(["re", "im"]):
        assert getattr(_lib.DcState, name).offset == 8 * i == DC_STATE.fields[name][1]
    for i, name in enumerate(["f", "g_re", "g_im", "frames"]):
        assert getattr(_lib.DcRow, name).offset == 8 * i == DC_ROW.fields[name][1]
        assert getattr(_lib.DcRow, name).size == 8


def test_null_arguments_are_einval_and_no_device_is_enodev(lib):
    """What "IQGPU_ENODEV without a device" amounts to: every compute call takes a chain, and no chain can exist without a device --
    iqgpu_chain_create is where ENODEV is reported, so that is the call checked here; the compute calls themselves can only be
    reached with a NULL chain, which is IQGPU_EINVAL."""
    from iq_tool_amd import _lib
    st, row, rows = _lib.DcState(), _lib.DcRow(), (_lib.DcRow * 2)()
    buf = (C.c_char * 64)()
    assert lib.iqgpu_chain_get_dc_state(None, C.byref(st)) == EINVAL
    assert lib.iqgpu_chain_dc_measure(None, 0, buf, 8, C.byref(row)) == EINVAL
    assert lib.iqgpu_chain_dc_measure_device(None, 4096, buf, 8, C.byref(row)) == EINVAL
    assert lib.iqgpu_chain_dc_advance(None, C.byref(st), rows, 2, None) == EINVAL
    assert lib.iqgpu_chain_seek_dc(None, 0, None, 0, 0, None) == EINVAL
    assert lib.iqgpu_chain_seek_dc_device(None, 4096, buf, 8, 8, C.byref(st)) == EINVAL
    assert b"NULL" in lib.iqgpu_last_error()
    # no device, no chain: creating a DC-blocker chain fails with ENODEV here and there is nothing to measure, walk or seek with
    if lib.iqgpu_device_count() == 0:
        from iq_tool_amd.chain import make_desc
        h = C.c_void_p()
        d = make_desc(dc_block=True)
        assert lib.iqgpu_chain_create(C.byref(d), C.byref(h)) == ENODEV and not h.value


@pytest.mark.parametrize("args,kw", [
    (NRSC5_ARGS, dict(in_format="cs16", out_format="cs16", input_rate_hz=2.4e6, target_rate_hz=744187.5, shift_hz=200e3)),
    (CONFIG3_ARGS, dict(in_format="cs16", out_format="cs16", input_rate_hz=10e6, target_rate_hz=2.4e6,
                        filters=(("passband", 158.5e3, 113e3),), filter_taps=1024))])
@pytest.mark.parametrize("shards,n,chunk", [(4, 1 << 28, 1 << 22), (4, 2_000_003, 131072), (3, 100_000_003, 3 * 16384), (5, 7_777_777, 8192)])
def test_dry_placement_plans_the_three_pass_job(lib, args, kw, shards, n, chunk):
    import iq_tool_amd
    r = harness("--synthetic", str(n), "--synthetic-hash", "5", *args, "--dc-block", "--shards", str(shards), "--seamless-dc",
                "--chunk-frames", str(chunk), "--dry-placement", "--no-numa-bind")
    assert r.returncode == 0, r.stderr
    info = json.loads(r.stdout.strip().splitlines()[-1])
    assert info["dry_placement"] is True and info["seamless_dc"] is True and "seamless" not in info and "seamless_agc" not in info
    grid = math.lcm(4096, chunk)
    p_fir = iq_tool_amd.design_preroll_frames(**kw)                # the description with the blocker OFF: the filters' memory alone
    p_old = iq_tool_amd.design_preroll_frames(dc_block=True, **kw)
    want_pre = -(-p_fir // chunk) * chunk                          # ... in whole calls
    assert p_fir > 0 and want_pre - p_fir < chunk and p_old > 50 * p_fir
    kw_dc = dict(kw, dc_block=True)
    at = out_at = 0
    for s, ps in enumerate(info["per_shard"]):
        assert ps["shard"] == s and ps["first_frame"] == at and ps["first_frame"] % grid == 0
        assert ps["first_frame"] == (s * (n // shards)) // grid * grid
        assert ps["preroll_frames"] == min(ps["first_frame"], want_pre) and ps["preroll_frames"] % chunk == 0
        # one row per call of the range; the last shard measures nothing (nobody starts behind it)
        assert ps["dc_rows"] == (-(-ps["frames_in"] // chunk) if s < shards - 1 else 0)
        first, count = iq_tool_amd.design_out_frames_range(ps["first_frame"], ps["frames_in"], **kw_dc)
        assert ps["planned_out"] == count and ps["out_offset_bytes"] == 4 * first == out_at
        at += ps["frames_in"]; out_at += 4 * count
    assert at == n and len(info["per_shard"]) == shards
    assert info["frames_out"] == iq_tool_amd.design_out_frames(n, **kw_dc)


def test_harness_refusals_without_a_device(lib):
    base = ["--synthetic", "2000003", "--synthetic-hash", "1", *NRSC5_ARGS, "--shards", "2", "--dry-placement", "--chunk-frames", "131072"]
    assert harness(*base, "--seamless-dc", "--dc-block").returncode == 0
    r = harness(*base, "--seamless-dc")
    assert r.returncode != 0 and "--dc-block" in r.stderr and not r.stdout.strip()
    for agc in (["--agc-profile", "digital"], ["--agc-profile", "dx"], ["--output-agc"]):
        r = harness(*base, "--seamless-dc", "--dc-block", *agc)
        assert r.returncode != 0 and "AGC" in r.stderr and not r.stdout.strip()
    for other in ("--seamless", "--seamless-agc"):
        r = harness(*base, "--seamless-dc", "--dc-block", other)
        assert r.returncode != 0 and "exclude" in r.stderr and not r.stdout.strip()
    # it is an option of a sharded job
    r = harness("--synthetic", "2000003", "--synthetic-hash", "1", *NRSC5_ARGS, "--dry-placement", "--chunk-frames", "131072", "--seamless-dc", "--dc-block")
    assert r.returncode != 0 and "--shards" in r.stderr
    # the passes must read one stream: the constant filling of a bare --synthetic is none
    r = harness("--synthetic", "2000003", *NRSC5_ARGS, "--shards", "2", "--dry-placement", "--chunk-frames", "131072", "--seamless-dc", "--dc-block")
    assert r.returncode != 0 and "--synthetic-hash" in r.stderr
    # a capture too small for its shards on the cut grid (2^22 frames by default): refused, not planned with empty shards
    r = harness("--synthetic", "2000003", "--synthetic-hash", "1", *NRSC5_ARGS, "--shards", "2", "--dry-placement", "--seamless-dc", "--dc-block")
    assert r.returncode != 0 and "too few" in r.stderr


def test_seamless_with_the_blocker_keeps_its_bounded_plan(lib):
    """--seamless --dc-block is unchanged: its preroll still holds the blocker's warm-up"""
    import iq_tool_amd
    kw = dict(in_format="cs16", out_format="cs16", input_rate_hz=2.4e6, target_rate_hz=744187.5, shift_hz=200e3, dc_block=True)
    r = harness("--synthetic", str(1 << 26), "--synthetic-hash", "1", *NRSC5_ARGS, "--dc-block", "--shards", "2", "--seamless", "--dry-placement",
                "--no-numa-bind")
    assert r.returncode == 0, r.stderr
    info = json.loads(r.stdout.strip().splitlines()[-1])
    assert info["seamless"] is True and info["per_shard"][1]["preroll_frames"] == iq_tool_amd.design_preroll_frames(**kw)
