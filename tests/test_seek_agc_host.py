"""Seamless range sharding of digital-AGC chains, host side (no device): the harness's `--shards N --seamless-agc` plan, the
refusals that need no GPU, and the v8 entry points of the C ABI."""
import ctypes as C
import json
import math
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "iq_tool_amd", "lib", "iqgpu_run")
EINVAL = -1
NRSC5_ARGS = ["--raw-file-input-rate", "2.4e6", "--raw-file-input-sample-format", "cs16", "--output-rate", "744187.5",
              "--output-sample-format", "cs16", "--freq-shift", "200e3"]
CU8_ARGS = ["--raw-file-input-rate", "2.4e6", "--raw-file-input-sample-format", "cu8", "--output-rate", "1488375",
            "--output-sample-format", "cu8"]
V8 = ("iqgpu_chain_measure", "iqgpu_chain_measure_device", "iqgpu_chain_agc_advance", "iqgpu_chain_agc_initial_state",
      "iqgpu_chain_seek_agc", "iqgpu_chain_seek_agc_device")


@pytest.fixture(scope="module")
def lib():
    import iq_tool_amd
    return iq_tool_amd.load()


def harness(*args):
    return subprocess.run([EXE, *args], capture_output=True, text=True)


@pytest.mark.parametrize("args,fmt", [(NRSC5_ARGS, "cs16"), (CU8_ARGS, "cu8")])
@pytest.mark.parametrize("shards,n,chunk,agc_chunk", [(4, 1 << 28, 1 << 22, 16384), (3, 100_000_003, 3 * 16384, 16384), (5, 77_777_777, 81920, 16384)])
def test_dry_placement_plans_the_two_pass_job(lib, args, fmt, shards, n, chunk, agc_chunk):
    import iq_tool_amd
    r = harness("--synthetic", str(n), "--synthetic-hash", "5", *args, "--agc-profile", "digital", "--shards", str(shards), "--seamless-agc", "--chunk-frames", str(chunk),
                "--dry-placement", "--no-numa-bind")
    assert r.returncode == 0, r.stderr
    info = json.loads(r.stdout.strip().splitlines()[-1])
    assert info["dry_placement"] is True and info["seamless_agc"] is True and "seamless" not in info
    grid = math.lcm(4096, agc_chunk, chunk)
    kw = dict(in_format=fmt, out_format=fmt, input_rate_hz=2.4e6, target_rate_hz=744187.5 if fmt == "cs16" else 1488375.0,
              shift_hz=200e3 if fmt == "cs16" else 0.0)
    want_pre = iq_tool_amd.design_preroll_frames(**kw)             # placement comes from the description WITHOUT the AGC
    at = out_at = 0
    for s, ps in enumerate(info["per_shard"]):
        assert ps["shard"] == s and ps["first_frame"] == at and ps["first_frame"] % grid == 0
        assert ps["first_frame"] == (s * (n // shards)) // grid * grid
        assert ps["preroll_frames"] == min(ps["first_frame"], want_pre)
        # one row per AGC chunk of the range; the last shard measures nothing (nobody starts behind it)
        assert ps["agc_rows"] == (-(-ps["frames_in"] // agc_chunk) if s < shards - 1 else 0)
        first, count = iq_tool_amd.design_out_frames_range(ps["first_frame"], ps["frames_in"], **kw)
        assert ps["planned_out"] == count and ps["out_offset_bytes"] == first * (4 if fmt == "cs16" else 2) == out_at
        at += ps["frames_in"]; out_at += count * (4 if fmt == "cs16" else 2)
    assert at == n and len(info["per_shard"]) == shards                     # the ranges tile the stream
    assert info["frames_out"] == iq_tool_amd.design_out_frames(n, **kw)


def test_harness_refusals_without_a_device(lib):
    base = ["--synthetic", "1000000", "--synthetic-hash", "1", *NRSC5_ARGS, "--shards", "2", "--dry-placement"]
    # --seamless with an AGC option keeps failing as it did (pinned by test_seek_host.py; seen again from here)
    r = harness(*base, "--seamless", "--agc-profile", "digital")
    assert r.returncode != 0 and "AGC" in r.stderr
    for profile in ("dx", "local"):
        r = harness(*base, "--seamless-agc", "--agc-profile", profile)
        assert r.returncode != 0 and "dx / local" in r.stderr and "digital" in r.stderr
    r = harness(*base, "--seamless-agc")
    assert r.returncode != 0 and "no output AGC" in r.stderr
    r = harness(*base, "--seamless-agc", "--seamless", "--agc-profile", "digital")
    assert r.returncode != 0
    # the two passes must read one stream: the constant filling of a bare --synthetic is none
    r = harness("--synthetic", "100000000", *NRSC5_ARGS, "--shards", "2", "--dry-placement", "--seamless-agc", "--agc-profile", "digital")
    assert r.returncode != 0 and "--synthetic-hash" in r.stderr
    # a capture too small for its shards on the cut grid (2^22 frames by default): refused, not planned with empty shards
    r = harness(*base, "--seamless-agc", "--agc-profile", "digital")
    assert r.returncode != 0 and "too few" in r.stderr
    r = harness("--synthetic", "1000000", "--synthetic-hash", "1", *NRSC5_ARGS, "--shards", "2", "--dry-placement", "--seamless-agc", "--agc-profile",
                "digital", "--chunk-frames", "65536")
    assert r.returncode == 0, r.stderr


def test_abi_v8_entry_points(lib):
    from iq_tool_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "iqgpu.h")).read()
    version = int(re.search(r"#define\s+IQGPU_ABI_VERSION\s+(\d+)", hdr).group(1))
    assert version >= 8 and lib.iqgpu_abi_version() == version
    bound = {n for n, _, _ in _lib.SYMBOLS}
    for name in V8:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in bound and getattr(lib, name) is not None
    # the row of the table, as the header lays it out and as ctypes / numpy mirror it
    from iq_tool_amd.chain import AGC_ROW
    assert C.sizeof(_lib.AgcChunk) == 16 == AGC_ROW.itemsize
    assert _lib.AgcChunk.frames_out.offset == 8 == AGC_ROW.fields["frames_out"][1]


def test_null_arguments_are_einval_without_a_device(lib):
    from iq_tool_amd import _lib
    st, rows, got = _lib.AgcState(), (_lib.AgcChunk * 4)(), C.c_size_t(5)
    buf = (C.c_char * 64)()
    assert lib.iqgpu_chain_measure(None, buf, 16, rows, 4, C.byref(got)) == EINVAL
    assert lib.iqgpu_chain_measure_device(None, buf, 16, rows, 4, C.byref(got)) == EINVAL
    assert lib.iqgpu_chain_agc_advance(None, C.byref(st), rows, 4, None) == EINVAL
    assert lib.iqgpu_chain_agc_initial_state(None, C.byref(st)) == EINVAL
    assert lib.iqgpu_chain_seek_agc(None, 0, None, 0, None) == EINVAL
    assert lib.iqgpu_chain_seek_agc_device(None, 4096, buf, 16, C.byref(st)) == EINVAL
    assert b"NULL" in lib.iqgpu_last_error()
    # no device, no chain: creating an AGC chain fails with ENODEV here and there is nothing to measure with
    if lib.iqgpu_device_count() == 0:
        from iq_tool_amd.chain import make_desc
        h = C.c_void_p()
        d = make_desc(agc=True)
        assert lib.iqgpu_chain_create(C.byref(d), C.byref(h)) == -2
