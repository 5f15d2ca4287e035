"""Exact seamless sharding of chains with the DC blocker and the dx / local output AGC, host side (no device): the preroll
iqgpu_design_preroll_frames_dcrms reports and its refusals, the refusals of the older calls that stay as they are, the header and the
ctypes table, and the harness's `--shards N --seamless-dc-rms` plan and refusals (--dry-placement: no GPU call).

The yardstick of the preroll is the existing call: iqgpu_design_preroll_frames_rms of the same description without the blocker."""
import ctypes as C
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -10
NAMES = ("iqgpu_design_preroll_frames_dcrms", "iqgpu_chain_dcrms_dc_measure", "iqgpu_chain_dcrms_dc_measure_device",
         "iqgpu_chain_dcrms_dc_advance", "iqgpu_chain_dcrms_seek", "iqgpu_chain_dcrms_seek_device")
RATE = 2.4e6
POINTWISE = dict(in_format="cs16", out_format="cs16", input_rate_hz=RATE, target_rate_hz=RATE, no_resample=True)
NRSC5 = dict(in_format="cs16", out_format="cs16", input_rate_hz=RATE, target_rate_hz=744187.5, shift_hz=200e3)
UP = dict(in_format="cs16", out_format="cs16", input_rate_hz=RATE, target_rate_hz=RATE * 1.2, shift_hz=150e3)


@pytest.fixture(scope="module")
def lib():
    import iq_tool_amd
    return iq_tool_amd.load()


@pytest.mark.parametrize("name,kw", [("pointwise", POINTWISE), ("nrsc5_decimation", NRSC5), ("upsampling_1.2", UP)])
@pytest.mark.parametrize("profile", ["local", "dx"])
def test_preroll_is_that_of_the_description_without_the_blocker(lib, name, kw, profile):
    import iq_tool_amd as g
    both = dict(kw, dc_block=True, agc=True, agc_profile=profile)
    got = g.design_preroll_frames_dcrms(**both)
    want = g.design_preroll_frames_rms(**dict(both, dc_block=False))
    print("%s %s: P %d, design_preroll_frames_rms without the blocker %d" % (name, profile, got, want))
    assert got == want > 0
    assert g.design_preroll_frames_dcrms(g.make_desc(**both)) == got                  # both spellings of the Python call


def test_refusals_of_the_new_design_call_and_of_the_old_one(lib):
    import iq_tool_amd as g
    both = dict(NRSC5, dc_block=True, agc=True, agc_profile="local")
    n = C.c_uint64(7)
    assert lib.iqgpu_design_preroll_frames_dcrms(None, C.byref(n)) == EINVAL
    d = g.make_desc(**both)
    assert lib.iqgpu_design_preroll_frames_dcrms(C.byref(d), None) == EINVAL and b"NULL" in lib.iqgpu_last_error()
    for over, code, word in ((dict(dc_block=False), EINVAL, "DC blocker"), (dict(agc=False), EINVAL, "AGC"),
                             (dict(agc_profile="digital"), EUNSUPPORTED, "digital")):
        with pytest.raises(g.IqgpuError) as e:
            g.design_preroll_frames_dcrms(**dict(both, **over))
        print(e.value)
        assert e.value.code == code and word in str(e.value)
        d = g.make_desc(**dict(both, **over))
        n = C.c_uint64(7)
        assert lib.iqgpu_design_preroll_frames_dcrms(C.byref(d), C.byref(n)) == code and n.value == 0
    # a description create refuses: design_probe's own code
    for over in (dict(target_rate_hz=RATE * 1e-4), dict(in_format=7), dict(agc_profile=9)):
        d = g.make_desc(**dict(both, **over))
        info = g.chain.ChainInfo()
        want = lib.iqgpu_design_probe(C.byref(d), C.byref(info), None, 0, None, 0, None, 0)
        n = C.c_uint64(7)
        got = lib.iqgpu_design_preroll_frames_dcrms(C.byref(d), C.byref(n))
        assert want < 0 and got == want and n.value == 0, over
    # the existing refusal still holds, in its old words
    with pytest.raises(g.IqgpuError) as e:
        g.design_preroll_frames_rms(**both)
    assert e.value.code == EUNSUPPORTED and "DC blocker" in str(e.value)


def declared(name):
    """(return type, [parameter types]) of `name` as include/iqgpu.h declares it"""
    hdr = open(os.path.join(ROOT, "include", "iqgpu.h")).read()
    m = re.search(r"^(\w+)\s+" + name + r"\(([^;]*?)\);", hdr, re.M | re.S)
    assert m, name
    params = [" ".join(p.split()) for p in m.group(2).split(",")]
    return m.group(1), [p.rsplit(" ", 1)[0].replace("const ", "") + ("*" if p.rsplit(" ", 1)[1].startswith("*") else "") for p in params]


@pytest.mark.parametrize("name", NAMES)
def test_the_header_names_the_new_calls_as_the_ctypes_table_binds_them(lib, name):
    from iq_tool_amd import _lib
    assert hasattr(lib, name)
    res, args = {n: (r, a) for n, r, a in _lib.SYMBOLS}[name]
    ret, params = declared(name)
    print(name, params)
    assert ret == "int" and res is C.c_int and len(args) == len(params)
    by_type = {"uint64_t": C.c_uint64, "size_t": C.c_size_t, "uint64_t*": C.POINTER(C.c_uint64),
               "iqgpu_chain_desc*": C.POINTER(_lib.ChainDesc), "iqgpu_dc_row*": (C.POINTER(_lib.DcRow), C.c_void_p),
               "iqgpu_dc_state*": (C.POINTER(_lib.DcState), C.c_void_p), "iqgpu_chain*": C.c_void_p, "void*": C.c_void_p}
    for got, p in zip(args, params):
        want = by_type[p]
        assert got in want if isinstance(want, tuple) else got == want, (name, p)


def test_abi_version_null_chains_and_python_methods(lib):
    from iq_tool_amd import _lib
    from iq_tool_amd.chain import Chain
    hdr = open(os.path.join(ROOT, "include", "iqgpu.h")).read()
    assert int(re.search(r"#define\s+IQGPU_ABI_VERSION\s+(\d+)", hdr).group(1)) == 9 == lib.iqgpu_abi_version()
    buf, row, st = (C.c_uint8 * 64)(), _lib.DcRow(), _lib.DcState()
    assert lib.iqgpu_chain_dcrms_dc_measure(None, 0, buf, 8, C.byref(row)) == EINVAL
    assert lib.iqgpu_chain_dcrms_dc_measure_device(None, 0, buf, 8, C.byref(row)) == EINVAL
    assert lib.iqgpu_chain_dcrms_dc_advance(None, C.byref(st), buf, 1, None) == EINVAL
    assert lib.iqgpu_chain_dcrms_seek(None, 0, None, 0, 0, None) == EINVAL
    assert lib.iqgpu_chain_dcrms_seek_device(None, 4096, buf, 16, 0, None) == EINVAL
    assert b"NULL chain" in lib.iqgpu_last_error()
    for m in ("dcrms_dc_measure", "dcrms_dc_measure_device", "dcrms_dc_advance", "dcrms_seek", "dcrms_seek_device"):
        assert callable(getattr(Chain, m))


def _dry(tmp_path, total, *extra, shards=3, chunk=65536):
    from iq_tool_amd.build import HARNESS_BIN
    env = dict(os.environ)
    for k in ("ROCR_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        env.pop(k, None)
    cmd = [HARNESS_BIN, "--synthetic", str(total), "--synthetic-hash", "7", "--raw-file-input-rate", "2400000", "--raw-file-input-sample-format", "cs16",
           "--output-rate", "744187.5", "--output-sample-format", "cs16", "--freq-shift", "200000", "--shards", str(shards), "--devices", "8",
           "--chunk-frames", str(chunk), "--dry-placement", "--no-numa-bind", "--debug", "sysfs_root=" + str(tmp_path), *extra]
    return subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("profile", ["local", "dx"])
def test_harness_dry_placement_of_a_seamless_dc_rms_job(lib, tmp_path, profile):
    import iq_tool_amd as g
    kw = dict(NRSC5)
    total, chunk = 3_000_001, 65536
    p = _dry(tmp_path, total, "--seamless-dc-rms", "--dc-block", "--agc-profile", profile)
    assert p.returncode == 0, p.stderr
    r = json.loads(p.stdout.strip().splitlines()[-1])
    assert r["dry_placement"] is True and r["seamless_dc_rms"] is True and "seamless_dc" not in r and "seamless_rms" not in r
    pre = -(-g.design_preroll_frames_dcrms(**dict(kw, dc_block=True, agc=True, agc_profile=profile)) // chunk) * chunk   # in whole calls
    per, off, end = total // 3, 0, 0
    for s, sh in enumerate(r["per_shard"]):
        assert sh["first_frame"] == s * per // chunk * chunk == end
        end = sh["first_frame"] + sh["frames_in"]
        assert sh["preroll_frames"] == min(sh["first_frame"], pre)
        first, count = g.design_out_frames_range(sh["first_frame"], sh["frames_in"], **kw)
        assert (sh["out_offset_bytes"], sh["planned_out"]) == (4 * first, count) and sh["out_offset_bytes"] == off
        off += 4 * sh["planned_out"]
        assert sh["dc_rows"] == (-(-sh["frames_in"] // chunk) if s < 2 else 0)
    assert end == total and off // 4 == r["frames_out"]


def test_harness_refuses_what_the_mode_does_not_cover(lib, tmp_path):
    both = ("--dc-block", "--agc-profile", "local")
    for other in ("--seamless", "--seamless-agc", "--seamless-dc", "--seamless-rms", "--seamless-dc-agc"):
        for order in ((other, "--seamless-dc-rms"), ("--seamless-dc-rms", other)):
            p = _dry(tmp_path, 1 << 22, *order, *both)
            assert p.returncode == 2 and "excludes" in p.stderr and not p.stdout.strip(), (order, p.returncode, p.stderr)
    for extra, word in [(("--agc-profile", "local"), "--dc-block"), (("--dc-block",), "AGC"),
                        (("--dc-block", "--agc-profile", "digital"), "digital")]:
        p = _dry(tmp_path, 1 << 22, "--seamless-dc-rms", *extra)
        assert p.returncode == 1 and word in p.stderr and not p.stdout.strip(), (extra, p.returncode, p.stderr)
    p = _dry(tmp_path, 1 << 17, "--seamless-dc-rms", *both, shards=4)                   # too few frames for the grid
    assert p.returncode == 1 and "too few" in p.stderr
    # the older modes keep their refusal of such a chain, in their own words
    p = _dry(tmp_path, 1 << 22, "--seamless-dc", *both)
    assert p.returncode == 1 and "AGC" in p.stderr and not p.stdout.strip()
    p = _dry(tmp_path, 1 << 22, "--seamless-rms", *both)
    assert p.returncode == 1 and "DC blocker" in p.stderr and not p.stdout.strip()
    p = _dry(tmp_path, 1 << 22, "--seamless-dc-agc", *both)
    assert p.returncode == 1 and "dx / local" in p.stderr and not p.stdout.strip()
