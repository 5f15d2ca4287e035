"""Seamless range sharding of chains with the dx / local output AGC, host side (no device): the preroll iqgpu_design_preroll_frames_rms
asks for is long enough at EVERY stream position, its error codes, the ctypes prototypes, and the harness's refusals.

The property (include/iqgpu.h): with P_fir the FIR memory (iqgpu_design_preroll_frames of the description without the AGC) and
P_rms what the new call reports, the last P_rms - P_fir input frames in front of any position make the chain emit at least
warm + chunk output frames -- the window k_agc_rms_seek may need -- whatever the open group, the resampler phase and the pending
FFT-block samples are there.  The yardstick is the existing closed form, iqgpu_design_out_frames_range, not the new code."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "iq_tool_amd", "lib", "iqgpu_run")
EINVAL, EUNSUPPORTED = -1, -10
# agc_rms_geometry (agc.hip): warm = 26 / alpha, chunk = max(256, warm / 16), both even
WINDOW = {"local": (2600, 256), "dx": (260000, 16250)}
NEW = ("iqgpu_design_preroll_frames_rms", "iqgpu_chain_seek_rms", "iqgpu_chain_seek_rms_device")


@pytest.fixture(scope="module")
def lib():
    import iq_tool_amd
    return iq_tool_amd.load()


def random_desc(rng):
    """ratios both ways and none, no filter / FIR / FFT filter (behind a decimating resampler, in front of an interpolating one)"""
    in_rate = float(rng.choice([96e3, 1.0e6, 2.4e6, 10e6]))
    kind = rng.integers(0, 5)
    kw = dict(in_format="cs16", out_format="cs16", input_rate_hz=in_rate)
    if kind == 0:
        kw.update(no_resample=True, target_rate_hz=in_rate)
    else:
        lo, hi = ((0.004, 0.98) if kind in (1, 2) else (1.02, 6.0))
        kw.update(target_rate_hz=in_rate * float(np.exp(rng.uniform(np.log(lo), np.log(hi)))))
    filt = rng.integers(0, 3)
    if filt:
        edge = 0.2 * min(kw["target_rate_hz"], in_rate)
        kw.update(filters=(("lowpass", edge, 0.0),), filter_taps=int(rng.choice([31, 63, 129])),
                  filter_impl="fir" if filt == 1 else "fft")
        if filt == 2 and rng.integers(0, 2):
            kw.update(fft_size=int(rng.choice([512, 1024, 4096])))
    return kw


def test_preroll_emits_the_agc_window_at_every_position(lib):
    import iq_tool_amd as g
    rng = np.random.default_rng(20240607)
    seen = set()
    for trial in range(60):
        kw = random_desc(rng)
        profile = ("local", "dx")[trial % 2]
        warm, chunk = WINDOW[profile]
        p_fir = g.design_preroll_frames(**kw)
        p_rms = g.design_preroll_frames_rms(**dict(kw, agc=True, agc_profile=profile))
        extra = p_rms - p_fir
        assert extra > 0
        info = g.chain.ChainInfo()
        d = g.make_desc(**kw)
        assert lib.iqgpu_design_probe(C.byref(d), C.byref(info), None, 0, None, 0, None, 0) == 0
        seen.add((bool(kw.get("no_resample")), int(info.interp), bool(info.filter_block), int(info.filter_post_resample)))
        positions = [p_rms, p_rms + 1, p_rms + 4096, 1 << 30, (1 << 38) + 12345] + [int(x) for x in rng.integers(p_rms, 1 << 36, 40)]
        worst = min(g.design_out_frames_range(pos - extra, extra, **kw)[1] for pos in positions)
        print("trial %d %s ratio %.5f filter %s block %d: P_fir %d P_rms %d, fewest outputs of the last %d frames %d (needs %d)"
              % (trial, profile, info.ratio, kw.get("filter_impl", "none"), info.filter_block, p_fir, p_rms, extra, worst, warm + chunk))
        assert worst >= warm + chunk, (kw, profile)
        # ... and not absurdly more: the bound is the worst position's, within a block, a group and a few outputs of it
        slack = info.filter_block * (max(info.ratio, 1.0) if not info.filter_post_resample else 1.0) * 2 + 2 * (1 << info.num_halfband_stages) + 8
        assert worst <= warm + chunk + 2 * slack, (kw, profile, worst)
    # every family of the closed form was drawn: no resampler, both directions, FFT block on either side
    assert {s[0] for s in seen} == {True, False} and {s[1] for s in seen} == {0, 1}
    assert any(s[2] and s[3] for s in seen) and any(s[2] and not s[3] and not s[0] for s in seen)


def test_error_codes_are_design_probes_then_the_seeks_refusals(lib):
    import iq_tool_amd as g
    n = C.c_uint64(7)
    assert lib.iqgpu_design_preroll_frames_rms(None, C.byref(n)) == EINVAL
    d = g.make_desc(agc=True, agc_profile="local")
    assert lib.iqgpu_design_preroll_frames_rms(C.byref(d), None) == EINVAL
    assert b"NULL" in lib.iqgpu_last_error()
    # a description create refuses: design_probe's own code, and *frames = 0
    bad = [dict(target_rate_hz=2.4e6 * 1e-4), dict(in_format=7), dict(shift_hz=2.4e6 * 6), dict(filters=(("lowpass", 700e3, 0.0),)),
           dict(agc_profile=9), dict(block_samples=1000)]
    for over in bad:
        d = g.make_desc(**dict(dict(agc=True, agc_profile="local"), **over))
        info = g.chain.ChainInfo()
        want = lib.iqgpu_design_probe(C.byref(d), C.byref(info), None, 0, None, 0, None, 0)
        n = C.c_uint64(7)
        got = lib.iqgpu_design_preroll_frames_rms(C.byref(d), C.byref(n))
        print(over, "design_probe", want, "preroll_frames_rms", got)
        assert want < 0 and got == want and n.value == 0
    # descriptions the seek refuses: no AGC (EINVAL), digital and the DC blocker (EUNSUPPORTED)
    for over, code, word in ((dict(agc=False), EINVAL, "no output AGC"), (dict(agc_profile="digital"), EUNSUPPORTED, "iqgpu_chain_seek_agc"),
                             (dict(dc_block=True), EUNSUPPORTED, "DC blocker")):
        with pytest.raises(g.IqgpuError) as e:
            g.design_preroll_frames_rms(**dict(dict(agc=True, agc_profile="local"), **over))
        assert e.value.code == code and word in str(e.value)
    # both spellings of the Python call
    kw = dict(agc=True, agc_profile="dx")
    assert g.design_preroll_frames_rms(g.make_desc(**kw)) == g.design_preroll_frames_rms(**kw) > 260000 + 16250


def test_entry_points_are_declared_bound_and_refuse_null(lib):
    from iq_tool_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "iqgpu.h")).read()
    assert int(re.search(r"#define\s+IQGPU_ABI_VERSION\s+(\d+)", hdr).group(1)) == 9 == lib.iqgpu_abi_version()
    bound = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in bound and getattr(lib, name).argtypes == bound[name][1]
    buf = (C.c_char * 64)()
    assert lib.iqgpu_chain_seek_rms(None, 0, None, 0) == EINVAL
    assert lib.iqgpu_chain_seek_rms_device(None, 4096, buf, 16) == EINVAL
    assert b"NULL" in lib.iqgpu_last_error()
    import iq_tool_amd
    assert hasattr(iq_tool_amd.Chain, "seek_rms") and hasattr(iq_tool_amd.Chain, "seek_rms_device")


def harness(*args):
    return subprocess.run([EXE, *args], capture_output=True, text=True)


def test_harness_plans_and_refuses_without_a_device(lib):
    import json
    import iq_tool_amd as g
    args = ["--raw-file-input-rate", "2.4e6", "--raw-file-input-sample-format", "cs16", "--output-rate", "744187.5",
            "--output-sample-format", "cs16", "--freq-shift", "200e3"]
    base = ["--synthetic", "3000000", "--synthetic-hash", "1", *args, "--shards", "3", "--dry-placement", "--no-numa-bind", "--seamless-rms"]
    r = harness(*base, "--output-agc")                                       # --output-agc alone is the local profile
    assert r.returncode == 0, r.stderr
    info = json.loads(r.stdout.strip().splitlines()[-1])
    kw = dict(in_format="cs16", out_format="cs16", input_rate_hz=2.4e6, target_rate_hz=744187.5, shift_hz=200e3)
    p = g.design_preroll_frames_rms(**dict(kw, agc=True, agc_profile="local"))
    assert info["seamless_rms"] is True and len(info["per_shard"]) == 3
    at = 0
    for s, ps in enumerate(info["per_shard"]):
        assert ps["first_frame"] == at == (s * 1000000) // 4096 * 4096 and ps["preroll_frames"] == min(at, p)
        first, count = g.design_out_frames_range(at, ps["frames_in"], **kw)
        assert ps["planned_out"] == count and ps["out_offset_bytes"] == 4 * first
        at += ps["frames_in"]
    assert at == 3000000
    # chains the seek refuses, in the library's words
    for extra, word in ((["--agc-profile", "digital"], "iqgpu_chain_seek_agc"), ([], "no output AGC"), (["--output-agc", "--dc-block"], "DC blocker")):
        r = harness(*base, *extra)
        assert r.returncode == 1 and word in r.stderr, r.stderr
    r = harness(*base, "--output-agc", "--seamless")
    assert r.returncode == 2
    r = harness("--synthetic", "3000000", *args, "--shards", "3", "--dry-placement", "--seamless-rms", "--output-agc")
    assert r.returncode == 2 and "--synthetic-hash" in r.stderr
