"""Seamless range sharding, host side (no device): the two design-time closed forms a stitching writer needs --
iqgpu_design_out_frames_range, iqgpu_design_preroll_frames -- their refusals, and the harness's `--shards N --seamless` plan.

The range law is checked against an integer restatement written here in Python big ints over what iqgpu_chain_info reports
(arb_step, num_halfband_stages, filter_block, interp), not against the library's own arithmetic; the preroll against a lower bound
of summed tap spans computed here, deliberately on the short side."""
import ctypes as C
import json
import math
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EFORMAT, EUNSUPPORTED = -1, -5, -10

SHAPES = {
    "nrsc5": dict(in_format="cs16", out_format="cs16", input_rate_hz=2.4e6, target_rate_hz=744187.5, shift_hz=200e3),
    "fft1025_behind_10M_to_2M4": dict(in_format="cs16", out_format="cs16", input_rate_hz=10e6, target_rate_hz=2.4e6,
                                      filters=(("passband", 158.5e3, 113e3),), filter_taps=1024),
    "fir4097_behind_61M44_to_1M488": dict(in_format="cu8", out_format="cu8", input_rate_hz=61.44e6, target_rate_hz=1488375.0,
                                          filters=(("lowpass", 300e3, 0.0),), filter_taps=4097, filter_impl="fir"),
    "up_2M0_to_2M4": dict(in_format="cs16", out_format="cs16", input_rate_hz=2.0e6, target_rate_hz=2.4e6),
    "fft_in_front_of_1M0_to_2M5": dict(in_format="cs16", out_format="cf32", input_rate_hz=1.0e6, target_rate_hz=2.5e6,
                                       filters=(("lowpass", 200e3, 0.0),), filter_taps=257, filter_impl="fft"),
    "no_resample_fft": dict(input_rate_hz=2.4e6, no_resample=True, filters=(("passband", -300e3, 100e3),), transition_width_hz=20e3,
                            attenuation_db=70.0, filter_impl="fft", fft_size=2048),
    # ratios beyond 2^+-5.5 (tests/test_gpu_far_ratios.py runs them on the device): seven and nine half-band stages down, eight up
    "down_s7_10M_to_48k": dict(in_format="cs16", out_format="cs16", input_rate_hz=10e6, target_rate_hz=48e3, shift_hz=-25e3),
    "down_s9_20M_to_20k2": dict(in_format="cs16", out_format="cs16", input_rate_hz=20e6, target_rate_hz=20.2e3, shift_hz=-28e3),
    "up_s8_5k_to_2M4": dict(in_format="cu8", out_format="cs16", input_rate_hz=5e3, target_rate_hz=2.4e6),
}
# name -> (half-band stages, interpolating, stage semi-lengths in run order) of the deep chains
DEEP = {"down_s7_10M_to_48k": (7, 0, [3, 3, 3, 3, 3, 5, 10]), "down_s9_20M_to_20k2": (9, 0, [3] * 7 + [5, 10]), "up_s8_5k_to_2M4": (8, 1, None)}
POINTWISE = dict(in_format="cs16", out_format="cf32", input_rate_hz=2.4e6, no_resample=True, shift_hz=100e3)


@pytest.fixture(scope="module")
def lib():
    import iq_tool_amd
    return iq_tool_amd.load()


def probe(lib, **kw):
    from iq_tool_amd import _lib
    from iq_tool_amd.chain import make_desc
    d = make_desc(**kw)
    info = _lib.ChainInfo()
    assert lib.iqgpu_design_probe(C.byref(d), C.byref(info), None, 0, None, 0, None, 0) == 0
    return d, info


def out_range(lib, d, first, n):
    a, b = C.c_uint64(99), C.c_uint64(99)
    rc = lib.iqgpu_design_out_frames_range(C.byref(d), first, n, C.byref(a), C.byref(b))
    return rc, a.value, b.value


def preroll(lib, d):
    n = C.c_uint64(99)
    rc = lib.iqgpu_design_preroll_frames(C.byref(d), C.byref(n))
    return rc, n.value


def outputs_in_front_of(kw, info, a):
    """frames ONE stream has emitted when it has consumed a input frames, in Python integers"""
    S, step, block = int(info.num_halfband_stages), int(info.arb_step), int(info.filter_block)
    if kw.get("no_resample"):
        return a // block * block if block else a
    pre_filter = info.filter_ntaps > 0 and not info.filter_post_resample
    if info.interp or pre_filter:
        # r >= 1 form: the filter's block floor in front of the resampler, one burst of 2^S frames per polyphase output
        n_x = a // block * block if block else a
        return (-(-(n_x << 24) // step)) << (S if info.interp else 0)
    n = -(-((a >> S) << 24) // step)                    # ceil(groups 2^24 / step)
    return n // block * block if block else n


def positions(kw, info):
    S, block = int(info.num_halfband_stages), int(info.filter_block)
    pos = [0, 1, (1 << S) - 1, 1 << S, 4096, 2 * 10**10 + 12345, (1 << 36) - 7]
    if block:
        # the first input position at which a whole block has been emitted, and its neighbours
        lo, hi = 0, 1 << 30
        while lo < hi:
            mid = (lo + hi) // 2
            if outputs_in_front_of(kw, info, mid) >= block:
                hi = mid
            else:
                lo = mid + 1
        pos += [lo - 1, lo, lo + 1, 5 * lo - 1, 5 * lo + 1]
    return [p for p in pos if p >= 0]


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_range_law_against_an_integer_restatement(lib, name):
    kw = SHAPES[name]
    d, info = probe(lib, **kw)
    if "fft" in name:
        assert info.filter_block > 0, name
    if name == "fir4097_behind_61M44_to_1M488":
        assert info.filter_ntaps == 4097 and info.filter_block == 0 and info.num_halfband_stages == 5
    if name == "up_2M0_to_2M4":
        assert info.interp == 1
    if name in DEEP:
        S, interp, m = DEEP[name]
        assert (info.num_halfband_stages, info.interp) == (S, interp) and info.filter_ntaps == 0
        assert m is None or [int(info.stage_m[g]) for g in range(S)] == m
    for a in positions(kw, info):
        for n in (0, 1, 4095, 131_072 + 5, 10**9 + 1):
            rc, first, count = out_range(lib, d, a, n)
            assert rc == 0, (a, n, lib.iqgpu_last_error())
            want_first = outputs_in_front_of(kw, info, a)
            want = outputs_in_front_of(kw, info, a + n) - want_first
            assert (first, count) == (want_first, want), (name, a, n)
    # from frame 0 it is the count of a fresh chain
    for n in (0, 1, 1023, 50_001, 2 * 10**10 + 12345):
        got = C.c_size_t(0)
        assert lib.iqgpu_design_out_frames(C.byref(d), n, C.byref(got)) == 0
        assert out_range(lib, d, 0, n) == (0, 0, got.value)


def _tiles(lib, name, n, cuts):
    d, _ = probe(lib, **SHAPES[name])
    edges = sorted({0, n, *[c % (n + 1) for c in cuts]})
    whole = C.c_size_t(0)
    assert lib.iqgpu_design_out_frames(C.byref(d), n, C.byref(whole)) == 0
    run = 0
    for a, b in zip(edges[:-1], edges[1:]):
        rc, first, count = out_range(lib, d, a, b - a)
        assert rc == 0 and first == run, (name, edges, a)
        run += count
    assert run == whole.value


try:
    from hypothesis import HealthCheck, given, settings
    from hypothesis import strategies as st
except ImportError:                                          # (as tests/test_fuzz_host.py: the property needs hypothesis)
    def test_ranges_tile_the_output_of_one_stream():
        pytest.skip("needs hypothesis")
else:
    @settings(max_examples=int(os.environ.get("IQGPU_FUZZ_EXAMPLES", "150")), deadline=None, derandomize=True, database=None,
              suppress_health_check=[HealthCheck.too_slow, HealthCheck.function_scoped_fixture])
    @given(st.sampled_from(sorted(SHAPES)), st.integers(1, 1 << 36), st.lists(st.integers(0, 1 << 36), min_size=0, max_size=9))
    def test_ranges_tile_the_output_of_one_stream(lib, name, n, cuts):
        """any cut points 0 = a_0 < ... < a_k = n: the ranges' frames_out sum to iqgpu_design_out_frames(n) and every out_first
        is the running sum"""
        _tiles(lib, name, n, cuts)


def preroll_lower_bound(kw, info):
    """summed tap spans in input frames, on the short side: half-band stages in run order (4 m_g - 2) 2^g, the polyphase window
    13 2^S, the user filter's L - 1 taps and, for the FFT kind, one block, at the rate the filter runs at"""
    S = int(info.num_halfband_stages)
    ratio = float(info.ratio)
    n = 0.0
    resampled = not kw.get("no_resample")
    pre_filter = info.filter_ntaps > 0 and not info.filter_post_resample
    decim = resampled and not info.interp and not pre_filter
    if decim:
        n += sum((4 * int(info.stage_m[g]) - 2) << g for g in range(S)) + (13 << S)
    elif resampled:
        n += 13
    if info.filter_ntaps:
        per_out = 1.0 / ratio if decim else 1.0
        n += (int(info.filter_ntaps) - 1) * per_out + int(info.filter_block) * per_out
    return n


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_preroll_covers_the_tap_spans_and_grows_by_the_dc_warm_up(lib, name):
    kw = SHAPES[name]
    d, info = probe(lib, **kw)
    rc, p = preroll(lib, d)
    assert rc == 0
    low = preroll_lower_bound(kw, info)
    assert low > 0 and p >= low, (name, p, low)
    if name in DEEP:
        assert info.num_halfband_stages == DEEP[name][0]
        if not info.interp:
            assert low > 26 << info.num_halfband_stages          # the last two stages (m = 5, 10) and the polyphase window alone
    d_dc, info_dc = probe(lib, **dict(kw, dc_block=True))
    rc, p_dc = preroll(lib, d_dc)
    assert rc == 0 and info_dc.dc_alpha > 0
    assert p_dc - p == math.ceil(math.log(1e6) / float(info_dc.dc_alpha)), (name, p, p_dc)


def test_preroll_of_a_pointwise_chain_is_zero(lib):
    d, _ = probe(lib, **POINTWISE)                        # unpack -> NCO -> pack
    assert preroll(lib, d) == (0, 0)
    d, _ = probe(lib, **dict(POINTWISE, shift_hz=0.0, in_format="cu8", out_format="cs16"))
    assert preroll(lib, d) == (0, 0)


@pytest.mark.parametrize("profile", ["digital", "dx", "local"])
def test_agc_descriptions_are_refused(lib, profile):
    d, _ = probe(lib, agc=True, agc_profile=profile, **SHAPES["nrsc5"])
    assert preroll(lib, d) == (EUNSUPPORTED, 0)
    assert "AGC" in lib.iqgpu_last_error().decode()
    assert out_range(lib, d, 4096, 4096) == (EUNSUPPORTED, 0, 0)
    # create-time validation keeps its own codes and comes first
    from iq_tool_amd.chain import make_desc
    bad = make_desc(agc=True, **SHAPES["nrsc5"])
    bad.in_format = 77
    assert preroll(lib, bad)[0] == EFORMAT and out_range(lib, bad, 0, 1)[0] == EFORMAT


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_positions_beyond_the_arithmetic_are_refused_not_wrapped(lib, name):
    d, _ = probe(lib, **SHAPES[name])
    assert out_range(lib, d, (1 << 36) - 4096, 4096)[0] == 0          # 2^36 frames as one stream works
    for first, n in [(1 << 63, 1), ((1 << 64) - 1, 1), (1, (1 << 64) - 1), (1 << 62, 1 << 62), ((1 << 64) - 4096, 8192)]:
        assert out_range(lib, d, first, n) == (EINVAL, 0, 0), (first, n)
    a, b = C.c_uint64(0), C.c_uint64(0)
    assert lib.iqgpu_design_out_frames_range(None, 0, 0, C.byref(a), C.byref(b)) == EINVAL
    assert lib.iqgpu_design_preroll_frames(C.byref(d), None) == EINVAL


def test_python_mirror(lib):
    import iq_tool_amd
    kw = SHAPES["fft1025_behind_10M_to_2M4"]
    d, info = probe(lib, **kw)
    assert iq_tool_amd.design_preroll_frames(**kw) == preroll(lib, d)[1]
    assert iq_tool_amd.design_out_frames_range(123_457, 1 << 20, **kw) == out_range(lib, d, 123_457, 1 << 20)[1:]
    with pytest.raises(iq_tool_amd.IqgpuError) as e:
        iq_tool_amd.design_preroll_frames(agc=True, **kw)
    assert e.value.code == EUNSUPPORTED


# --------------------------------------------------------------------------------------------
# the harness's plan: iqgpu_run --dry-placement --shards 8 --seamless on a stand-in sysfs (no GPU call)
# --------------------------------------------------------------------------------------------
def _two_socket_sysfs(root):
    """KFD topology + PCI devices of an 8-GPU, two-socket box: nodes 0, 1 are the CPU sockets, the GPUs follow"""
    def put(path, text):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as fh:
            fh.write(text)
    allowed = sorted(os.sched_getaffinity(0))
    cpus = ",".join(str(c) for c in allowed)
    nodes = os.path.join(root, "class", "kfd", "kfd", "topology", "nodes")
    for n in range(2):
        put(os.path.join(nodes, str(n), "properties"), "cpu_cores_count 64\nsimd_count 0\nlocation_id 0\ndomain 0\n")
    for i, bus in enumerate([0x0d, 0x26, 0x43, 0x5b, 0x8a, 0xa7, 0xc4, 0xdc]):
        put(os.path.join(nodes, str(2 + i), "properties"), "cpu_cores_count 0\nsimd_count 1024\nlocation_id %d\ndomain 0\n" % (bus << 8))
        dev = os.path.join(root, "bus", "pci", "devices", "0000:%02x:00.0" % bus)
        put(os.path.join(dev, "numa_node"), "%d\n" % (0 if i < 4 else 1))
        put(os.path.join(dev, "local_cpulist"), cpus + "\n")


def _dry(tmp_path, total, *extra, shards=8):
    from iq_tool_amd.build import HARNESS_BIN
    env = dict(os.environ)
    for k in ("ROCR_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        env.pop(k, None)
    cmd = [HARNESS_BIN, "--synthetic", str(total), "--synthetic-hash", "7", "--raw-file-input-rate", "2400000", "--raw-file-input-sample-format", "cs16",
           "--output-rate", "744187.5", "--output-sample-format", "cs16", "--freq-shift", "200000", "--shards", str(shards), "--devices", "8",
           "--dry-placement", "--debug", "sysfs_root=" + str(tmp_path), *extra]
    return subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=120)


def test_harness_dry_placement_of_a_seamless_job(lib, tmp_path):
    import iq_tool_amd
    _two_socket_sysfs(str(tmp_path))
    total = 8 * 2_500_000_000 + 12_345
    p = _dry(tmp_path, total, "--seamless")
    assert p.returncode == 0, p.stderr
    r = json.loads(p.stdout.strip().splitlines()[-1])
    assert r["dry_placement"] is True and r["seamless"] is True and r["shards"] == 8 and r["distinct_devices"] == 8
    kw = SHAPES["nrsc5"]
    want_pre = iq_tool_amd.design_preroll_frames(**kw)
    assert want_pre > 0
    per, off, end = total // 8, 0, 0
    for s, sh in enumerate(r["per_shard"]):
        assert sh["first_frame"] % 4096 == 0 and sh["first_frame"] == s * per // 4096 * 4096 and sh["first_frame"] == end
        end = sh["first_frame"] + sh["frames_in"]
        assert sh["preroll_frames"] == (0 if s == 0 else want_pre)
        first, count = iq_tool_amd.design_out_frames_range(sh["first_frame"], sh["frames_in"], **kw)
        assert (sh["out_offset_bytes"], sh["planned_out"]) == (4 * first, count) and sh["out_offset_bytes"] == off
        off += 4 * sh["planned_out"]
    assert end == total
    # the stitched file is as long as the single stream's
    assert off // 4 == iq_tool_amd.design_out_frames(total, **kw) == r["frames_out"]
    # a preroll never reaches in front of frame 0: shards that start inside the chain's memory are warmed up from the start
    p = _dry(tmp_path, 16 * 1024, "--seamless", shards=4)
    assert p.returncode == 0, p.stderr
    r = json.loads(p.stdout.strip().splitlines()[-1])
    assert [sh["first_frame"] for sh in r["per_shard"]] == [0, 4096, 8192, 12288]
    assert [sh["preroll_frames"] for sh in r["per_shard"]] == [0, min(4096, want_pre), min(8192, want_pre), min(12288, want_pre)]


def test_harness_without_seamless_reports_what_it_always_did(lib, tmp_path):
    _two_socket_sysfs(str(tmp_path))
    p = _dry(tmp_path, 8 * 2_500_000_000)
    assert p.returncode == 0, p.stderr
    r = json.loads(p.stdout.strip().splitlines()[-1])
    assert "seamless" not in r and all("preroll_frames" not in sh for sh in r["per_shard"])
    assert [sh["first_frame"] for sh in r["per_shard"]] == [s * 2_500_000_000 for s in range(8)]


def test_harness_refuses_seamless_with_an_agc_option(lib, tmp_path):
    _two_socket_sysfs(str(tmp_path))
    p = _dry(tmp_path, 1 << 24, "--seamless", "--agc-profile", "digital")
    assert p.returncode != 0 and "AGC" in p.stderr and not p.stdout.strip()
    p = _dry(tmp_path, 1 << 24, "--agc-profile", "digital")          # independent shards keep their AGC
    assert p.returncode == 0, p.stderr
