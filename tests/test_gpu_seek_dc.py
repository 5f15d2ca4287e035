"""Exact seamless range sharding of chains with the DC blocker, on the device: measure the map of every call (iqgpu_chain_dc_measure),
walk the maps (iqgpu_chain_dc_advance), start a chain mid-stream with the walked state (iqgpu_chain_seek_dc).

Every comparison here is for equality of bytes -- of the blocker's double state against the state a processing chain reports after
every call, and of output frames against ONE chain that processes the stream on the same call grid.  No tolerance appears anywhere:
a call a shard makes is a call the single stream makes, from the same state, so any differing bit is a defect.

The streams are synth.raw_stream with a DC offset added (a fifth of full scale), so that the state |v| ~ offset / alpha is of the
order 1e4 and an error in its last bits would reach the output codes."""
import ctypes as C
import filecmp
import functools
import os
import subprocess

import numpy as np
import pytest

from iq_tool_amd import synth

from shard_support import EINVAL, EUNSUPPORTED, EXE, expect, frames, run, same as same_bytes, set_switches

pytestmark = pytest.mark.gpu
CALL = 131072
SWITCHES = ("FORCE_FAT", "FAT", "NO_P0", "NO_S2", "FORCE_GENERIC", "NO_FAST", "FFT_NO_R16", "FFT_LOG2N", "NO_FAT", "NO_CASC2", "CASC2_MIN_RUN")

CONFIG3_FRONT = dict(in_format="cs16", out_format="cs16", input_rate_hz=10e6, target_rate_hz=2.4e6, dc_block=True, iq_correct=True,
                     iq_mag=0.01, iq_phase=-0.005)
CONFIG3_FILTER = dict(filters=(("passband", 158.5e3, 113e3),), filter_taps=1024)              # 1025 taps, FFT kind, block 2048
NRSC5_DC = dict(in_format="cs16", out_format="cs16", input_rate_hz=2.4e6, target_rate_hz=744187.5, shift_hz=200e3, dc_block=True)
CU8_NRSC5_DC = dict(in_format="cu8", out_format="cu8", input_rate_hz=2.4e6, target_rate_hz=1488375.0, dc_block=True)
CF32_POINTWISE_DC = dict(in_format="cf32", out_format="cs16", input_rate_hz=2.4e6, no_resample=True, shift_hz=100e3, dc_block=True)

# name -> (description, IQGPU_<NAME> switches, front kernel of a whole grid call): both DcGeom modes (wave runs: the first four;
# regular blocks of k_front: the last two) and every load path of k_dc_prefix (16-bit, 8-bit, the general one on cf32)
ROUTINGS = {
    "config3_front_s2": (CONFIG3_FRONT, {}, "k_front_s2"),
    "config3_front_cascade": (CONFIG3_FRONT, dict(NO_S2="1"), "k_cascade+k_front_s1"),
    "nrsc5_cs16_s1": (NRSC5_DC, {}, "k_front_s1"),
    "nrsc5_cu8": (CU8_NRSC5_DC, {}, "k_front_s1"),
    "generic": (NRSC5_DC, dict(FORCE_GENERIC="1"), "k_front"),
    "cf32_no_resample": (CF32_POINTWISE_DC, {}, "k_front"),
}


@functools.lru_cache(maxsize=None)
def dc_stream(n, rate_hz, fmt):
    """synth.raw_stream plus a DC offset of about (0.2, -0.15) of full scale, as interleaved components of the raw format (read only)"""
    raw = synth.raw_stream(n, rate_hz, 61, fmt)
    if fmt == "cf32":
        out = (raw.reshape(-1, 2) + np.array([0.2, -0.15], np.float32)).astype(np.float32).reshape(-1)
    else:
        off, lo, hi = {"cs16": ((6500, -4900), -32768, 32767), "cu8": ((25, -19), 0, 255)}[fmt]
        out = np.clip(raw.reshape(-1, 2).astype(np.int32) + np.array(off, np.int32), lo, hi).astype(raw.dtype).reshape(-1)
    out.setflags(write=False)
    return out


def calls(n, c=CALL):
    return [(a, min(a + c, n)) for a in range(0, n, c)]


def p_fir(gpu, kw):
    return gpu.design_preroll_frames(**dict(kw, dc_block=False))


def single_stream(gpu, kw, raw, n, c=CALL):
    """ONE chain over the stream on the call grid: (output of every call, DC state behind every call, front kernel of the first call)"""
    ch = gpu.Chain(**kw)
    outs, states, kernel = [], [], None
    for a, b in calls(n, c):
        outs.append(ch.process(frames(kw, raw, a, b)))
        states.append(ch.dc_state().copy())
        kernel = kernel or ch.front_kernel()
    return outs, states, kernel


def measure_all(gpu, ch, kw, raw, n, c=CALL, unaligned=()):
    from iq_tool_amd.chain import DC_ROW
    rows = np.zeros(len(calls(n, c)), DC_ROW)
    for k, (a, b) in enumerate(calls(n, c)):
        src = frames(kw, raw, a, b)
        if k in unaligned:
            # the same frames from a host address that is 1 byte past an aligned one: the call is staged like any other
            pad = np.empty(src.nbytes + 64, np.uint8)
            lead = (-pad.ctypes.data) % 16 + 1
            pad[lead:lead + src.nbytes] = src
            src = pad[lead:lead + src.nbytes]
            assert src.ctypes.data % 16 == 1
        rows[k] = ch.dc_measure(a, src)
        assert rows[k]["frames"] == b - a and 0.0 < rows[k]["f"] <= 1.0
    return rows


# --------------------------------------------------------------------------------------------
# 1. the walked state is the stream's, bit for bit
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ROUTINGS))
def test_walked_state_is_the_streams_bit_for_bit(gpu, monkeypatch, name):
    kw, sw, kernel = ROUTINGS[name]
    set_switches(monkeypatch, SWITCHES, sw)
    n = 6 * CALL + 50_001                                        # six whole calls and a ragged, odd one
    raw = dc_stream(n, kw["input_rate_hz"], kw["in_format"])
    outs, states, got_kernel = single_stream(gpu, kw, raw, n)
    print("%s: %s, |v| behind the stream %.6g" % (name, got_kernel, float(np.hypot(states[-1]["re"], states[-1]["im"]))))
    assert got_kernel == kernel
    assert np.hypot(states[-1]["re"], states[-1]["im"]) > 1000.0           # a state whose last bits matter

    m = gpu.Chain(**kw)
    rows = measure_all(gpu, m, kw, raw, n, unaligned=(2,))
    st, before = m.dc_advance(None, rows)
    assert before.size == len(states)
    zero = np.zeros((), before.dtype)
    for k in range(len(states)):
        want = zero if k == 0 else states[k - 1]
        assert same_bytes(before[k], want), (name, k, before[k], want)
    assert same_bytes(st, states[-1]), (name, st, states[-1])
    # ... however the rows are grouped into walks
    st2, _ = m.dc_advance(None, rows[:3])
    st2, before2 = m.dc_advance(st2, rows[3:])
    assert same_bytes(st2, st) and same_bytes(before2, before[3:])

    # the measuring chain is exactly as it was: it now processes the stream -- measuring another position half way -- to the bytes
    # of the chain that never measured
    assert same_bytes(m.dc_state(), zero)
    for k, (a, b) in enumerate(calls(n)):
        if k == 4:
            again = m.dc_measure(CALL, frames(kw, raw, CALL, 2 * CALL))
            assert same_bytes(again, rows[1])
        assert same_bytes(m.process(frames(kw, raw, a, b)), outs[k]), (name, k)
        assert same_bytes(m.dc_state(), states[k])


def test_device_variant_measures_the_same_row(gpu):
    kw = CONFIG3_FRONT
    n = 2 * CALL
    raw = dc_stream(6 * CALL + 50_001, kw["input_rate_hz"], kw["in_format"])
    ch = gpu.Chain(**kw)
    src = frames(kw, raw, CALL, n)
    buf = gpu.DeviceBuffer(src.nbytes)
    buf.upload(src)
    assert same_bytes(ch.dc_measure_device(CALL, buf.ptr, CALL), ch.dc_measure(CALL, src))
    buf.free()


@pytest.mark.parametrize("lead", [0, 4])
def test_device_variants_continue_the_stream_at_the_single_streams_alignment(gpu, lead):
    """process_device, dc_measure_device and seek_dc_device on device addresses: every call of the single stream and of the shard
    starts `lead` bytes past a 16-byte boundary (0: the aligned load paths; 4: raw_aligned = 0 -- k_dc_prefix's and the front
    kernel's unaligned paths and the segmentation that goes with them), the same on both sides as the header asks."""
    kw = dict(CONFIG3_FRONT, **CONFIG3_FILTER)
    n, k0 = 5 * CALL, 2
    raw = dc_stream(6 * CALL + 50_001, kw["input_rate_hz"], kw["in_format"])
    buf = gpu.DeviceBuffer(n * 4 + 64)
    stage = np.zeros(n * 4 + 64, np.uint8)
    stage[lead:lead + n * 4] = frames(kw, raw, 0, n)
    buf.upload(stage)
    assert buf.ptr % 16 == 0 and (CALL * 4) % 16 == 0
    at = lambda k: buf.ptr + lead + k * CALL * 4               # device address of grid call k
    cap = gpu.Chain(**kw).max_out_frames(CALL) * 4
    out = gpu.DeviceBuffer(cap)

    def run(ch, k):
        got = ch.process_device(at(k), CALL, out.ptr, cap)
        ch.synchronize()
        return out.download(got * 4).copy()

    one = gpu.Chain(**kw)
    outs, states = [], []
    for k in range(n // CALL):
        outs.append(run(one, k))
        states.append(one.dc_state().copy())
    m = gpu.Chain(**kw)
    from iq_tool_amd.chain import DC_ROW
    rows = np.zeros(k0, DC_ROW)
    for k in range(k0):
        rows[k] = m.dc_measure_device(k * CALL, at(k), CALL)
    st, before = m.dc_advance(None, rows)
    assert same_bytes(st, states[k0 - 1]) and same_bytes(before[1], states[0])
    ch = gpu.Chain(**kw)
    ch.seek_dc_device(k0 * CALL, at(k0 - 1), CALL, CALL, before[k0 - 1])
    assert same_bytes(ch.dc_state(), states[k0 - 1])
    for k in range(k0, n // CALL):
        g = run(ch, k)
        assert g.size > 0 and same_bytes(g, outs[k]), (lead, k)
    assert same_bytes(ch.dc_state(), states[-1])
    buf.free(); out.free()


# --------------------------------------------------------------------------------------------
# 2. bytes: a chain started by seek_dc behind a preroll of whole grid calls writes the single stream's bytes
# --------------------------------------------------------------------------------------------
BYTE_CASES = [(name, fmt, False) for name in sorted(ROUTINGS) for fmt in ("cs16", "cf32")] + \
             [("config3_front_s2", "cs16", True), ("config3_front_s2", "cf32", True)]


@pytest.mark.parametrize("name,out_format,filtered", BYTE_CASES)
def test_seek_dc_continues_the_stream_byte_for_byte(gpu, monkeypatch, name, out_format, filtered):
    kw, sw, _ = ROUTINGS[name]
    kw = dict(kw, out_format=out_format, **(CONFIG3_FILTER if filtered else {}))
    set_switches(monkeypatch, SWITCHES, sw)
    n, k0 = 6 * CALL + 50_001, 3
    raw = dc_stream(n, kw["input_rate_hz"], kw["in_format"])
    assert p_fir(gpu, kw) <= CALL                                # the preroll is ONE grid call
    outs, states, _ = single_stream(gpu, kw, raw, n)
    m = gpu.Chain(**kw)
    _, before = m.dc_advance(None, measure_all(gpu, m, kw, raw, k0 * CALL))
    ch = gpu.Chain(**kw)
    ch.seek_dc(k0 * CALL, frames(kw, raw, (k0 - 1) * CALL, k0 * CALL), CALL, before[k0 - 1])
    assert same_bytes(ch.dc_state(), states[k0 - 1])
    total = differing = 0
    for k, (a, b) in enumerate(calls(n)):
        if k < k0:
            continue
        g = ch.process(frames(kw, raw, a, b))
        assert g.nbytes == outs[k].nbytes and (g.nbytes > 0 or filtered)
        differing += int((g.view(np.uint8) != outs[k].view(np.uint8)).sum())
        total += g.nbytes
    print("%s %s%s: %d of %d bytes differ behind the cut" % (name, out_format, " + fft1025" if filtered else "", differing, total))
    assert total > 0 and differing == 0
    assert same_bytes(ch.dc_state(), states[-1])


def test_preroll_of_three_grid_calls_where_the_call_is_shorter_than_the_filter_memory(gpu):
    c = 8192
    kw = dict(CONFIG3_FRONT, **CONFIG3_FILTER)
    p = p_fir(gpu, kw)
    assert p == 17_424 and c < p <= 3 * c
    n, k0 = 40 * c + 3_001, 21
    raw = dc_stream(6 * CALL + 50_001, kw["input_rate_hz"], kw["in_format"])
    outs, states, _ = single_stream(gpu, kw, raw, n, c)
    m = gpu.Chain(**kw)
    _, before = m.dc_advance(None, measure_all(gpu, m, kw, raw, k0 * c, c))
    ch = gpu.Chain(**kw)
    ch.seek_dc(k0 * c, frames(kw, raw, (k0 - 3) * c, k0 * c), c, before[k0 - 3])
    got = [ch.process(frames(kw, raw, a, b)) for a, b in calls(n, c)[k0:]]
    want = np.concatenate(outs[k0:])
    assert want.size > 0 and same_bytes(np.concatenate(got), want)
    # two grid calls are shorter than the filters' memory: refused
    with pytest.raises(gpu.IqgpuError) as e:
        ch.seek_dc(k0 * c, frames(kw, raw, (k0 - 2) * c, k0 * c), c, before[k0 - 2])
    assert e.value.code == EINVAL and "shorter" in str(e.value)


@pytest.mark.parametrize("filtered", [False, True])
def test_four_range_stitch_from_one_walk(gpu, filtered):
    kw = dict(CONFIG3_FRONT, **(CONFIG3_FILTER if filtered else {}))
    n = 6 * CALL + 50_001
    raw = dc_stream(n, kw["input_rate_hz"], kw["in_format"])
    outs, states, _ = single_stream(gpu, kw, raw, n)
    cuts = [0, 2, 3, 5]                                          # in grid calls; the last range takes the ragged call
    m = gpu.Chain(**kw)
    # measure: every range but the last, one row per grid call; walk: ONE dc_advance over all rows
    rows = measure_all(gpu, m, kw, raw, cuts[-1] * CALL)
    _, before = m.dc_advance(None, rows)
    grid = calls(n)
    stitched = []
    for r, k0 in enumerate(cuts):
        k1 = cuts[r + 1] if r + 1 < len(cuts) else len(grid)
        ch = gpu.Chain(**kw)
        if k0:
            ch.seek_dc(k0 * CALL, frames(kw, raw, (k0 - 1) * CALL, k0 * CALL), CALL, before[k0 - 1])
        stitched += [ch.process(frames(kw, raw, a, b)) for a, b in grid[k0:k1]]
    assert same_bytes(np.concatenate(stitched), np.concatenate(outs))


# --------------------------------------------------------------------------------------------
# 3. the old path asks for the warm-up where the new one does not
# --------------------------------------------------------------------------------------------
def test_seek_refuses_the_short_preroll_that_seek_dc_accepts(gpu):
    kw = dict(CONFIG3_FRONT, **CONFIG3_FILTER)
    n, k0 = 6 * CALL + 50_001, 3
    raw = dc_stream(n, kw["input_rate_hz"], kw["in_format"])
    p = p_fir(gpu, kw)
    assert gpu.design_preroll_frames(**kw) > 100 * p             # the warm-up of the blocker dominates what iqgpu_chain_seek asks for
    pre = frames(kw, raw, k0 * CALL - p, k0 * CALL)
    ch = gpu.Chain(**kw)
    with pytest.raises(gpu.IqgpuError) as e:
        ch.seek(k0 * CALL, pre)
    assert e.value.code == EINVAL and "shorter" in str(e.value)
    m = gpu.Chain(**kw)
    st, _ = m.dc_advance(None, np.atleast_1d(m.dc_measure(0, frames(kw, raw, 0, k0 * CALL - p))))
    ch.seek_dc(k0 * CALL, pre, 0, st)                            # accepted: P_fir frames, one call
    assert ch.process(frames(kw, raw, k0 * CALL, n)).size > 0


# --------------------------------------------------------------------------------------------
# 4. errors
# --------------------------------------------------------------------------------------------
def test_errors(gpu):
    from iq_tool_amd import _lib
    from iq_tool_amd.chain import DC_ROW
    kw = dict(CONFIG3_FRONT, **CONFIG3_FILTER)
    n, k0 = 3 * CALL, 2
    raw = dc_stream(6 * CALL + 50_001, kw["input_rate_hz"], kw["in_format"])
    fresh = gpu.Chain(**kw).process(frames(kw, raw, 0, n))
    pre = frames(kw, raw, (k0 - 1) * CALL, k0 * CALL)
    good = np.zeros(1, DC_ROW)
    good["f"] = 0.5

    # a chain without the blocker
    plain = gpu.Chain(**dict(kw, dc_block=False))
    expect(gpu, EINVAL, plain.dc_state, word="DC blocker")
    expect(gpu, EINVAL, plain.dc_measure, 0, frames(kw, raw, 0, CALL), word="DC blocker")
    expect(gpu, EINVAL, plain.dc_advance, None, good, word="DC blocker")
    expect(gpu, EINVAL, plain.seek_dc, k0 * CALL, pre, CALL, None, word="DC blocker")

    ch = gpu.Chain(**kw)
    lib, h = ch._lib, ch._h
    row, st = _lib.DcRow(), _lib.DcState()
    buf = np.zeros(64, np.uint8).ctypes.data_as(C.c_void_p)
    # NULL arguments
    assert lib.iqgpu_chain_get_dc_state(h, None) == EINVAL and lib.iqgpu_chain_get_dc_state(None, C.byref(st)) == EINVAL
    assert lib.iqgpu_chain_dc_measure(h, 0, buf, 8, None) == EINVAL and lib.iqgpu_chain_dc_measure(h, 0, None, 8, C.byref(row)) == EINVAL
    assert lib.iqgpu_chain_dc_measure(None, 0, buf, 8, C.byref(row)) == EINVAL
    assert lib.iqgpu_chain_dc_measure_device(h, 0, None, 8, C.byref(row)) == EINVAL
    assert lib.iqgpu_chain_dc_advance(h, None, good.ctypes.data_as(C.c_void_p), 1, None) == EINVAL
    assert lib.iqgpu_chain_dc_advance(h, C.byref(st), None, 1, None) == EINVAL
    assert lib.iqgpu_chain_dc_advance(None, C.byref(st), good.ctypes.data_as(C.c_void_p), 1, None) == EINVAL
    assert lib.iqgpu_chain_seek_dc(None, 0, None, 0, 0, None) == EINVAL and lib.iqgpu_chain_seek_dc_device(None, 0, None, 0, 0, None) == EINVAL
    assert lib.iqgpu_chain_seek_dc(h, k0 * CALL, None, CALL, CALL, None) == EINVAL           # NULL preroll
    # positions beyond 2^39 frames
    expect(gpu, EINVAL, ch.dc_measure, (1 << 39) + 1, frames(kw, raw, 0, 8), word="2^39")
    expect(gpu, EINVAL, ch.dc_measure, (1 << 39) - 4, frames(kw, raw, 0, 8), word="2^39")
    expect(gpu, EINVAL, ch.seek_dc, 1 << 63, None, 0, None, word="2^39")
    # prerolls: too short, in front of frame 0, not a whole number of calls
    expect(gpu, EINVAL, ch.seek_dc, k0 * CALL, pre[:4 * 1000], 0, None, word="shorter")
    expect(gpu, EINVAL, ch.seek_dc, 100, frames(kw, raw, 0, 101), 0, None)
    expect(gpu, EINVAL, ch.seek_dc, k0 * CALL, pre, 4096 * 3, None, word="whole number")
    assert same_bytes(ch.process(frames(kw, raw, 0, n)), fresh)              # a refused seek_dc leaves the chain reset
    # rows that no measurement gives
    for f, g_re, g_im in [(0.0, 0.0, 0.0), (-0.5, 0.0, 0.0), (1.5, 0.0, 0.0), (float("nan"), 0.0, 0.0), (0.5, float("inf"), 0.0),
                          (0.5, 0.0, float("nan"))]:
        bad = np.zeros(3, DC_ROW)
        bad["f"] = 0.5
        bad[1] = (f, g_re, g_im, 8)
        expect(gpu, EINVAL, ch.dc_advance, None, bad, word="row 1")
    st2, before = ch.dc_advance(None, np.zeros(0, DC_ROW))                 # no rows: the state as it came
    assert before.size == 0 and same_bytes(st2, np.zeros((), st2.dtype))
    one = np.zeros(1, DC_ROW)
    one[0] = (1.0, 2.0, -3.0, 8)                                           # f = 1 is in range
    st3, _ = ch.dc_advance(None, one)
    assert (float(st3["re"]), float(st3["im"])) == (2.0, -3.0)

    # with the output AGC: the state can be read, the exact recipe is not offered
    agc = gpu.Chain(**dict(NRSC5_DC, agc=True))
    araw = dc_stream(6 * CALL + 50_001, 2.4e6, "cs16")
    agc.process(frames(NRSC5_DC, araw, 0, CALL))
    assert np.hypot(agc.dc_state()["re"], agc.dc_state()["im"]) > 0.0
    expect(gpu, EUNSUPPORTED, agc.dc_measure, 0, frames(NRSC5_DC, araw, 0, CALL), word="AGC")
    expect(gpu, EUNSUPPORTED, agc.dc_advance, None, good, word="AGC")
    expect(gpu, EUNSUPPORTED, agc.seek_dc, CALL, frames(NRSC5_DC, araw, 0, CALL), CALL, None, word="AGC")


def test_seek_dc_at_frame_zero_is_a_fresh_chain(gpu):
    kw = dict(CONFIG3_FRONT, **CONFIG3_FILTER)
    raw = dc_stream(6 * CALL + 50_001, kw["input_rate_hz"], kw["in_format"])
    fresh = gpu.Chain(**kw).process(frames(kw, raw, 0, 2 * CALL))
    ch = gpu.Chain(**kw)
    ch.process(frames(kw, raw, 0, 123_457))
    ch.seek_dc(0)
    assert same_bytes(ch.process(frames(kw, raw, 0, 2 * CALL)), fresh)


# --------------------------------------------------------------------------------------------
# 5. the harness: --shards 4 --seamless-dc writes the file --shards 1 writes
# --------------------------------------------------------------------------------------------
ARGS = ["--raw-file-input-rate", "2.4e6", "--raw-file-input-sample-format", "cs16", "--output-rate", "744187.5",
        "--output-sample-format", "cs16", "--freq-shift", "200e3"]


def test_harness_seamless_dc_shards_write_the_single_stream(gpu, tmp_path):
    n, seed = 2_000_003, 41
    one, many = tmp_path / "one.cs16", tmp_path / "many.cs16"
    src = ["--synthetic", str(n), "--synthetic-hash", str(seed), *ARGS, "--dc-block", "--chunk-frames", str(CALL)]
    run(*src, "-o", str(one), "--shards", "1")
    info = run(*src, "-o", str(many), "--shards", "4", "--seamless-dc", "--devices", "1")
    kw = dict(NRSC5_DC)
    pre = -(-p_fir(gpu, kw) // CALL) * CALL
    assert info["seamless_dc"] is True and "seamless" not in info and info["frames_out"] == gpu.design_out_frames(n, **kw)
    for s, ps in enumerate(info["per_shard"]):
        assert ps["first_frame"] == s * (n // 4) // CALL * CALL and ps["frames_out"] == ps["planned_out"]
        assert ps["preroll_frames"] == min(ps["first_frame"], pre)
        assert ps["dc_rows"] == (-(-ps["frames_in"] // CALL) if s < 3 else 0)
    assert os.path.getsize(one) == 4 * info["frames_out"] > 0
    assert filecmp.cmp(one, many, shallow=False)


def test_harness_refuses_seamless_dc_without_the_blocker_or_with_an_agc(gpu):
    base = [EXE, "--synthetic", "2000003", "--synthetic-hash", "1", *ARGS, "--shards", "2", "--seamless-dc", "--chunk-frames", str(CALL)]
    r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode != 0 and "--dc-block" in r.stderr and not r.stdout.strip()
    r = subprocess.run(base + ["--dc-block", "--agc-profile", "digital"], capture_output=True, text=True)
    assert r.returncode != 0 and "AGC" in r.stderr and not r.stdout.strip()


def test_harness_seamless_dc_on_a_chain_without_filter_memory(gpu, tmp_path):
    """a pointwise chain (no resampler, no filter): P_fir = 0, no shard has a preroll, and the last shard enters with the state BEHIND
    the last measured row"""
    n, seed = 1_000_003, 42
    one, many = tmp_path / "one.cf32", tmp_path / "many.cf32"
    src = ["--synthetic", str(n), "--synthetic-hash", str(seed), "--raw-file-input-rate", "2.4e6", "--raw-file-input-sample-format", "cs16",
           "--no-resample", "--output-sample-format", "cf32", "--freq-shift", "100e3", "--dc-block", "--chunk-frames", str(CALL)]
    run(*src, "-o", str(one), "--shards", "1")
    info = run(*src, "-o", str(many), "--shards", "4", "--seamless-dc", "--devices", "1")
    assert [ps["preroll_frames"] for ps in info["per_shard"]] == [0, 0, 0, 0] and info["frames_out"] == n
    assert any(ps["entry"]["re"] != 0.0 for ps in info["per_shard"][1:])
    assert os.path.getsize(one) == 8 * n and filecmp.cmp(one, many, shallow=False)
