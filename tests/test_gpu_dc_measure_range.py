"""The DC measure pass over a whole range in one call (include/iqgpu.h, iqgpu_chain_*_dc_measure_range): every grid call of a range
planned up front, measured by k_dc_prefix_batch / k_dc_scan_batch in one submission.

The yardstick is always the family's per-call form, looped over the same grid calls IN THE SAME TEST ON THE SAME CHAIN, and every
comparison is of the raw bytes of the rows (f, g_re, g_im, frames): no tolerance appears anywhere.  The per-call kernels and the batch
kernels run one definition of the arithmetic (kernels.hip: dc_prefix_segment, dc_scan_fold), so anything but equality is a bug in the
entry table or in the planning.

Shapes are the smallest that take every path: 65 536-frame calls plus a 12 288-frame tail and 4 096-frame calls on the wave kernels'
segments; the workgroup-tiled route (FORCE_GENERIC: segments of 16 tiles = 32 768 frames) for k_dc_prefix's 4-chunk (16-bit) and
8-chunk (8-bit) load paths, which need segments longer than 5 and 9 chunks of 1024 frames; one call more than a launch holds."""
import ctypes as C

import numpy as np
import pytest

from iq_tool_amd import synth
from iq_tool_amd.chain import DC_ROW

from shard_support import ECAPACITY, EINVAL, EUNSUPPORTED, expect, frames, grid, noise, same, set_switches

pytestmark = pytest.mark.gpu
SWITCHES = ("FORCE_FAT", "FAT", "NO_P0", "NO_S2", "FORCE_GENERIC", "NO_FAST", "NO_FAT", "NO_CASC2", "AGC_NOFUSE", "MEASURE_ROUTE",
            "DC_RANGE_SLICE_FRAMES")
RATE = 2.4e6
NRSC5_DC = dict(in_format="cs16", out_format="cs16", input_rate_hz=RATE, target_rate_hz=744187.5, shift_hz=200e3, dc_block=True)
CU8_NRSC5_DC = dict(in_format="cu8", out_format="cu8", input_rate_hz=RATE, target_rate_hz=1488375.0, dc_block=True)
CF32_POINTWISE_DC = dict(in_format="cf32", out_format="cs16", input_rate_hz=RATE, no_resample=True, shift_hz=100e3, dc_block=True)
# name -> (description, IQGPU_<NAME> switches)
DC_CHAINS = {
    "nrsc5_cs16_wave": (NRSC5_DC, {}),                            # a decimating chain on the wave kernels' runs
    "cu8_nrsc5_no_halfband": (CU8_NRSC5_DC, {}),                  # no half-band stage: 256-frame tiles
    "cf32_pointwise": (CF32_POINTWISE_DC, {}),                    # no_resample: the workgroup-tiled k_front's blocks
    "nrsc5_cs16_generic": (NRSC5_DC, dict(FORCE_GENERIC="1")),    # 32 768-frame segments: the 4-chunk load path
    "cu8_nrsc5_generic": (CU8_NRSC5_DC, dict(FORCE_GENERIC="1")),   # ... and the 8-chunk one
}
# (call_frames, frames of the range): 6 whole calls and a short last one; 40 tiny calls
GRIDS = {"64k_tail": (65536, 6 * 65536 + 12288), "4k_x40": (4096, 40 * 4096)}

_inputs = {}


def stream(fmt, n, seed=11):
    """shard_support.noise (cf32: its 16-bit values scaled to +-1) -- computed once per (format, length), left unchanged"""
    key = (fmt, n, seed)
    if key not in _inputs:
        x = noise(n, "cu8" if fmt == "cu8" else "cs16", seed)
        _inputs[key] = (x.astype(np.float32) / np.float32(32768.0)) if fmt == "cf32" else x
        _inputs[key].setflags(write=False)
    return _inputs[key]


def loop(measure, kw, x, first, n, c):
    """the per-call form over the grid calls of stream frames [first, first + n): x holds the range; (rows, first_row)"""
    per_call = [np.atleast_1d(measure(first + p, frames(kw, x, p, q))) for p, q in grid(0, n, c)]
    first_row = np.concatenate([[0], np.cumsum([r.size for r in per_call])])[:-1]
    return np.concatenate(per_call), first_row.astype(np.uint32)


def check_equal(got, want, what):
    rows, first_row = got
    want_rows, want_first = want
    print("%s: %d rows of %d calls; f[0] %.17g g[0] %.9g %+.9gi" % (what, rows.size, first_row.size, want_rows["f"][0], want_rows["g_re"][0],
                                                                    want_rows["g_im"][0]))
    assert rows.dtype == DC_ROW and rows.size == want_rows.size and same(rows, want_rows), what
    assert first_row.dtype == np.uint32 and same(first_row, want_first), what


# --------------------------------------------------------------------------------------------
# 1. the Dc family: formats, routes, grids, stream positions
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first_calls", [0, 3])
@pytest.mark.parametrize("grid_name", sorted(GRIDS))
@pytest.mark.parametrize("name", sorted(DC_CHAINS))
def test_dc_rows_equal_the_per_call_loops(gpu, monkeypatch, name, grid_name, first_calls):
    kw, sw = DC_CHAINS[name]
    set_switches(monkeypatch, SWITCHES, sw)
    c, n = GRIDS[grid_name]
    first = first_calls * c                                       # (a non-zero stream position changes rem0 in the geometry)
    x = stream(kw["in_format"], n)
    ch = gpu.Chain(**kw)
    want = loop(ch.dc_measure, kw, x, first, n, c)
    assert want[0].size == -(-n // c) and int(want[0]["frames"][-1]) == n - (n - 1) // c * c
    check_equal(ch.dc_measure_range(first, x, c), want, "%s %s first %d" % (name, grid_name, first))
    assert np.all(want[0]["f"] > 0.0) and np.all(want[0]["f"] < 1.0) and np.any(want[0]["g_re"] != 0.0)


def test_more_calls_than_one_launch_holds(gpu, monkeypatch):
    set_switches(monkeypatch, SWITCHES, {})
    cap = gpu.load().iqgpu_dc_measure_range_launch_entries()
    c, calls = 4096, cap + 1
    x = stream("cs16", calls * c, seed=12)
    ch = gpu.Chain(**NRSC5_DC)
    want = loop(ch.dc_measure, NRSC5_DC, x, 0, calls * c, c)
    got = ch.dc_measure_range(0, x, c)
    assert got[0].size == cap + 1
    check_equal(got, want, "%d calls, %d entries per launch" % (calls, cap))


# --------------------------------------------------------------------------------------------
# 2. the _device variants: every call's alignment is taken from its own address
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lead", [0, 4])
def test_device_variant_equals_the_per_call_device_loop_on_the_same_addresses(gpu, monkeypatch, lead):
    """lead 0: the base 16-byte aligned; lead 4: one cs16 frame past a boundary -- raw_aligned = 0 in every call's plan, k_dc_prefix's
    unaligned paths and the segmentation that goes with them"""
    set_switches(monkeypatch, SWITCHES, {})
    kw = NRSC5_DC
    c, n = 65536, 3 * 65536 + 12288
    x = stream("cs16", n)
    buf = gpu.DeviceBuffer(n * 4 + 64)
    stage = np.zeros(n * 4 + 64, np.uint8)
    stage[lead:lead + n * 4] = frames(kw, x, 0, n)
    buf.upload(stage)
    assert buf.ptr % 16 == 0
    base = buf.ptr + lead
    ch = gpu.Chain(**kw)
    for first in (0, 3 * c):
        per_call = [ch.dc_measure_device(first + p, base + p * 4, q - p).reshape(1) for p, q in grid(0, n, c)]
        want = (np.concatenate(per_call), np.arange(len(per_call), dtype=np.uint32))
        check_equal(ch.dc_measure_range_device(first, base, n, c), want, "lead %d first %d" % (lead, first))
    if lead == 0:
        check_equal(ch.dc_measure_range(0, x, c), want if first == 0 else loop(ch.dc_measure, kw, x, 0, n, c), "host form, aligned staging")
    buf.free()


# --------------------------------------------------------------------------------------------
# 3. DcAgc: one row per piece; DcRms: one row per call
# --------------------------------------------------------------------------------------------
K = 96e3 / 2.4e6                                                  # test_gpu_seek_dcagc's time scaling: the 2 s lock near input frame 196 608
B = 65536
LOCK_CALL = 3
BOTH = dict(input_rate_hz=96e3, dc_block=True, agc=True)
NRSC5_BOTH = dict(BOTH, in_format="cs16", out_format="cs16", target_rate_hz=744187.5 * K, shift_hz=200e3 * K)
USB_BOTH = dict(BOTH, in_format="cs16", out_format="cs16", target_rate_hz=744187.5 * K, filters=(("passband", 158.5e3 * K, 113e3 * K),))
N_AGC = 8 * B


def agc_stream():
    """noise at half scale with a DC offset of 3 % / -2 % of full scale (the offset of test_gpu_seek_dcagc's stream)"""
    key = ("dcagc", N_AGC)
    if key not in _inputs:
        raw = synth.raw_stream(N_AGC, 2.4e6, 61, "cs16").astype(np.float64).reshape(-1, 2)
        _inputs[key] = np.clip(np.rint(raw * 0.5 + np.array([0.03, -0.02]) * 32768.0), -32768, 32767).astype(np.int16).reshape(-1)
        _inputs[key].setflags(write=False)
    return _inputs[key]


@pytest.mark.parametrize("name,kw,cuts", [("nrsc5", NRSC5_BOTH, True), ("usb_filter", USB_BOTH, False)])
def test_dcagc_rows_are_the_per_call_loops_one_row_per_piece(gpu, monkeypatch, name, kw, cuts):
    set_switches(monkeypatch, SWITCHES, dict(FORCE_FAT="1"))
    x = agc_stream()
    ch = gpu.Chain(**kw)
    # from 0 across the locking call
    n = 6 * B
    want = loop(ch.dcagc_dc_measure, kw, x, 0, n, B)
    rows, first_row = ch.dcagc_dc_measure_range(0, frames(kw, x, 0, n), B)
    check_equal((rows, first_row), want, name + " across the lock")
    per_call = np.diff(np.concatenate([first_row, [rows.size]]))
    print("%s: rows per call %s" % (name, per_call.tolist()))
    assert per_call.tolist() == [2 if (cuts and k == LOCK_CALL) else 1 for k in range(6)]
    if cuts:
        a = first_row[LOCK_CALL]
        assert int(rows["frames"][a]) + int(rows["frames"][a + 1]) == B and int(rows["frames"][a]) % 16384 == 0
    # a range that starts behind the lock, with a short last call
    first, n = 5 * B, 2 * B + 16384
    tail = frames(kw, x, first, first + n)
    want = loop(ch.dcagc_dc_measure, kw, tail, first, n, B)
    got = ch.dcagc_dc_measure_range(first, tail, B)
    check_equal(got, want, name + " behind the lock")
    assert got[0].size == 3


def test_dcrms_rows_equal_the_per_call_loop(gpu, monkeypatch):
    set_switches(monkeypatch, SWITCHES, {})
    kw = dict(in_format="cs16", out_format="cs16", input_rate_hz=RATE, target_rate_hz=744187.5, shift_hz=200e3, dc_block=True, agc=True,
              agc_profile="local")                                # test_gpu_seek_dcrms's local_decim
    c, n = 65536, 5 * 65536 + 12288
    x = stream("cs16", n, seed=13)
    ch = gpu.Chain(**kw)
    for first in (0, 2 * c):
        check_equal(ch.dcrms_dc_measure_range(first, x, c), loop(ch.dcrms_dc_measure, kw, x, first, n, c), "local_decim first %d" % first)


# --------------------------------------------------------------------------------------------
# 4. end to end: the range form's rows through the walk, against the single stream
# --------------------------------------------------------------------------------------------
def test_dc_walk_over_range_rows_meets_the_single_stream(gpu, monkeypatch):
    set_switches(monkeypatch, SWITCHES, {})
    kw, c, n = NRSC5_DC, 65536, 6 * 65536 + 12288
    x = stream("cs16", n)
    m = gpu.Chain(**kw)
    rows, first_row = m.dc_measure_range(0, x, c)
    st, before = m.dc_advance(None, rows)
    st2, before2 = m.dc_advance(None, loop(m.dc_measure, kw, x, 0, n, c)[0])
    assert same(before, before2) and same(st, st2)
    one = gpu.Chain(**kw)
    for k, (p, q) in enumerate(grid(0, n, c)):
        one.process(frames(kw, x, p, q))
        if k + 1 in (2, 5):                                       # two cuts: the state in front of grid calls 2 and 5
            assert same(one.dc_state(), before[first_row[k + 1]]), k
    assert same(one.dc_state(), st) and np.hypot(st["re"], st["im"]) > 0.0


def test_dcagc_walk_over_range_rows_meets_the_single_stream(gpu, monkeypatch):
    set_switches(monkeypatch, SWITCHES, dict(FORCE_FAT="1"))
    kw, n = NRSC5_BOTH, 6 * B
    x = agc_stream()
    m = gpu.Chain(**kw)
    rows, first_row = m.dcagc_dc_measure_range(0, frames(kw, x, 0, n), B)
    st, before = m.dcagc_dc_advance(None, rows)
    st2, before2 = m.dcagc_dc_advance(None, loop(m.dcagc_dc_measure, kw, x, 0, n, B)[0])
    assert same(before, before2) and same(st, st2)
    one = gpu.Chain(**kw)
    for k in range(6):
        one.process(frames(kw, x, k * B, (k + 1) * B))
        if k + 1 in (LOCK_CALL, LOCK_CALL + 1):                   # in front of the call the stream cuts, and behind it
            assert same(one.dc_state(), before[first_row[k + 1]]), k
    assert same(one.dc_state(), st)


# --------------------------------------------------------------------------------------------
# 5. the handle is untouched
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True])
def test_the_handle_is_left_exactly_as_it_was(gpu, monkeypatch, device):
    set_switches(monkeypatch, SWITCHES, {})
    kw, c, n = NRSC5_DC, 65536, 4 * 65536
    x = stream("cs16", n)
    ch, twin = gpu.Chain(**kw), gpu.Chain(**kw)
    for k in range(2):
        assert same(ch.process(frames(kw, x, k * c, (k + 1) * c)), twin.process(frames(kw, x, k * c, (k + 1) * c)))
    was = (ch.tell(), ch.dc_state().copy(), ch.save_state())
    if device:
        buf = gpu.DeviceBuffer(n * 4)
        buf.upload(frames(kw, x, 0, n))
        rows, _ = ch.dc_measure_range_device(0, buf.ptr, n, c)
        buf.free()
    else:
        rows, _ = ch.dc_measure_range(0, x, c)
    assert rows.size == 4
    assert ch.tell() == was[0] == (2 * c, twin.tell()[1]) and same(ch.dc_state(), was[1]) and bytes(ch.save_state()) == bytes(was[2])
    assert same(ch.process(frames(kw, x, 2 * c, 3 * c)), twin.process(frames(kw, x, 2 * c, 3 * c)))
    assert same(ch.dc_state(), twin.dc_state())


# --------------------------------------------------------------------------------------------
# 6. the host variants: more than one staging slice
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slice_frames,c", [(262144, 65536), (4096, 65536)])
def test_host_variant_over_several_staging_slices(gpu, monkeypatch, slice_frames, c):
    """the slice is a diagnostic switch (dc_range_slice_frames; 2^24 frames by default), taken by the chain when it is created: 262 144
    frames -- four calls a slice, five slices, the last one short -- and a slice below one call, which holds one call"""
    set_switches(monkeypatch, SWITCHES, dict(DC_RANGE_SLICE_FRAMES=str(slice_frames)))
    kw, n = NRSC5_DC, 16 * 65536 + 12288
    x = stream("cs16", n, seed=14)
    ch = gpu.Chain(**kw)
    assert gpu._lib.debug_switches().get("dc_range_slice_frames") == str(slice_frames)
    want = loop(ch.dc_measure, kw, x, 0, n, c)
    check_equal(ch.dc_measure_range(0, x, c), want, "slices of %d frames" % slice_frames)
    check_equal(ch.dc_measure_range(2 * c, x, c), loop(ch.dc_measure, kw, x, 2 * c, n, c), "again, the staging buffers reused")


# --------------------------------------------------------------------------------------------
# 7. errors
# --------------------------------------------------------------------------------------------
def test_every_family_keeps_its_refusals_under_the_new_names(gpu, monkeypatch):
    set_switches(monkeypatch, SWITCHES, {})
    x = stream("cs16", 2 * 65536)
    plain = dict(in_format="cs16", out_format="cs16", input_rate_hz=RATE, target_rate_hz=744187.5)
    digital = gpu.Chain(**dict(plain, dc_block=True, agc=True))
    local = gpu.Chain(**dict(plain, dc_block=True, agc=True, agc_profile="local"))
    no_dc, no_dc_agc = gpu.Chain(**plain), gpu.Chain(**dict(plain, agc=True))
    expect(gpu, EUNSUPPORTED, digital.dc_measure_range, 0, x, 65536, word="iqgpu_chain_dc_measure_range:")
    expect(gpu, EUNSUPPORTED, local.dc_measure_range, 0, x, 65536, word="output AGC")
    expect(gpu, EUNSUPPORTED, local.dcagc_dc_measure_range, 0, x, 65536, word="iqgpu_chain_dcagc_dc_measure_range:")
    expect(gpu, EUNSUPPORTED, digital.dcrms_dc_measure_range, 0, x, 65536, word="iqgpu_chain_dcrms_dc_measure_range:")
    expect(gpu, EINVAL, no_dc.dc_measure_range, 0, x, 65536, word="no DC blocker")
    expect(gpu, EINVAL, no_dc_agc.dcagc_dc_measure_range, 0, x, 65536, word="no DC blocker")
    expect(gpu, EINVAL, no_dc_agc.dcrms_dc_measure_range, 0, x, 65536, word="no DC blocker")
    buf = gpu.DeviceBuffer(x.nbytes)
    expect(gpu, EUNSUPPORTED, digital.dc_measure_range_device, 0, buf.ptr, 2 * 65536, 65536, word="iqgpu_chain_dc_measure_range:")
    buf.free()


def test_arguments_off_the_contract_are_refused_and_leave_the_handle_alone(gpu, monkeypatch):
    set_switches(monkeypatch, SWITCHES, {})
    kw, c = NRSC5_DC, 65536
    x = stream("cs16", 2 * c)
    ch = gpu.Chain(**kw)
    ch.process(frames(kw, x, 0, c))
    was = (ch.tell(), ch.dc_state().copy(), ch.save_state())
    expect(gpu, EINVAL, ch.dc_measure_range, 0, x, 0, word="4096")                         # call_frames 0
    expect(gpu, EINVAL, ch.dc_measure_range, 0, x, 4096 + 2048, word="4096")               # not a multiple of 4096
    expect(gpu, EINVAL, ch.dc_measure_range, c + 4096, x, c, word="grid")                  # first_frame off the grid
    expect(gpu, EINVAL, ch.dc_measure_range, 1 << 39, x, c, word="2^39")                   # a position beyond 2^39
    both = gpu.Chain(**dict(kw, agc=True, agc_chunk_frames=16384))
    expect(gpu, EINVAL, both.dcagc_dc_measure_range, 0, x, 4096, word="agc_chunk_frames")  # DcAgc: off the chunk grid
    expect(gpu, EINVAL, both.dcagc_dc_measure_range, 1 << 39, x, c, word="2^39")

    lib = gpu.load()
    raw = np.ascontiguousarray(x)
    rows, got, first = np.zeros(4, DC_ROW), C.c_size_t(0), np.zeros(4, np.uint32)
    args = lambda cap, r=rows: (ch._h, 0, raw.ctypes.data_as(C.c_void_p), 2 * c, c, r.ctypes.data_as(C.c_void_p) if r is not None else None, cap)
    assert lib.iqgpu_chain_dc_measure_range(*args(1), C.byref(got), first.ctypes.data_as(C.c_void_p)) == ECAPACITY    # cap one too small
    assert got.value == 2 and b"iqgpu_chain_dc_measure_range:" in lib.iqgpu_last_error()
    assert not rows.tobytes().strip(b"\0")                                                  # ... and nothing was written
    assert lib.iqgpu_chain_dc_measure_range(*args(2), C.byref(got), None) == 0 and got.value == 2                     # first_row may be NULL
    assert lib.iqgpu_chain_dc_measure_range(*args(2, None), C.byref(got), None) == EINVAL                              # NULL rows
    assert lib.iqgpu_chain_dc_measure_range(*args(2), None, None) == EINVAL                                            # NULL n_rows
    assert lib.iqgpu_chain_dc_measure_range(ch._h, 0, None, 2 * c, c, rows.ctypes.data_as(C.c_void_p), 4, C.byref(got), None) == EINVAL
    # no frames: no rows, no error -- through every family's wrapper
    for fn in (ch.dc_measure_range, both.dcagc_dc_measure_range):
        r, f = fn(0, np.empty(0, np.int16), c)
        assert r.size == 0 and f.size == 0
    assert ch.tell() == was[0] and same(ch.dc_state(), was[1]) and bytes(ch.save_state()) == bytes(was[2])
    check = ch.dc_measure_range(c, frames(kw, x, c, 2 * c), c)                              # and the chain still measures
    assert same(check[0], np.atleast_1d(ch.dc_measure(c, frames(kw, x, c, 2 * c))))
