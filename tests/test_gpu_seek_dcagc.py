"""Exact seamless range sharding of chains with the DC blocker AND the digital output AGC (include/iqgpu.h, iqgpu_chain_dcagc_*):
the DC maps of a call, one row per piece the ordinary call is cut into; one walk over them; the AGC rows of a range from shadow
calls; the AGC walk; and a chain put at a seam with both states, which continues the stream byte for byte.

The time scaling is test_gpu_seek_agc's: the preset RATIOS at an input rate of 96 kHz put the 2 s lock at 192 000 input frames, so
45 calls of 65 536 frames walk the AGC through scanning, the locking chunk (it starts at frame 196 608 = the first chunk of call 3),
the locked phase, a fade (hang interval, then creep) and a burst that ratchets.  The stream carries a DC offset of 3 % / -2 % of full
scale, and the blocker's alpha at 96 kHz is 6.5e-4: its memory is far longer than any preroll here, so a stale DC state cannot pass
by decay.

The yardstick is always ONE ordinary chain on the same grid, and every comparison is of bytes: no tolerance appears anywhere.  Which
call the ordinary chain cuts is read off the ordinary chain itself: a cut call launches k_dc_scan twice (its profile counts it)."""
import ctypes as C
import filecmp
import json
import os
import subprocess

import numpy as np
import pytest

from iq_tool_amd import synth

from shard_support import ECAPACITY, EINVAL, EUNSUPPORTED, EXE, expect, fr, same, set_switches

pytestmark = pytest.mark.gpu
RATE = 96e3
K = RATE / 2.4e6
CHUNK = 16384
B = 4 * CHUNK
N_CALLS = 45
N = N_CALLS * B
T_FADE, T_BURST, T_BURST_END = 10.0, 24.0, 24.5
LOCK_CALL = 3                                   # the chunk that starts at 196 608 frames = 2.048 s is the first one of call 3
SEAMS = dict(scanning=2 * B, locking_call=3 * B, locked=10 * B, hang=17 * B, creeping=25 * B, behind_ratchet=38 * B)
SWITCHES = ("FORCE_FAT", "FAT", "NO_P0", "NO_S2", "FORCE_GENERIC", "AGC_NOFUSE", "NO_FAST", "NO_CASC2", "MEASURE_ROUTE")

BOTH = dict(input_rate_hz=RATE, dc_block=True, agc=True)
NRSC5 = dict(BOTH, in_format="cs16", out_format="cs16", target_rate_hz=744187.5 * K, shift_hz=200e3 * K)
CU8_NRSC5 = dict(BOTH, in_format="cu8", out_format="cu8", target_rate_hz=1488375.0 * K)
USB = dict(BOTH, in_format="cs16", out_format="cs16", target_rate_hz=744187.5 * K, filters=(("passband", 158.5e3 * K, 113e3 * K),))
AM = dict(BOTH, in_format="cs16", out_format="cs16", target_rate_hz=46511.71875 * K)
INTERP = dict(BOTH, in_format="cs16", out_format="cs16", target_rate_hz=2.4e6 * K * 1.2, shift_hz=150e3 * K)
# name -> (description, IQGPU_<NAME> switches, does the ordinary chain cut the locking call: True / False / None = whatever it does)
# (FORCE_FAT asks for the long-call kernels -- k_front_mid, k_front_p0 -- at these call lengths; with the blocker on the library keeps
#  such chains on k_front_s1, whose fused variant these cases then run: front_kernel() is compared call by call either way)
ROUTINGS = {
    "nrsc5_cs16_mid": (NRSC5, dict(FORCE_FAT="1"), True),
    "cu8_nrsc5_p0": (CU8_NRSC5, dict(FORCE_FAT="1"), True),
    "usb_filter_epilogue": (USB, dict(FORCE_FAT="1"), False),
    "am_cascade": (AM, {}, None),
    "interp": (INTERP, {}, False),
    "agc_nofuse": (NRSC5, dict(AGC_NOFUSE="1"), False),
    "nrsc5_iq_correct": (dict(NRSC5, iq_correct=True, iq_mag=0.02, iq_phase=-0.015), dict(FORCE_FAT="1"), True),
}


_streams = {}


def stream(fmt):
    """test_gpu_seek_agc's envelope over noise, plus a DC offset of 3 % (I) and -2 % (Q) of full scale"""
    if fmt not in _streams:
        raw = synth.raw_stream(N, 2.4e6, 61, "cs16").astype(np.float64).reshape(-1, 2)
        env = np.full(N, 0.5)
        env[int(T_FADE * RATE):] = 0.15
        env[int(T_BURST * RATE):int(T_BURST_END * RATE)] = 0.65
        env[int(T_BURST_END * RATE):] = 0.5
        cs16 = np.clip(np.rint(raw * env[:, None] + np.array([0.03, -0.02]) * 32768.0), -32768, 32767).astype(np.int16).reshape(-1)
        _streams["cs16"] = cs16
        _streams["cu8"] = ((cs16.astype(np.int32) >> 8) + 128).astype(np.uint8)
    return _streams[fmt]


def p_fir(gpu, kw):
    return gpu.design_preroll_frames(**dict(kw, dc_block=False, agc=False))


def pre_calls(gpu, kw):
    return -(-p_fir(gpu, kw) // B)


_single = {}


def single_stream(gpu, name):
    """the yardstick, computed once per routing (under its switches) and left unchanged: one ordinary chain, calls of B frames --
    per call its bytes, front kernel, k_dc_scan launches, and the DC / AGC state behind it"""
    if name not in _single:
        kw = ROUTINGS[name][0]
        x = stream(kw["in_format"])
        ch = gpu.Chain(**kw)
        ch.set_profiling(True)
        r = dict(outs=[], kernels=[], scans=[], dc=[], agc=[])
        for a in range(0, N, B):
            r["outs"].append(ch.process(fr(x, a, a + B)))
            r["kernels"].append(ch.front_kernel())
            r["dc"].append(ch.dc_state().copy())
            r["agc"].append(bytes(ch.agc_state_raw()))
            r["scans"].append(ch.profile()["dc_scan"]["launches"])          # (a reading empties the counters: launches of THIS call)
        _single[name] = r
    return _single[name]


def dc_walk(gpu, kw, x, upto):
    """steps 1 and 2 over [0, upto): the rows per grid call, the first row index of every call, before[]"""
    m = gpu.Chain(**kw)
    per_call = [m.dcagc_dc_measure(a, fr(x, a, a + B)) for a in range(0, upto, B)]
    first_row = np.concatenate([[0], np.cumsum([r.size for r in per_call])]).astype(int)
    st, before = m.dcagc_dc_advance(None, np.concatenate(per_call))
    return per_call, first_row, before, st


def dc_in_front_of(before, first_row, st, k):
    """the walked state in front of grid call k (behind the last row: st)"""
    return before[first_row[k]] if first_row[k] < before.size else st


def seek_to(gpu, kw, x, k, dc_before, first_row, st, entry):
    """a fresh chain put in front of grid call k by the recipe: the preroll is the ceil(P_fir / B) grid calls in front of it"""
    n = min(k, pre_calls(gpu, kw))
    ch = gpu.Chain(**kw)
    ch.dcagc_seek(k * B, fr(x, (k - n) * B, k * B), B, dc_in_front_of(dc_before, first_row, st, k - n), entry)
    return ch


# --------------------------------------------------------------------------------------------
# 1. seams: rows per call, both walked states, and the stream behind the seam
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ROUTINGS))
def test_seams_are_invisible(gpu, monkeypatch, name):
    kw, sw, cuts = ROUTINGS[name]
    set_switches(monkeypatch, SWITCHES, sw)
    x = stream(kw["in_format"])
    one = single_stream(gpu, name)
    last = max(SEAMS.values()) // B
    per_call, first_row, before, st = dc_walk(gpu, kw, x, last * B)

    # one row per piece: two exactly for the call the ordinary chain cuts
    got = [r.size for r in per_call]
    print("%s: rows per call %s; k_dc_scan launches of the ordinary chain %s; kernels %s" % (name, got, one["scans"][:last], sorted(set(one["kernels"]))))
    assert got == one["scans"][:last]
    if cuts is not None:
        assert got == [2 if (cuts and k == LOCK_CALL) else 1 for k in range(last)]
    for k, r in enumerate(per_call):
        assert int(r["frames"].sum()) == B and (r.size == 1 or int(r["frames"][0]) == CHUNK)

    # the DC walk: before[first_row[k]] is the ordinary chain's state behind call k - 1, for EVERY call
    for k in range(1, last + 1):
        assert same(dc_in_front_of(before, first_row, st, k), one["dc"][k - 1]), (name, k)
    assert np.hypot(one["dc"][last - 1]["re"], one["dc"][last - 1]["im"]) > 0.0

    # the AGC rows from shadow calls, walked: the ordinary chain's AGC state behind every call
    g = gpu.Chain(**kw)
    g.dcagc_seek(0)
    fresh = bytes(g.agc_state_raw())
    rows = [g.dcagc_measure(fr(x, a, a + B)) for a in range(0, last * B, B)]
    assert all(r.size == B // CHUNK for r in rows) and bytes(g.agc_state_raw()) == fresh
    entry, entries = g.agc_initial_state(), {}
    for k in range(last):
        entry = g.agc_advance(entry, rows[k])
        assert bytes(entry) == one["agc"][k], (name, k)
        entries[k + 1] = entry
    assert entries[LOCK_CALL].locked == 0 and entries[LOCK_CALL + 1].locked == 1

    # behind every seam: bytes, kernel names, final states
    for what, a in sorted(SEAMS.items(), key=lambda kv: kv[1]):
        k0 = a // B
        ch = seek_to(gpu, kw, x, k0, before, first_row, st, entries[k0])
        assert ch.tell()[0] == a and same(ch.dc_state(), one["dc"][k0 - 1]) and bytes(ch.agc_state_raw()) == one["agc"][k0 - 1]
        differing = 0
        for k in range(k0, N_CALLS):
            out = ch.process(fr(x, k * B, (k + 1) * B))
            assert out.nbytes == one["outs"][k].nbytes and ch.front_kernel() == one["kernels"][k], (name, what, k, ch.front_kernel())
            differing += int((out.view(np.uint8) != one["outs"][k].view(np.uint8)).sum())
        print("%s seam %s (call %d): %d bytes differ behind it" % (name, what, k0, differing))
        assert differing == 0
        assert same(ch.dc_state(), one["dc"][-1]) and bytes(ch.agc_state_raw()) == one["agc"][-1]


# --------------------------------------------------------------------------------------------
# 2. the five steps over four ranges
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nrsc5_cs16_mid", "usb_filter_epilogue"])
def test_four_range_stitch_from_one_pair_of_walks(gpu, monkeypatch, name):
    kw, sw, _ = ROUTINGS[name]
    set_switches(monkeypatch, SWITCHES, sw)
    x = stream(kw["in_format"])
    one = single_stream(gpu, name)
    cuts = [0, 3, 16, 30]                                        # in grid calls: in front of the locking call, in the hang interval, behind the ratchet
    _, first_row, before, st = dc_walk(gpu, kw, x, cuts[-1] * B)                             # steps 1 + 2
    tables = []
    for r, k0 in enumerate(cuts[:-1]):                                                       # step 3
        m = seek_to(gpu, kw, x, k0, before, first_row, st, None)
        tables.append(np.concatenate([m.dcagc_measure(fr(x, k * B, (k + 1) * B)) for k in range(k0, cuts[r + 1])]))
    w = gpu.Chain(**kw)
    entry, entries = w.agc_initial_state(), []
    for r in range(len(cuts)):                                                               # step 4
        entries.append(entry)
        if r < len(tables):
            entry = w.agc_advance(entry, tables[r])
    stitched = []
    for r, k0 in enumerate(cuts):                                                            # step 5
        k1 = cuts[r + 1] if r + 1 < len(cuts) else N_CALLS
        ch = seek_to(gpu, kw, x, k0, before, first_row, st, entries[r])
        stitched += [ch.process(fr(x, k * B, (k + 1) * B)) for k in range(k0, k1)]
    assert same(np.concatenate(stitched), np.concatenate(one["outs"]))
    assert same(ch.dc_state(), one["dc"][-1]) and bytes(ch.agc_state_raw()) == one["agc"][-1]


# --------------------------------------------------------------------------------------------
# 3. shadow calls change nothing they should not
# --------------------------------------------------------------------------------------------
def test_shadow_calls_leave_the_rest_alone(gpu, monkeypatch):
    name = "nrsc5_cs16_mid"
    kw, sw, _ = ROUTINGS[name]
    set_switches(monkeypatch, SWITCHES, sw)
    x = stream(kw["in_format"])
    one = single_stream(gpu, name)
    # a dcagc_dc_measure between ordinary calls: the chain continues byte-identically
    ch = gpu.Chain(**kw)
    for k in range(8):
        ch.dcagc_dc_measure(((k + 5) % 7) * B, fr(x, ((k + 5) % 7) * B, ((k + 5) % 7 + 1) * B))
        assert same(ch.process(fr(x, k * B, (k + 1) * B)), one["outs"][k]), k
    assert same(ch.dc_state(), one["dc"][7]) and bytes(ch.agc_state_raw()) == one["agc"][7]
    # dcagc_measure moves tell() and the DC state as process does and leaves the AGC state as it was
    ref = gpu.Chain(**kw)
    m = gpu.Chain(**kw)
    m.dcagc_seek(0)
    agc0 = bytes(m.agc_state_raw())
    for k in range(6):
        ref.process(fr(x, k * B, (k + 1) * B))
        m.dcagc_measure(fr(x, k * B, (k + 1) * B))
        assert m.tell() == ref.tell() and same(m.dc_state(), ref.dc_state()) and same(m.dc_state(), one["dc"][k])
        assert bytes(m.agc_state_raw()) == agc0
    # probe rules 2 and 3: shadow calls leave no block, the seek drops a held one, the first ordinary call leaves its head
    p = gpu.Chain(**kw)
    p.enable_iq_probe(True)
    p.process(fr(x, 0, B))
    assert p.read_iq_probe() is not None
    p.dcagc_seek(0)
    assert p.read_iq_probe() is None
    p.dcagc_measure(fr(x, 0, B))
    p.dcagc_dc_measure(B, fr(x, B, 2 * B))
    assert p.read_iq_probe() is None
    q = gpu.Chain(**kw)
    q.enable_iq_probe(True)
    q.process(fr(x, 0, B))
    q.read_iq_probe()
    q.process(fr(x, B, 2 * B))
    p.process(fr(x, B, 2 * B))
    blk = p.read_iq_probe()
    assert blk is not None and same(blk, q.read_iq_probe())


# --------------------------------------------------------------------------------------------
# 4. device variants
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lead", [0, 4])
def test_device_variants_at_the_single_streams_alignment(gpu, monkeypatch, lead):
    """every call of the single stream and of the shard starts `lead` bytes past a 16-byte boundary, the same on both sides as the
    header asks; at lead 0 that is the host variants' staging, whose rows and bytes the device variants then give"""
    name = "nrsc5_cs16_mid"
    kw, sw, _ = ROUTINGS[name]
    set_switches(monkeypatch, SWITCHES, sw)
    x = stream("cs16")
    n_calls, k0 = 8, 5
    buf = gpu.DeviceBuffer(n_calls * B * 4 + 64)
    stage = np.zeros(n_calls * B * 4 + 64, np.uint8)
    stage[lead:lead + n_calls * B * 4] = fr(x, 0, n_calls * B).view(np.uint8)
    buf.upload(stage)
    assert buf.ptr % 16 == 0
    at = lambda k: buf.ptr + lead + k * B * 4
    cap = gpu.Chain(**kw).max_out_frames(B) * 4
    out = gpu.DeviceBuffer(cap)

    def run(ch, k):
        got = ch.process_device(at(k), B, out.ptr, cap)
        ch.synchronize()
        return out.download(got * 4).copy()

    ref = gpu.Chain(**kw)
    outs, dcs, agcs = [], [], []
    for k in range(n_calls):
        outs.append(run(ref, k))
        dcs.append(ref.dc_state().copy())
        agcs.append(bytes(ref.agc_state_raw()))
    m = gpu.Chain(**kw)
    per_call = [m.dcagc_dc_measure_device(k * B, at(k), B) for k in range(k0)]
    assert [r.size for r in per_call] == [2 if k == LOCK_CALL else 1 for k in range(k0)]
    first_row = np.concatenate([[0], np.cumsum([r.size for r in per_call])]).astype(int)
    st, before = m.dcagc_dc_advance(None, np.concatenate(per_call))
    assert same(st, dcs[k0 - 1]) and all(same(before[first_row[k]], dcs[k - 1]) for k in range(1, k0))
    g = gpu.Chain(**kw)
    g.dcagc_seek_device(0, 0, 0)
    rows = [g.dcagc_measure_device(at(k), B) for k in range(k0)]
    entry = g.agc_advance(g.agc_initial_state(), np.concatenate(rows))
    assert bytes(entry) == agcs[k0 - 1]
    if lead == 0:
        one = single_stream(gpu, name)
        assert all(same(o, w) for o, w in zip(outs, one["outs"]))
        h = gpu.Chain(**kw)
        h.dcagc_seek(0)
        for k in range(k0):
            assert same(per_call[k], h.dcagc_dc_measure(k * B, fr(x, k * B, (k + 1) * B)))
            assert same(rows[k], h.dcagc_measure(fr(x, k * B, (k + 1) * B)))
    n = min(k0, pre_calls(gpu, kw))
    ch = gpu.Chain(**kw)
    ch.dcagc_seek_device(k0 * B, at(k0 - n), n * B, B, before[first_row[k0 - n]], entry)
    for k in range(k0, n_calls):
        assert same(run(ch, k), outs[k]), (lead, k)
    assert same(ch.dc_state(), dcs[-1]) and bytes(ch.agc_state_raw()) == agcs[-1]
    buf.free(); out.free()


# --------------------------------------------------------------------------------------------
# 5. one definition of the DC walk
# --------------------------------------------------------------------------------------------
def test_dcagc_dc_advance_is_dc_advance(gpu, monkeypatch):
    kw, sw, _ = ROUTINGS["nrsc5_cs16_mid"]
    set_switches(monkeypatch, SWITCHES, sw)
    x = stream("cs16")
    per_call, _, before, st = dc_walk(gpu, kw, x, 6 * B)
    rows = np.concatenate(per_call)
    plain = gpu.Chain(**dict(kw, agc=False))
    st2, before2 = plain.dc_advance(None, rows)
    assert rows.size == 7 and same(st, st2) and same(before, before2)


# --------------------------------------------------------------------------------------------
# 6. errors
# --------------------------------------------------------------------------------------------
def test_errors(gpu, monkeypatch):
    from iq_tool_amd import _lib
    from iq_tool_amd.chain import AGC_ROW, DC_ROW, DC_STATE
    name = "usb_filter_epilogue"                                  # (a chain with filter memory: P_fir > 0)
    kw, sw, _ = ROUTINGS[name]
    set_switches(monkeypatch, SWITCHES, sw)
    x = stream("cs16")
    one = single_stream(gpu, name)
    assert 0 < p_fir(gpu, kw) <= B
    call0, pre = fr(x, 0, B), fr(x, B, 2 * B)
    good = np.zeros(1, DC_ROW)
    good["f"] = 0.5

    def all_calls(ch, code, word):
        expect(gpu, code, ch.dcagc_dc_measure, 0, call0, word=word)
        expect(gpu, code, ch.dcagc_dc_advance, None, good, word=word)
        expect(gpu, code, ch.dcagc_seek, 2 * B, pre, B, None, None, word=word)
        expect(gpu, code, ch.dcagc_measure, call0, word=word)

    # a chain without the blocker, without the AGC; the profiles dx / local and the wall clock
    all_calls(gpu.Chain(**dict(kw, dc_block=False)), EINVAL, "DC blocker")
    all_calls(gpu.Chain(**dict(kw, agc=False)), EINVAL, "AGC")
    all_calls(gpu.Chain(**dict(kw, agc_profile="dx")), EUNSUPPORTED, "dx / local")
    all_calls(gpu.Chain(**dict(kw, agc_profile="local")), EUNSUPPORTED, "dx / local")
    all_calls(gpu.Chain(**dict(kw, agc_clock="wall")), EUNSUPPORTED, "WALL")

    ch = gpu.Chain(**kw)
    lib, h = ch._lib, ch._h
    st, n = _lib.DcState(), C.c_size_t(0)
    buf = call0.ctypes.data_as(C.c_void_p)
    drows, arows = np.zeros(2, DC_ROW), np.zeros(4, AGC_ROW)
    dp, ap = drows.ctypes.data_as(C.c_void_p), arows.ctypes.data_as(C.c_void_p)
    # a refused measure leaves the handle as it was: the chain is two calls into the stream while it is refused
    ch.process(fr(x, 0, B))
    # NULL arguments
    for f in (lib.iqgpu_chain_dcagc_dc_measure, lib.iqgpu_chain_dcagc_dc_measure_device):
        assert f(None, 0, buf, B, dp, 2, C.byref(n)) == EINVAL and f(h, 0, buf, B, None, 2, C.byref(n)) == EINVAL
        assert f(h, 0, buf, B, dp, 2, None) == EINVAL and f(h, 0, None, B, dp, 2, C.byref(n)) == EINVAL
        assert f(h, 0, buf, B, dp, 1, C.byref(n)) == EINVAL                                   # cap < 2
    for f in (lib.iqgpu_chain_dcagc_measure, lib.iqgpu_chain_dcagc_measure_device):
        assert f(None, buf, B, ap, 4, C.byref(n)) == EINVAL and f(h, buf, B, ap, 4, None) == EINVAL
        assert f(h, None, B, ap, 4, C.byref(n)) == EINVAL and f(h, buf, B, None, 4, C.byref(n)) == EINVAL
        assert f(h, buf, B, ap, 3, C.byref(n)) == ECAPACITY                                   # below the chunk count
    assert lib.iqgpu_chain_dcagc_dc_advance(None, C.byref(st), good.ctypes.data_as(C.c_void_p), 1, None) == EINVAL
    assert lib.iqgpu_chain_dcagc_dc_advance(h, None, good.ctypes.data_as(C.c_void_p), 1, None) == EINVAL
    assert lib.iqgpu_chain_dcagc_dc_advance(h, C.byref(st), None, 1, None) == EINVAL
    # positions: beyond 2^39 frames, off the chunk grid
    expect(gpu, EINVAL, ch.dcagc_dc_measure, 1 << 39, call0, word="2^39")
    expect(gpu, EINVAL, ch.dcagc_dc_measure, CHUNK + 4096, call0, word="agc_chunk_frames")
    bad = np.zeros(2, DC_ROW)
    bad["f"] = (0.5, float("nan"))
    expect(gpu, EINVAL, ch.dcagc_dc_advance, None, bad, word="row 1")
    # ... the existing exact calls still refuse this chain
    expect(gpu, EUNSUPPORTED, ch.dc_measure, 0, call0, word="AGC")
    expect(gpu, EUNSUPPORTED, ch.dc_advance, None, good, word="AGC")
    assert same(ch.process(fr(x, B, 2 * B)), one["outs"][1])       # every refusal so far: the handle as it was, one call into the stream
    expect(gpu, EUNSUPPORTED, ch.seek_dc, 2 * B, pre, B, None, word="AGC")

    # refused seeks leave the chain reset
    nan = np.zeros((), DC_STATE)
    nan["re"] = float("nan")
    entry = ch.agc_initial_state()
    entry.locked = 2
    assert lib.iqgpu_chain_dcagc_seek(None, 0, None, 0, 0, None, None) == EINVAL
    assert lib.iqgpu_chain_dcagc_seek_device(None, 0, None, 0, 0, None, None) == EINVAL
    assert lib.iqgpu_chain_dcagc_seek(h, 2 * B, None, B, B, None, None) == EINVAL              # NULL preroll
    for args, word in [((1 << 63, None, 0, None, None), "2^39"),
                       ((2 * B + 4096, fr(x, B + 4096, 2 * B + 4096), 0, None, None), "agc_chunk_frames"),     # first_frame off the grid
                       ((2 * B, pre, 4096 * 4 * 3, None, None), None),                                          # call_frames: not whole calls / off the grid
                       ((2 * B, pre, CHUNK + 8, None, None), None),
                       ((2 * B, fr(x, 2 * B - CHUNK - 8, 2 * B), 0, None, None), "agc_chunk_frames"),           # a preroll off the grid
                       ((2 * B, fr(x, 2 * B - CHUNK, 2 * B)[:0], 0, None, None), "shorter"),                    # shorter than min(first_frame, P_fir)
                       ((2 * B, fr(x, 0, 3 * B), B, None, None), "in front of"),
                       ((2 * B, pre, B, nan, None), "finite"),
                       ((2 * B, pre, B, None, entry), "locked")]:
        ch.process(fr(x, 0, B))
        expect(gpu, EINVAL, ch.dcagc_seek, *args, word=word)
        assert ch.tell() == (0, 0)
        assert same(ch.process(fr(x, 0, B)), one["outs"][0]), args[2:]
        ch.reset()


# --------------------------------------------------------------------------------------------
# 7. the harness
# --------------------------------------------------------------------------------------------
def test_harness_seamless_dc_agc_shards_write_the_single_stream(gpu, tmp_path):
    n, seed = 1_500_003, 43
    one, many = tmp_path / "one.cs16", tmp_path / "many.cs16"
    # (the rates of NRSC5 above: the stream locks at 196 608 frames, inside shard 0, and shards 1 and 2 start behind the lock)
    src = ["--synthetic", str(n), "--synthetic-hash", str(seed), "--raw-file-input-rate", str(RATE), "--raw-file-input-sample-format", "cs16",
           "--output-rate", str(744187.5 * K), "--output-sample-format", "cs16", "--freq-shift", str(200e3 * K), "--dc-block",
           "--agc-profile", "digital", "--chunk-frames", str(B)]

    def run(*args):
        r = subprocess.run([EXE, *src, *args], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr + r.stdout
        return json.loads(r.stdout.strip().splitlines()[-1])

    run("-o", str(one), "--shards", "1")
    info = run("-o", str(many), "--shards", "3", "--seamless-dc-agc", "--devices", "1")
    assert info["seamless_dc_agc"] is True and info["frames_out"] == gpu.design_out_frames(n, **dict(NRSC5, agc=False))
    pre = pre_calls(gpu, NRSC5) * B
    for s, ps in enumerate(info["per_shard"]):
        assert ps["first_frame"] == s * (n // 3) // B * B and ps["frames_out"] == ps["planned_out"]
        assert ps["preroll_frames"] == min(ps["first_frame"], pre)
        calls = -(-ps["frames_in"] // B)
        assert ps["dc_rows"] == ((calls + 1 if s == 0 else calls) if s < 2 else 0)             # the locking call gives two rows
        assert ps["agc_rows"] == (-(-ps["frames_in"] // CHUNK) if s < 2 else 0)
    assert info["per_shard"][1]["entry"]["locked"] == 1 and info["per_shard"][1]["dc_entry"]["re"] != 0.0
    assert os.path.getsize(one) == 4 * info["frames_out"] > 0
    assert filecmp.cmp(one, many, shallow=False)
    # the two older exact modes keep refusing such a chain
    r = subprocess.run([EXE, *src, "--shards", "3", "--seamless-dc"], capture_output=True, text=True)
    assert r.returncode != 0 and "AGC" in r.stderr


# --------------------------------------------------------------------------------------------
# 8. negative control: the comparison can tell the difference
# --------------------------------------------------------------------------------------------
def test_negative_control_seek_agc_meets_the_stream_only_to_the_dc_bound(gpu, monkeypatch):
    """today's route to the same seam -- iqgpu_chain_seek_agc behind its DC warm-up, with the AGC entry walked from
    iqgpu_chain_measure's rows -- is good to the 1e-6 bound, not to the bit: the DC state or at least one output byte differs from the
    single stream's, and the comparisons above would say so"""
    name = "nrsc5_cs16_mid"
    kw, sw, _ = ROUTINGS[name]
    set_switches(monkeypatch, SWITCHES, sw)
    x = stream("cs16")
    one = single_stream(gpu, name)
    k0 = SEAMS["locked"] // B
    m = gpu.Chain(**kw)
    rows = np.concatenate([m.measure(fr(x, k * B, (k + 1) * B)) for k in range(k0)])
    entry = m.agc_advance(m.agc_initial_state(), rows)
    p = min(k0 * B, gpu.design_preroll_frames(**dict(kw, agc=False)))
    ch = gpu.Chain(**kw)
    ch.seek_agc(k0 * B, fr(x, k0 * B - p, k0 * B), entry)
    dc_differs = not same(ch.dc_state(), one["dc"][k0 - 1])
    differing = sum(int((ch.process(fr(x, k * B, (k + 1) * B)).view(np.uint8) != one["outs"][k].view(np.uint8)).sum()) for k in range(k0, k0 + 8))
    print("seek_agc at call %d behind a preroll of %d frames: DC state %s, %d output bytes differ in 8 calls; AGC entry %s" % (
        k0, p, "differs" if dc_differs else "equal", differing, "equal" if bytes(entry) == one["agc"][k0 - 1] else "differs"))
    if not dc_differs and differing == 0:
        pytest.xfail("on this stream the 1e-6 route happens to meet the single stream bit for bit: nothing to tell apart")
    assert dc_differs or differing > 0
