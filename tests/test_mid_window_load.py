"""k_front_mid (front_mid.hip) against k_front_s1 on calls that the size rule itself hands to k_front_mid.

Every case processes one seeded stream twice -- as the plan chooses (k_front_mid, asserted through front_kernel()) and with
IQGPU_NO_FAT=1 in the environment, which the package forwards as iqgpu_debug_set("no_fat", "1") when the chain is made (k_front_s1:
the switch front_mid_select honours) -- and asks for equal bytes and equal frame counts
per call: k_front_mid does the same products in the same order, however it fetches its frames and however long it holds its NCO
phasors.  The calls are the shortest the plan still gives to k_front_mid (found by asking front_kernel(), once per session), so at
256 CUs a wave runs about six 768-frame tiles and the launch is mostly run starts, warm-up tiles and edge-wave hand-overs."""
import ctypes as C

import numpy as np
import pytest

RATE = 2.4e6
NRSC5 = dict(in_format="cs16", out_format="cs16", input_rate_hz=RATE, target_rate_hz=744187.5, shift_hz=200e3)
TAIL = 1235            # every call length is the crossover plus an odd tail: no multiple of 768 or of 12
LANE = np.arange(64, dtype=np.int64)
HELD = np.concatenate([4 * LANE + 256 * c + s for c in range(3) for s in (0, 2)] + [12 * LANE - 19 + 2 * i for i in range(6)])

_cache, _streams = {}, {}


def mid_min_frames(gpu):
    """the shortest call of the headline chain that front_kernel() reports on k_front_mid: the size rule is a whole number of
    768-frame tiles for each of 12 waves on every CU, so multiples of 768 * 12 * 6 between 2^23 and 2^24 are bisected"""
    if "n" not in _cache:
        unit = 768 * 12 * 6

        def on_mid(k):
            ch = gpu.Chain(**NRSC5)
            ch.process(np.zeros(2 * unit * k, np.int16))
            return ch.front_kernel().startswith("k_front_mid<6,")

        lo, hi = (1 << 23) // unit, (1 << 24) // unit + 1
        assert not on_mid(lo) and on_mid(hi), "the crossover is not between 2^23 and 2^24 frames"
        while hi - lo > 1:
            m = (lo + hi) // 2
            lo, hi = (lo, m) if on_mid(m) else (m, hi)
        _cache["n"] = unit * hi
    return _cache["n"]


def stream(n, fmt, seed):
    """n frames of seeded noise at a quarter of full scale (nothing saturates), as the raw format's component type"""
    key = (n, fmt, seed)
    if key not in _streams:
        rng = np.random.default_rng(seed)
        if fmt == "cs16":
            raw = rng.integers(-8192, 8192, 2 * n, dtype=np.int16)
        elif fmt == "cs8":
            raw = rng.integers(-32, 32, 2 * n, dtype=np.int8)
        else:
            raw = rng.integers(96, 160, 2 * n, dtype=np.uint8)
        raw.setflags(write=False)
        _streams.clear()                                  # (one stream alive at a time: the tests of a seed run in a row)
        _streams[key] = raw
    return _streams[key]


def run_calls(gpu, monkeypatch, kw, raw, splits, s1, then_reset=False, want_agc=False):
    """the stream through one chain in calls of `splits` frames (then, after reset(), the first call again):
    ([output of each call], [kernel of each call], AGC state)"""
    if s1:
        monkeypatch.setenv("IQGPU_NO_FAT", "1")
    else:
        monkeypatch.delenv("IQGPU_NO_FAT", raising=False)
    try:
        ch = gpu.Chain(**kw)
        outs, names, pos = [], [], 0
        for k in splits:
            outs.append(ch.process(raw[2 * pos:2 * (pos + k)])); pos += k
            names.append(ch.front_kernel())
        if then_reset:
            ch.reset()
            outs.append(ch.process(raw[:2 * splits[0]]))
            names.append(ch.front_kernel())
        return outs, names, (ch.agc_state() if want_agc else None)
    finally:
        monkeypatch.delenv("IQGPU_NO_FAT", raising=False)


def both_kernels_agree(gpu, monkeypatch, kw, raw, splits, **how):
    got, names, st = run_calls(gpu, monkeypatch, kw, raw, splits, False, **how)
    ref, names_ref, st_ref = run_calls(gpu, monkeypatch, kw, raw, splits, True, **how)
    assert all(nm.startswith("k_front_mid<6,") for nm in names), names
    assert all(nm == "k_front_s1" for nm in names_ref), names_ref
    for i, (g, r) in enumerate(zip(got, ref)):
        assert g.size == r.size, (i, g.size, r.size)
        assert np.array_equal(g, r), (i, int((g != r).sum()), int(np.flatnonzero(g != r)[0]))
    assert st == st_ref, (st, st_ref)
    return names


def _chooser():
    from iq_tool_amd import _lib
    f = getattr(C.CDLL(_lib.LIB_PATH), "_ZN5iqgpu22front_mid_nco_hold_allEji")
    f.argtypes = [C.c_uint32, C.c_int]; f.restype = C.c_int
    return f


def arcs_cover(dth):
    """front_mid_nco_hold_all's measure (the instantiations that hold all twelve phasors of a lane, the headline's among them): the share of tile positions at which one of a wave's 768 held phases crosses a cell edge"""
    d = abs((768 * dth + 2 ** 31) % 2 ** 32 - 2 ** 31)
    p = np.sort((HELD * dth) & 0x3fffff)
    gaps = np.diff(np.concatenate([p, [p[0] + (1 << 22)]]))
    return float(np.minimum(gaps, d).sum()) / (1 << 22)


@pytest.mark.gpu
def test_headline_chain_whole_ragged_and_after_reset(gpu, monkeypatch):
    """cs16 -> cs16 at +200 kHz: the whole stream in one call, and three calls in a row, each the crossover length plus a different odd tail (the history one call
    leaves is what the next one's edge waves and first runs start from), then the same chain again after reset()."""
    n = mid_min_frames(gpu)
    # (whole 16-byte words per call -- a call that starts inside one is all edge tiles to the plan and stays on k_front_s1 -- but no
    #  multiple of 12 or of 768 frames)
    splits = [n + 1240, n + 1556, n + 2324]
    raw = stream(sum(splits), "cs16", 201)
    names = both_kernels_agree(gpu, monkeypatch, NRSC5, raw, splits, then_reset=True)
    assert names == ["k_front_mid<6,nco>"] * 4
    # ... and the stream as ONE call on k_front_mid gives the bytes of its three calls in a row
    whole, names, _ = run_calls(gpu, monkeypatch, NRSC5, raw, [sum(splits)], False)
    parts, _, _ = run_calls(gpu, monkeypatch, NRSC5, raw, splits, False)
    assert names == ["k_front_mid<6,nco>"]
    parts = np.concatenate(parts)
    assert whole[0].size == parts.size
    assert np.array_equal(whole[0], parts), int((whole[0] != parts).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("shift,held", [(200000.14, 0), (200000.12, 1), (-199999.90, 1)])
def test_shifts_around_the_hold_threshold(gpu, oracle, monkeypatch, shift, held):
    """The hold is off at 200 000.14 Hz (a tile moves the phases by 204 800: 30 % of the tiles would look up), on at the shift one
    float32 step below (155 648: 22 %, the last one inside the quarter) and on at -199 999.90 Hz, where the phases move DOWN by
    139 264 a tile (hold_d < 0) and the mixer runs conjugated."""
    dth = int(oracle.Nco(np.float32(2 * np.pi * abs(shift) / RATE)).dtheta_u32)
    d = (768 * dth + 2 ** 31) % 2 ** 32 - 2 ** 31
    assert _chooser()(dth, 6) == held
    cover = arcs_cover(dth)
    assert (0.2 < cover <= 0.25 if shift == 200000.12 else 0.25 < cover < 0.3 if not held else cover <= 0.25), cover
    assert (d < 0) == (shift < 0)
    n = mid_min_frames(gpu) + TAIL
    both_kernels_agree(gpu, monkeypatch, dict(NRSC5, shift_hz=shift), stream(n, "cs16", 202), [n])


@pytest.mark.gpu
@pytest.mark.parametrize("name,fmt,kw,kernel", [
    ("nonco", "cs16", dict(shift_hz=0.0), "k_front_mid<6,nonco>"),
    ("cu8-cu8", "cu8", dict(in_format="cu8", out_format="cu8"), "k_front_mid<6,nco,8bit>"),
    ("cs8-cs16", "cs8", dict(in_format="cs8"), "k_front_mid<6,nco,8bit>"),
    ("gain", "cs16", dict(gain=0.5), "k_front_mid<6,nco,gain>"),
    ("cf32-filter", "cs16", dict(filters=(("passband", 158.5e3, 113e3),)), "k_front_mid<6,nco,cf32>"),
    ("second-step-class", "cs16", dict(target_rate_hz=696000.0, shift_hz=-150e3), "k_front_mid<6,nco>"),     # step / 2^24 = 1.724: L3 = 5
])
def test_every_shape_of_six_per_lane(gpu, monkeypatch, name, fmt, kw, kernel):
    """no mixer, 8-bit frames on either side, 16-bit frames with a gain (normalised at the unpack), cf32 out to a band-pass behind
    the resampler, and the second step class (floor(3 step / 2^24) = 5)"""
    n = mid_min_frames(gpu) + TAIL
    names = both_kernels_agree(gpu, monkeypatch, dict(NRSC5, **kw), stream(n, fmt, 203), [n])
    assert names == [kernel]


@pytest.mark.gpu
def test_fused_agc_with_chunk_boundaries_inside_the_call(gpu, monkeypatch):
    """The digital AGC locks during the first call (3 s of a steady level, whichever kernels that takes); the second call runs the
    locked phase fused into the front kernel, with chunks of 5000 frames -- no multiple of the tile, a boundary every six or seven
    tiles: equal bytes, equal AGC state."""
    splits = [7_200_000, mid_min_frames(gpu) + 1556]
    kw = dict(NRSC5, agc=True, agc_chunk_frames=5000)
    raw = stream(sum(splits), "cs16", 204)
    got, names, st = run_calls(gpu, monkeypatch, kw, raw, splits, False, want_agc=True)
    ref, names_ref, st_ref = run_calls(gpu, monkeypatch, kw, raw, splits, True, want_agc=True)
    assert names[1] == "k_front_mid<6,nco>", names          # (cs16 straight out of the front kernel: the gain is applied in it)
    assert names_ref[1] == "k_front_s1", names_ref
    assert st["locked"] and st == st_ref, (st, st_ref)
    for g, r in zip(got, ref):
        assert g.size == r.size
        assert np.array_equal(g, r), int((g != r).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("off", [0, 4, 8])
def test_input_pointer_off_the_sixteen_byte_grid(gpu, off):
    """A device input that starts 4 or 8 bytes behind a 16-byte boundary.  k_front_mid's even stream comes in through coalesced
    16-byte loads, which need that grid: the plan counts such a call as all edge tiles and keeps it on k_front_s1 (plan.cpp) -- the
    same bytes as the aligned call on k_front_mid all the same.  (A kernel that fetches its frames without that rule changes the
    name asserted here, nothing else.)"""
    from iq_tool_amd.chain import DeviceBuffer
    n = mid_min_frames(gpu) + TAIL
    raw = stream(n, "cs16", 205)
    if "aligned" not in _cache:
        ch = gpu.Chain(**NRSC5)
        _cache["aligned"] = ch.process(raw).view(np.uint8)
        assert ch.front_kernel() == "k_front_mid<6,nco>"
    ref = _cache["aligned"]
    d_in = DeviceBuffer(4 * n + 16)
    assert d_in.ptr % 16 == 0
    d_in.upload(np.concatenate([np.zeros(off // 2, np.int16), raw]))
    ch = gpu.Chain(**NRSC5)
    cap = (ch.next_out_frames(n) + 1) * 4
    d_out = DeviceBuffer(cap)
    got = ch.process_device(d_in.ptr + off, n, d_out.ptr, cap)
    ch.synchronize()
    assert ch.front_kernel() == ("k_front_mid<6,nco>" if off == 0 else "k_front_s1")
    out = d_out.download(4 * got).copy()
    d_out.free(); d_in.free()
    assert out.size == ref.size
    assert np.array_equal(out, ref), int((out != ref).sum())
