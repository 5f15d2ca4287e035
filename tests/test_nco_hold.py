"""The NCO phasor hold of k_front_mid (front_mid.hip run_mid, front_mid_nco_hold).

A phasor is table entry (theta + 2^21) >> 22 of the 1024-entry table, and from one 768-frame tile to the next every phase of a wave
moves by the same D = 768 dtheta (mod 2^32).  k_front_mid looks the odd stream's six phasors per lane up only on the tiles where one
of the wave's indices moves and holds them otherwise; nco_hold=0 (IQGPU_NCO_HOLD=0) looks them up on every tile.  The CPU tests
restate the refresh schedule in numpy -- it is why the hold pays on the shifts of the 3.125 kHz grid -- and check the chain's
chooser against it; the GPU tests check that the hold changes no byte."""
import ctypes as C

import numpy as np
import pytest

from iq_tool_amd import synth

RATE = 2.4e6
NRSC5 = dict(in_format="cs16", out_format="cs16", input_rate_hz=RATE, target_rate_hz=744187.5, shift_hz=200e3)
LANE = np.arange(64, dtype=np.int64)
# the frames of a tile whose phasors k_front_mid looks up (6 per lane): even stream 4 lane + 256 c + {0, 2}, odd stream 12 lane - 19 + 2 i
EVEN = np.concatenate([4 * LANE + 256 * c + s for c in range(3) for s in (0, 2)])
ODD = np.concatenate([12 * LANE - 19 + 2 * i for i in range(6)])


def dtheta(oracle, shift_hz):
    return int(oracle.Nco(np.float32(2 * np.pi * abs(shift_hz) / RATE)).dtheta_u32)


def per_tile_advance(dth):
    """D = 768 dtheta mod 2^32 as a signed 32-bit value"""
    return (768 * dth + 2 ** 31) % 2 ** 32 - 2 ** 31


def tiles_with_a_change(dth, frames, n_tiles=2000, t0=0, theta0=0):
    """how many of tiles t0 + 1 .. t0 + n_tiles - 1 see a table index of `frames` differ from the tile before"""
    T = np.arange(t0, t0 + n_tiles, dtype=np.int64)
    th = (theta0 + (T[:, None] * 768 + frames[None, :]) * dth) % 2 ** 32
    idx = ((th + 2 ** 21) >> 22) & 1023
    return int((idx[1:] != idx[:-1]).any(axis=1).sum())


def countdown_schedule(dth, frames, n_tiles, t0=0, theta0=0):
    """the kernel's schedule: look up on the first tile, then skip min over phases of the room to the cell edge / |D| tiles"""
    d = per_tile_advance(dth)
    looked, T = [], t0
    while T < t0 + n_tiles:
        looked.append(T)
        u = (theta0 + (T * 768 + frames) * dth + 2 ** 21) % 2 ** 32
        room = int(((u ^ (0x3fffff if d > 0 else 0)) & 0x3fffff).min())
        T += 1 + (10 ** 9 if d == 0 else room // abs(d))
    return looked


# shift, D, tiles (of 1999) where any of a wave's 768 phasors changes its index (the issue's table and the shifts below)
TABLE = [(200e3, 8192, 24), (-150e3, 0, 0), (100e3, 4096, 12), (310e3, 858980352, 1999), (123.456e3, -2122055680, 1999),
         (250e3, -8192, 24), (199999.97, -65536, 188)]


@pytest.mark.parametrize("shift,d,changes", TABLE)
def test_refresh_schedule_model(oracle, shift, d, changes):
    """On the 3.125 kHz grid (rate / 768) a wave's phases fall into three narrow clusters and |D| is a small multiple of 4096, so
    the wave's 768 indices change together on ~1 % of the tiles; off the grid every tile changes them.  The countdown schedule
    looks up exactly on the first tile and the tiles where the held (odd-stream) indices change."""
    dth = dtheta(oracle, shift)
    assert per_tile_advance(dth) == d
    assert tiles_with_a_change(dth, np.concatenate([EVEN, ODD])) == changes
    for t0, theta0 in ((0, 0), (777, 0x9e3779b9)):
        looked = countdown_schedule(dth, ODD, 2000, t0, theta0)
        T = np.arange(t0, t0 + 2000, dtype=np.int64)
        th = (theta0 + (T[:, None] * 768 + ODD[None, :]) * dth) % 2 ** 32
        idx = ((th + 2 ** 21) >> 22) & 1023
        want = [t0] + [int(t) for t in T[1:][(idx[1:] != idx[:-1]).any(axis=1)]]
        assert looked == want


def _chooser():
    from iq_tool_amd import _lib
    f = getattr(C.CDLL(_lib.LIB_PATH), "_ZN5iqgpu18front_mid_nco_holdEji")
    f.argtypes = [C.c_uint32, C.c_int]; f.restype = C.c_int
    return f


@pytest.mark.parametrize("shift", [200e3, -150e3, 100e3, 250e3, 199999.97, 200000.03, 310e3, 123.456e3, 1e3, 200001.0])
def test_hold_chooser_follows_the_model(oracle, shift):
    """front_mid_nco_hold (front_mid.hip): the hold is on where at most a quarter of the tiles would look the odd phasors up --
    the union of the arcs [p, p + |D|) over the cell -- and never at 8 outputs per lane."""
    dth = dtheta(oracle, shift)
    d = per_tile_advance(dth)
    share = tiles_with_a_change(dth, ODD, 4000) / 3999.0 if abs(d) < 2 ** 22 else 1.0
    f = _chooser()
    got = f(dth, 6)
    assert f(dth, 8) == 0
    if share < 0.2:
        assert got == 1, share
    elif share > 0.3:
        assert got == 0, share
    if shift in (200e3, -150e3, 100e3, 250e3):
        assert got == 1
    if shift in (310e3, 123.456e3):
        assert got == 0


# --------------------------------------------------------------------------------------------------------------------------------
# GPU: the hold against nco_hold=0, byte for byte
# --------------------------------------------------------------------------------------------------------------------------------
GPU_SHIFTS = [200e3, -150e3, 100e3, 250e3, 199999.97, 310e3]


def _run(gpu, raw, kw, splits, reset=True):
    ch = gpu.Chain(**kw)
    per = raw.size // sum(splits)
    outs, names, pos = [], [], 0
    for k in splits:
        outs.append(ch.process(raw[per * pos:per * (pos + k)])); pos += k
        names.append(ch.front_kernel())
    if reset:
        ch.reset()
        outs.append(ch.process(raw[:per * 1_200_000]))
        names.append(ch.front_kernel())
    return np.concatenate(outs), names


@pytest.mark.gpu
@pytest.mark.parametrize("shift", GPU_SHIFTS)
def test_hold_keeps_the_bytes_on_long_runs(gpu, oracle, monkeypatch, shift):
    """Eight CUs (cus=8: 96 waves), so every wave's run is ~200 tiles long and crosses several index changes (checked with the
    model), whole calls, ragged splits and a reset: equal bytes with and without the hold."""
    n = (1 << 24) + 1235
    raw = synth.raw_stream(n, RATE, 91, "cs16")
    kw = dict(NRSC5, shift_hz=shift)
    dth = dtheta(oracle, shift)
    if shift in (200e3, 199999.97):
        run = (n // 768) // 96
        assert min(tiles_with_a_change(dth, ODD, run, t0) for t0 in range(0, n // 768 - run, run)) >= 2
    monkeypatch.setenv("IQGPU_CUS", "8")
    monkeypatch.setenv("IQGPU_FORCE_FAT", "1")           # calls of any length on k_front_mid
    for splits in ([n], [5_000_001, 8, 4088, n - 5_004_097]):
        monkeypatch.setenv("IQGPU_NCO_HOLD", "0")
        ref, names_ref = _run(gpu, raw, kw, splits)
        monkeypatch.delenv("IQGPU_NCO_HOLD")
        got, names = _run(gpu, raw, kw, splits)
        assert names == names_ref and "k_front_mid<6,nco>" in names, names
        assert got.size == ref.size
        assert np.array_equal(got, ref), (splits, int((got != ref).sum()), int(np.flatnonzero(got != ref)[0]))


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [200e3, 199999.97])
@pytest.mark.parametrize("block_samples", [4096, 65536])
def test_hold_keeps_the_bytes_on_fixed_runs(gpu, monkeypatch, shift, block_samples):
    """block_samples: fixed-length runs dealt out inside a workgroup (the multi-run instantiation of k_front_mid), a run starting
    anywhere starts with a full lookup."""
    n = 6_000_017
    raw = synth.raw_stream(n, RATE, 92, "cs16")
    kw = dict(NRSC5, shift_hz=shift, block_samples=block_samples)
    monkeypatch.setenv("IQGPU_FORCE_FAT", "1")           # (the size rule keeps a call this short on k_front_s1)
    monkeypatch.setenv("IQGPU_NCO_HOLD", "0")
    ref, _ = _run(gpu, raw, kw, [n, ])
    monkeypatch.delenv("IQGPU_NCO_HOLD")
    got, names = _run(gpu, raw, kw, [n, ])
    assert any(nm.startswith("k_front_mid") for nm in names), names
    assert np.array_equal(got, ref), int((got != ref).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("in_format,out_format,extra", [("cu8", "cu8", {}), ("cs16", "cu8", {}), ("cs8", "cs16", {}),
                                                        ("cs16", "cs16", dict(agc=True)),
                                                        ("cu8", "cs16", dict(filters=(("passband", 158.5e3, 113e3),)))])
def test_hold_keeps_the_bytes_on_every_format(gpu, monkeypatch, in_format, out_format, extra):
    """8-bit frames either side, the fused AGC and cf32 out to a user filter: the same hold in every NCO instantiation."""
    n = 4_500_001
    raw = synth.raw_stream(n, RATE, 93, in_format)
    kw = dict(NRSC5, in_format=in_format, out_format=out_format, **extra)
    monkeypatch.setenv("IQGPU_FORCE_FAT", "1")
    splits = [n] if extra else [1_500_000, 8, 4088, n - 1_504_096]
    monkeypatch.setenv("IQGPU_NCO_HOLD", "0")
    ref, names_ref = _run(gpu, raw, kw, splits, reset=not extra)
    monkeypatch.delenv("IQGPU_NCO_HOLD")
    got, names = _run(gpu, raw, kw, splits, reset=not extra)
    assert names == names_ref and any(nm.startswith("k_front_mid<6,nco") for nm in names), names
    assert np.array_equal(got, ref), int((got != ref).sum())


@pytest.mark.gpu
def test_hold_output_is_close_to_the_oracle(gpu, oracle):
    """once against the CPU oracle: the headline chain with the hold (the bar of test_gpu_parity's int_close)"""
    n = 3_300_001
    raw = synth.raw_stream(n, RATE, 94, "cs16")
    got = gpu.Chain(**NRSC5).process(raw)
    want = oracle.Chain(**NRSC5).process(raw)
    assert got.shape == want.shape
    d = np.abs(got.astype(np.int64) - want.astype(np.int64))
    assert d.max() <= 1
    assert int((d != 0).sum()) <= max(3, int(np.ceil(0.002 * d.size)))
