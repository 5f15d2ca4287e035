"""Exact seamless range sharding of chains with the DC blocker AND the dx / local output AGC (include/iqgpu.h, iqgpu_chain_dcrms_*): the
DC map of every grid call, one walk over the maps, a seek that enters its preroll -- the single stream's own grid calls -- with the
walked state and rebuilds the AGC loop's state from the cf32 samples those calls leave, and the seam certificate behind it.

Every comparison is GPU against GPU with no tolerance.  The yardstick is ONE ordinary chain over the whole stream in calls on a grid
of C frames (the ordinary path, which the calls under test do not touch); three chains take three ranges.  Asserted per shape: the
walked DC state in front of every measured grid call is the single stream's get_dc_state there, bit for bit; at each seam gain,
peak_memory and samples_seen of the sought chain equal the single stream's at the cut AND the end state of the chain in front (the
seam certifies); the checkpoint right after the seek is byte-equal to the single stream's at that frame; tell() is equal; the
stitched bytes and the final DC and AGC states are equal.  The FFT-filter shape goes through the certificate procedure with its
fallback instead, and the certificate has to tell the truth.

Input: the noise generator and level steps of test_gpu_seek_rms.py (shard_support.noise): seeded Gaussian noise under steps of -14, +14, +12
and -18 dB, never silent.  The seam in silence has its own stream.

Geometry (agc_rms_geometry): local -> warm 2600, chunk 256; dx -> warm 260 000, chunk 16 250: a call of a dx chain costs ~50 ms
whatever its length, so the dx shape runs in few, long calls.

Every figure is printed before it is asserted (pytest -s)."""
import ctypes as C
import functools
import json
import subprocess

import numpy as np
import pytest

from shard_support import differing, EINVAL, EUNSUPPORTED, EXE, expect, fr, grid, noise, same, words

pytestmark = pytest.mark.gpu
RATE = 2.4e6
GEOM = {"local": (2600, 256), "dx": (260000, 16250)}          # profile -> (warm, chunk)

POINTWISE = dict(in_format="cs16", out_format="cs16", input_rate_hz=RATE, target_rate_hz=RATE, no_resample=True)
NRSC5 = dict(in_format="cs16", out_format="cs16", input_rate_hz=RATE, target_rate_hz=744187.5, shift_hz=200e3)
USB_FFT = dict(in_format="cs16", out_format="cf32", input_rate_hz=RATE, target_rate_hz=744187.5,
               filters=(("passband", 158.5e3, 113e3),), filter_impl="fft")
UP = dict(in_format="cs16", out_format="cs16", input_rate_hz=RATE, target_rate_hz=RATE * 1.2, shift_hz=150e3)
CU8 = dict(in_format="cu8", out_format="cs16", input_rate_hz=RATE, target_rate_hz=1488375.0)
# name -> (description, profile, input frames, the grid C, the two cuts in grid calls, must every seam certify)
SHAPES = {
    "local_pointwise": (POINTWISE, "local", 327_680, 4096, (25, 55), True),               # P < C: a one-call preroll
    # a preroll of several grid calls (their outputs contiguous across calls); the first cut lies so early that its preroll is all of [0, cut)
    "local_decim_small_grid": (NRSC5, "local", 1_000_000, 4096, (3, 150), True),
    "local_decim": (NRSC5, "local", 1_000_000, 65536, (2, 9), True),                      # one long preroll call
    "local_up": (UP, "local", 250_000, 8192, (5, 20), True),                              # the r >= 1 route
    "local_fft_cf32": (USB_FFT, "local", 1_000_000, 65536, (4, 10), False),               # FFT filter on the grid: whatever the certificate says
    "dx_decim_cu8": (CU8, "dx", 1_700_000, 262144, (2, 5), True),                         # dx geometry: a preroll of two grid calls
}


def on_grid(ch, x, a, b, c):
    outs = [ch.process(fr(x, p, q)) for p, q in grid(a, b, c)]
    return np.concatenate(outs) if outs else np.empty(0, np.uint8)


def full(kw, profile):
    return dict(kw, dc_block=True, agc=True, agc_profile=profile)


def single_over(gpu, kw, x, n, c, stops):
    """the ordinary path: one chain over [0, n) on the grid; the DC state behind every call, and at every stop the bytes since the
    stop in front, the AGC state, the checkpoint and tell()"""
    ch = gpu.Chain(**kw)
    dc, outs, at, part = [], [], {}, []
    for p, q in grid(0, n, c):
        part.append(ch.process(fr(x, p, q)))
        dc.append(ch.dc_state().copy())
        if q in stops:
            outs.append(np.concatenate(part))
            part = []
            at[q] = (ch.agc_state_raw(), ch.save_state(), ch.tell())
    return dict(dc=dc, outs=outs, at=at)


@functools.lru_cache(maxsize=None)
def single_stream(name):
    """once per shape, shared and left unchanged"""
    import iq_tool_amd as gpu
    kw, profile, n, c, cuts, _ = SHAPES[name]
    kw = full(kw, profile)
    x = noise(n, kw["in_format"], 7 + len(name))
    bounds = (0,) + tuple(k * c for k in cuts) + (n,)
    return kw, x, bounds, single_over(gpu, kw, x, n, c, set(bounds[1:]))


def walk(gpu, kw, x, c, upto, device_at=None):
    """steps 1 and 2 over the grid calls of [0, upto): the rows, before[], the state behind the last row"""
    m = gpu.Chain(**kw)
    if device_at is None:
        rows = [m.dcrms_dc_measure(p, fr(x, p, q)) for p, q in grid(0, upto, c)]
    else:
        rows = [m.dcrms_dc_measure_device(p, device_at(p), q - p) for p, q in grid(0, upto, c)]
    rows = np.concatenate([r.reshape(1) for r in rows])
    st, before = m.dcrms_dc_advance(None, rows)
    return rows, before, st


def dc_in_front_of(before, st, k):
    return before[k] if k < before.size else st


def pre_calls(gpu, kw, c, a):
    """the preroll of a cut at frame a, in grid calls: ceil(P / C), or all of [0, a) when that is less"""
    return min(a // c, -(-gpu.design_preroll_frames_dcrms(**kw) // c))


def seek_to(gpu, kw, x, c, a, before, st):
    k, n = a // c, pre_calls(gpu, kw, c, a)
    ch = gpu.Chain(**kw)
    ch.dcrms_seek(a, fr(x, (k - n) * c, a), c, dc_in_front_of(before, st, k - n))
    return ch


# --------------------------------------------------------------------------------------------
# 1. three ranges on three chains
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_three_shards_are_the_single_stream(gpu, name):
    _, profile, n, c, _, must_certify = SHAPES[name]
    kw, x, bounds, one = single_stream(name)
    warm, chunk = GEOM[profile]
    p = gpu.design_preroll_frames_dcrms(**kw)
    print("%s: P %d = %d grid calls of %d, warm %d, chunk %d, %d calls in the stream" % (name, p, -(-p // c), c, warm, chunk, len(one["dc"])))
    assert all(b % 4096 == 0 for b in bounds[:-1]) and c % 4096 == 0

    # steps 1 + 2: every grid call of every range but the last measured, one walk
    rows, before, st = walk(gpu, kw, x, c, bounds[2])
    wrong = [k for k in range(1, rows.size + 1) if not same(dc_in_front_of(before, st, k), one["dc"][k - 1])]
    last = one["dc"][rows.size - 1]
    print("%s: %d rows walked, %d states differ from the single stream's; state in front of the last range %.17g %+.17gi"
          % (name, rows.size, len(wrong), float(last["re"]), float(last["im"])))
    assert rows.size == bounds[2] // c and [int(r) for r in rows["frames"]] == [q - a for a, q in grid(0, bounds[2], c)]
    assert float(before[0]["re"]) == 0.0 and float(before[0]["im"]) == 0.0 and wrong == []
    assert np.hypot(float(last["re"]), float(last["im"])) > 0.0                         # (a state a stale zero would not pass for)

    # steps 3 + 4: seek, process on the grid, the certificate per seam in order
    end_prev = blob_prev = None
    stitched = []
    for s, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
        ch = gpu.Chain(**kw)
        if s:
            cut_out = gpu.design_out_frames_range(a, 0, **dict(kw, agc=False))[0]
            k = (cut_out - 1) // chunk
            ch = seek_to(gpu, kw, x, c, a, before, st)
            got, want, front = words(ch.agc_state_raw()), words(one["at"][a][0]), words(end_prev)
            certified, true = got == front, got == want
            print("%s cut %d: output frame %d = chunk %d + %d, trajectory from %d, preroll %d grid calls"
                  % (name, a, cut_out, k, cut_out - k * chunk, max(0, k * chunk - warm), pre_calls(gpu, kw, c, a)))
            print("   sought %s\n   single %s\n   shard in front %s\n   seam %d %s" % (got, want, front, s, "certified" if certified else "NOT certified"))
            assert certified == true and got[2] == cut_out          # the certificate tells the truth
            if must_certify:
                assert certified
            assert ch.tell() == one["at"][a][2] == (a, cut_out)
            assert same(ch.dc_state(), one["dc"][a // c - 1])
            blob = ch.save_state()
            diff = differing(np.frombuffer(blob, np.uint8), np.frombuffer(one["at"][a][1], np.uint8))
            print("   checkpoint behind the seek: %d bytes, %d differ from the single stream's" % (len(blob), diff))
            if certified:
                assert diff == 0
            else:
                # the fallback: this range from the checkpoint of the range in front
                ch = gpu.Chain(**kw)
                ch.load_state(blob_prev)
        out = on_grid(ch, x, a, b, c)
        diff = differing(out, one["outs"][s])
        print("%s range %d [%d, %d): %d output words, %d bytes differ" % (name, s, a, b, out.size, diff))
        assert out.size > 0 and diff == 0
        stitched.append(out)
        end_prev, blob_prev = ch.agc_state_raw(), ch.save_state()
        assert bytes(end_prev) == bytes(one["at"][b][0]) and same(ch.dc_state(), one["dc"][-(-b // c) - 1])
    assert same(np.concatenate(stitched), np.concatenate(one["outs"]))
    assert bytes(end_prev) == bytes(one["at"][n][0]) and same(ch.dc_state(), one["dc"][-1])      # the final states
    assert ch.tell() == one["at"][n][2]


# --------------------------------------------------------------------------------------------
# 2. the device entry points
# --------------------------------------------------------------------------------------------
def test_device_variants_give_the_host_variants_rows_and_states(gpu):
    name = "local_decim"
    _, _, n, c, _, _ = SHAPES[name]
    kw, x, bounds, one = single_stream(name)
    a = bounds[2]
    buf = gpu.DeviceBuffer(a * 4)
    buf.upload(fr(x, 0, a))
    assert buf.ptr % 16 == 0 and (c * 4) % 16 == 0                   # every call at the alignment of the host variants' staging
    at = lambda p: buf.ptr + p * 4
    rows_h, before_h, st_h = walk(gpu, kw, x, c, a)
    rows_d, before_d, st_d = walk(gpu, kw, x, c, a, device_at=at)
    print("device rows against host rows: %d bytes differ" % differing(rows_d, rows_h))
    assert same(rows_d, rows_h) and same(before_d, before_h) and same(st_d, st_h)
    k, npre = a // c, pre_calls(gpu, kw, c, a)
    host = seek_to(gpu, kw, x, c, a, before_h, st_h)
    dev = gpu.Chain(**kw)
    dev.process(fr(x, 0, 70_001))                                     # a chain that has run: the seek resets first
    dev.dcrms_seek_device(a, at((k - npre) * c), npre * c, c, dc_in_front_of(before_d, st_d, k - npre))
    buf.free()
    print("device seek %s, host seek %s, single %s" % (words(dev.agc_state_raw()), words(host.agc_state_raw()), words(one["at"][a][0])))
    assert bytes(dev.agc_state_raw()) == bytes(host.agc_state_raw()) == bytes(one["at"][a][0])
    assert same(dev.dc_state(), host.dc_state()) and dev.tell() == host.tell() == one["at"][a][2]
    assert dev.save_state() == host.save_state() == one["at"][a][1]
    assert same(on_grid(dev, x, a, n, c), one["outs"][2])
    dev.dcrms_seek_device(0, 0, 0)                                    # frame 0: a fresh chain
    assert dev.tell() == (0, 0) and same(on_grid(dev, x, 0, bounds[1], c), one["outs"][0])


# --------------------------------------------------------------------------------------------
# 3. the seam that must be caught: digital silence around the second cut
# --------------------------------------------------------------------------------------------
SILENT_N, SILENT_FROM, SILENT_TO, SILENT_C = 200_000, 60_000, 110_000, 4096
SILENT_CUTS = (4096 * 10, 4096 * 20)                                  # 40 960 in the noise, 81 920 with 21 920 zeros in front of it


def test_a_seam_in_silence_is_judged_truthfully_and_the_fallback_restores_the_stream(gpu):
    """behind the blocker a stretch of zeros is an output that decays from the blocker's state; whether the AGC's energy then stays
    under its freeze threshold for more than a chunk -- and the seam fails to certify -- depends on that state.  Asserted is what
    holds either way: the certificate's verdict is the comparison with the single stream, and after the fallback the bytes and the
    final states are the single stream's"""
    kw = full(POINTWISE, "local")
    c = SILENT_C
    x = noise(SILENT_N, "cs16", 99, levels=(1.0,))
    x[2 * SILENT_FROM:2 * SILENT_TO] = 0
    p = gpu.design_preroll_frames_dcrms(**kw)
    assert SILENT_CUTS[1] - SILENT_FROM > p and SILENT_TO > SILENT_CUTS[1]
    bounds = (0,) + SILENT_CUTS + (SILENT_N,)
    one = single_over(gpu, kw, x, SILENT_N, c, set(bounds[1:]))
    _, before, st = walk(gpu, kw, x, c, bounds[2])
    end_prev = blob_prev = None
    stitched, verdicts = [], []
    for s, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
        ch = gpu.Chain(**kw)
        if s:
            ch = seek_to(gpu, kw, x, c, a, before, st)
            got, want, front = words(ch.agc_state_raw()), words(one["at"][a][0]), words(end_prev)
            print("seam %d at %d: sought %s, shard in front ended %s, single stream %s" % (s, a, got, front, want))
            assert same(ch.dc_state(), one["dc"][a // c - 1])
            assert (got == front) == (got == want) and got[2] == front[2] == want[2]
            verdicts.append(got == front)
            if got != front:
                ch = gpu.Chain(**kw)
                ch.load_state(blob_prev)
        stitched.append(on_grid(ch, x, a, b, c))
        end_prev, blob_prev = ch.agc_state_raw(), ch.save_state()
        assert bytes(end_prev) == bytes(one["at"][b][0])
    print("seam in the noise %s, seam in the silence %s" % tuple("certified" if v else "NOT certified: range redone" for v in verdicts))
    assert verdicts[0]                                                                # the seam in the noise certifies
    assert all(same(o, w) for o, w in zip(stitched, one["outs"]))
    assert bytes(end_prev) == bytes(one["at"][SILENT_N][0]) and same(ch.dc_state(), one["dc"][-1])


# --------------------------------------------------------------------------------------------
# 4. refusals and argument checks
# --------------------------------------------------------------------------------------------
def test_refusals_and_argument_checks(gpu):
    from iq_tool_amd import _lib
    from iq_tool_amd.chain import DC_ROW, DC_STATE
    kw = full(NRSC5, "local")
    c = 4096
    x = noise(200_000, "cs16", 3)
    a = c * 30
    p = gpu.design_preroll_frames_dcrms(**kw)
    npre = -(-p // c) * c
    assert 1 < p < npre < a
    call0, pre = fr(x, 0, c), fr(x, a - npre, a)
    good = np.zeros(1, DC_ROW)
    good["f"] = 0.5

    # chains the new calls refuse -- and a refused call leaves them as they were
    for over, code, word in ((dict(dc_block=False), EINVAL, "DC blocker"), (dict(agc=False), EINVAL, "AGC"),
                             (dict(agc_profile="digital"), EUNSUPPORTED, "dx / local")):
        other = gpu.Chain(**dict(kw, **over))
        first = other.process(fr(x, 0, 20_000))
        expect(gpu, code, other.dcrms_dc_measure, 0, call0, word=word)
        expect(gpu, code, other.dcrms_dc_advance, None, good, word=word)
        assert other.tell()[0] == 20_000
        expect(gpu, code, other.dcrms_seek, a, pre, c, None, word=word)
        assert other.tell() == (0, 0) and same(other.process(fr(x, 0, 20_000)), first)       # a refused seek: reset
        with pytest.raises(gpu.IqgpuError) as e:
            gpu.design_preroll_frames_dcrms(**dict(kw, **over))
        assert e.value.code == code and word in str(e.value)

    ref = gpu.Chain(**kw)
    fresh, second = ref.process(fr(x, 0, 20_000)), ref.process(fr(x, 20_000, 40_000))
    ch = gpu.Chain(**kw)
    lib, h = ch._lib, ch._h
    row, st = _lib.DcRow(), _lib.DcState()
    buf = call0.ctypes.data_as(C.c_void_p)
    gp = good.ctypes.data_as(C.c_void_p)
    # refused measures and walks leave the handle as it was: the chain is one call into the stream while they are refused
    assert same(ch.process(fr(x, 0, 20_000)), fresh)
    for f in (lib.iqgpu_chain_dcrms_dc_measure, lib.iqgpu_chain_dcrms_dc_measure_device):
        assert f(None, 0, buf, c, C.byref(row)) == EINVAL and f(h, 0, buf, c, None) == EINVAL and f(h, 0, None, c, C.byref(row)) == EINVAL
        assert b"NULL" in lib.iqgpu_last_error()
    assert lib.iqgpu_chain_dcrms_dc_advance(None, C.byref(st), gp, 1, None) == EINVAL
    assert lib.iqgpu_chain_dcrms_dc_advance(h, None, gp, 1, None) == EINVAL
    assert lib.iqgpu_chain_dcrms_dc_advance(h, C.byref(st), None, 1, None) == EINVAL
    expect(gpu, EINVAL, ch.dcrms_dc_measure, 1 << 39, call0, word="2^39")
    bad = np.zeros(2, DC_ROW)
    bad["f"] = (0.5, float("nan"))
    expect(gpu, EINVAL, ch.dcrms_dc_advance, None, bad, word="row 1")
    nan = np.zeros((), DC_STATE)
    nan["re"] = float("nan")
    expect(gpu, EINVAL, ch.dcrms_dc_advance, nan, good, word="finite")
    # ... and the old calls still refuse this chain, with their old words
    expect(gpu, EUNSUPPORTED, ch.dc_measure, 0, call0, word="AGC")
    expect(gpu, EUNSUPPORTED, ch.dc_advance, None, good, word="AGC")
    expect(gpu, EUNSUPPORTED, ch.dcagc_dc_measure, 0, fr(x, 0, 16384), word="dx / local")
    expect(gpu, EUNSUPPORTED, ch.dcagc_dc_advance, None, good, word="dx / local")
    expect(gpu, EUNSUPPORTED, ch.dcagc_measure, fr(x, 0, 16384), word="dx / local")
    assert ch.tell()[0] == 20_000 and same(ch.process(fr(x, 20_000, 40_000)), second)
    for call, word in ((lambda: ch.seek_dc(a, pre, c, None), "AGC"), (lambda: ch.seek_rms(a, pre), "DC blocker"),
                       (lambda: ch.dcagc_seek(4 * 16384, fr(x, 0, 4 * 16384), 16384, None, None), "dx / local"),
                       (lambda: ch.seek(a, pre), "AGC"), (lambda: ch.seek_agc(a, pre), "dx / local")):
        expect(gpu, EUNSUPPORTED, call, word=word)
    with pytest.raises(gpu.IqgpuError) as e:
        gpu.design_preroll_frames_rms(**kw)
    assert e.value.code == EUNSUPPORTED and "DC blocker" in str(e.value)

    # refused seeks leave the chain reset
    assert lib.iqgpu_chain_dcrms_seek(None, 0, None, 0, 0, None) == EINVAL
    assert lib.iqgpu_chain_dcrms_seek_device(None, 0, None, 0, 0, None) == EINVAL
    ch.process(fr(x, 0, 5_000))
    assert lib.iqgpu_chain_dcrms_seek(h, a, None, npre, c, None) == EINVAL and b"NULL" in lib.iqgpu_last_error()      # NULL preroll
    assert ch.tell() == (0, 0)
    for args, word in [((a, fr(x, a - (p - 1), a), 0, None), "shorter"),                    # shorter than min(first_frame, P)
                       ((c, fr(x, 0, c)[:-8], 0, None), "shorter"),                           # ... where that is first_frame
                       ((a, fr(x, a - npre - 100, a), c, None), "whole number"),              # not whole calls
                       ((c, fr(x, 0, 2 * c), c, None), "in front of"),                        # longer than first_frame
                       ((a, pre, c, nan), "finite"),
                       (((1 << 39) + c, pre, c, None), "2^39")]:
        ch.process(fr(x, 0, 33_333))
        expect(gpu, EINVAL, ch.dcrms_seek, *args, word=word)
        assert ch.tell() == (0, 0)
        assert same(ch.process(fr(x, 0, 20_000)), fresh), word                              # reset: as a fresh chain
        ch.reset()
    # frame 0 without a preroll leaves a fresh chain
    ch.process(fr(x, 0, 33_333))
    ch.dcrms_seek(0)
    assert ch.tell() == (0, 0) and same(ch.process(fr(x, 0, 20_000)), fresh)


# --------------------------------------------------------------------------------------------
# 5. the I/Q probe: rules 2 and 3
# --------------------------------------------------------------------------------------------
def test_the_iq_probe_takes_no_block_from_the_measure_or_the_preroll(gpu):
    kw = full(NRSC5, "local")
    c = 8192
    x = noise(200_000, "cs16", 3)
    a = c * 12
    assert gpu.design_preroll_frames_dcrms(**kw) >= 1024
    _, before, st = walk(gpu, kw, x, c, a)
    k, npre = a // c, pre_calls(gpu, kw, c, a)
    ch = gpu.Chain(**kw)
    ch.enable_iq_probe()
    ch.process(fr(x, 0, c))
    assert ch.read_iq_probe() is not None
    ch.process(fr(x, c, 2 * c))                                        # a block staged and unread
    ch.dcrms_seek(0)
    assert ch.read_iq_probe() is None                                  # the seek drops it
    ch.dcrms_dc_measure(c, fr(x, c, 2 * c))
    assert ch.read_iq_probe() is None                                  # the measure call leaves none
    ch.process(fr(x, 0, c))
    assert ch.read_iq_probe() is not None                              # (held from here on)
    ch.dcrms_seek(a, fr(x, (k - npre) * c, a), c, dc_in_front_of(before, st, k - npre))
    assert ch.read_iq_probe() is None                                  # the held one dropped, none taken from the preroll
    ch.process(fr(x, a, a + 500))
    assert ch.read_iq_probe() is None                                  # (a short call leaves the slot as it is)
    ch.process(fr(x, a + 500, a + c))
    blk = ch.read_iq_probe()
    ref = gpu.Chain(**kw)
    ref.enable_iq_probe()
    on_grid(ref, x, 0, a, c)
    ref.process(fr(x, a, a + 500))
    ref.read_iq_probe()
    ref.process(fr(x, a + 500, a + c))
    assert blk is not None and same(blk, ref.read_iq_probe())          # the head of the first long call behind the seek


# --------------------------------------------------------------------------------------------
# 6. the harness: --shards 3 --seamless-dc-rms writes the file --shards 1 writes
# --------------------------------------------------------------------------------------------
def test_harness_seamless_dc_rms_writes_the_single_stream_and_certifies_both_seams(gpu, tmp_path):
    name = "local_decim"
    _, _, n, c, _, _ = SHAPES[name]
    kw, x, _, _ = single_stream(name)
    fin, one, many = tmp_path / "in.cs16", tmp_path / "one.cs16", tmp_path / "many.cs16"
    x.tofile(fin)
    args = ["-i", str(fin), "--raw-file-input-rate", "2.4e6", "--raw-file-input-sample-format", "cs16", "--output-rate", "744187.5",
            "--output-sample-format", "cs16", "--freq-shift", "200e3", "--dc-block", "--agc-profile", "local", "--chunk-frames", str(c)]

    def run(*more):
        r = subprocess.run([EXE, *args, *more], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr + r.stdout
        return json.loads(r.stdout.strip().splitlines()[-1])

    run("-o", str(one), "--shards", "1")
    info = run("-o", str(many), "--shards", "3", "--seamless-dc-rms", "--devices", "1")
    print({k: v for k, v in info.items() if k != "per_shard"})
    print([(ps["first_frame"], ps["preroll_frames"], ps["dc_rows"], ps["certified"], ps["redone"]) for ps in info["per_shard"]])
    a, b = np.fromfile(one, np.int16), np.fromfile(many, np.int16)
    diff = int((a != b).sum()) if a.size == b.size else -1
    print("--shards 3 --seamless-dc-rms against --shards 1: %d differing components of %d" % (diff, a.size))
    assert info["seamless_dc_rms"] is True and info["shards"] == 3 and info["seams"] == 2
    pre = -(-gpu.design_preroll_frames_dcrms(**kw) // c) * c
    for s, ps in enumerate(info["per_shard"]):
        assert ps["first_frame"] == s * (n // 3) // c * c and ps["preroll_frames"] == min(ps["first_frame"], pre)
        assert ps["dc_rows"] == (-(-ps["frames_in"] // c) if s < 2 else 0) and ps["frames_out"] == ps["planned_out"]
    assert a.size == b.size == 2 * info["frames_out"] and a.size > 0 and diff == 0
    assert info["seams_certified"] == 2 and info["ranges_redone"] == 0
    assert [ps["certified"] for ps in info["per_shard"]] == [False, True, True]
