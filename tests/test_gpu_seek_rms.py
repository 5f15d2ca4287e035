"""Seamless range sharding of chains with the dx / local output AGC (include/iqgpu.h): iqgpu_chain_seek_rms rebuilds the loop's state
at a stream position from the bounded window the library's own RMS kernels give it, and the seam certificate says whether it did.

Every comparison is GPU against GPU with no tolerance: ONE chain processes the whole stream (the unchanged ordinary path), three
chains seek to the starts of three ranges and process them.  Asserted per shape: at every seam the sought chain's gain, peak_memory
and samples_seen are bit-equal to the state of the chain that processed the range in front AND to the single stream's there; the
checkpoint right after a seek is byte-equal to the single stream's checkpoint at that frame (the blob is a function of the state:
this covers the warm-up window, the position words and the counters); the stitched bytes are the single stream's; so is the final
AGC state.

Geometry (agc_rms_geometry): local alpha 1e-2 -> warm 2600, chunk 256; dx alpha 1e-4 -> warm 260 000, chunk 16 250.  A call of a dx
chain costs warm + chunk dependent loop steps (~50 ms) whatever its length, so dx streams are processed in few, long calls.

Input: seeded Gaussian noise under level steps of -14, +14, +12 and -18 dB, never silent, so the single stream's own speculation
holds everywhere (the certificate at every seam is asserted, not assumed).  The seam that must NOT certify has its own stream.

Every figure is printed before it is asserted (pytest -s)."""
import functools

import numpy as np
import pytest

from shard_support import EINVAL, EUNSUPPORTED, fr, noise, run, words

pytestmark = pytest.mark.gpu
RATE = 2.4e6
GEOM = {"local": (2600, 256), "dx": (260000, 16250)}          # profile -> (warm, chunk)
RAGGED = 4 * 16384 + 37                                       # the call length of the checkpoint tests: 4 chunks + 37 frames

POINTWISE = dict(in_format="cs16", out_format="cs16", input_rate_hz=RATE, target_rate_hz=RATE, no_resample=True)
NRSC5 = dict(in_format="cs16", out_format="cs16", input_rate_hz=RATE, target_rate_hz=744187.5, shift_hz=200e3)
USB_FFT = dict(in_format="cs16", out_format="cf32", input_rate_hz=RATE, target_rate_hz=744187.5,
               filters=(("passband", 158.5e3, 113e3),), filter_impl="fft")
UP = dict(in_format="cs16", out_format="cs16", input_rate_hz=RATE, target_rate_hz=RATE * 1.2, shift_hz=150e3)
CU8 = dict(in_format="cu8", out_format="cs16", input_rate_hz=RATE, target_rate_hz=1488375.0)
# name -> (description, profile, input frames, the two cuts, calls of the single stream, what each cut is there for)
#   on_grid: cut_out is a multiple of the AGC chunk; from_reset: the trajectory in front of the cut starts at the reset (k chunk <= warm)
SHAPES = {
    "local_pointwise": (POINTWISE, "local", 327_680, (4096 * 25, 4096 * 55), 100_003, ("on_grid", "on_grid")),
    "local_decim": (NRSC5, "local", 1_000_000, (4096, 4096 * 150), 100_003, ("from_reset", "window")),
    # (the filter emits whole FFT blocks of 256: every cut of this chain is on the chunk grid of the local profile)
    "local_fft_cf32": (USB_FFT, "local", 1_000_000, (4096 * 80, 4096 * 170), 100_003, ("on_grid", "on_grid")),
    "local_up": (UP, "local", 250_000, (4096 * 20, 4096 * 41), 50_021, ("window", "window")),
    "dx_pointwise": (POINTWISE, "dx", 1_000_000, (4096 * 32, 4096 * 150), 250_007, ("from_reset", "window")),
    "dx_decim_cu8": (CU8, "dx", 1_700_000, (4096 * 60, 4096 * 250), 400_009, ("from_reset", "window")),
}


# The overlap-save windows of the FFT filter start at the head of a call's buffer, so its cf32 output is rounded as the calls are cut
# (the ordinary path's property: a fresh chain over [0, cut) in one call and in calls of 100 003 frames differ in the last bits).
# The AGC's window is made of those samples, so on such a chain a seek meets the single stream's state bit for bit where the single
# stream itself made the call the preroll is -- [cut - P_rms, cut) -- and elsewhere it is up to the certificate (include/iqgpu.h).
# In that shape the single stream ends every range with that call, and the shards make the single stream's calls.
SAME_CALLS = {"local_fft_cf32"}


def calls_of(name, a, b, per, n, p_rms):
    """the call boundaries of range [a, b)"""
    if name not in SAME_CALLS:
        return [(p, min(p + per, b)) for p in range(a, b, per)]
    last = b - p_rms if b != n else b
    return [(p, min(p + per, last)) for p in range(a, last, per)] + ([(last, b)] if last != b else [])


def no_agc(kw):
    return dict(kw, agc=False)


def in_calls(ch, x, a, b, per):
    return [ch.process(fr(x, p, min(p + per, b))) for p in range(a, b, per)]


@functools.lru_cache(maxsize=None)
def single_stream(name):
    """the ordinary path, once per shape: one chain over the whole stream, stopping at the cuts for its state and its checkpoint"""
    import iq_tool_amd as gpu
    kw, profile, n, cuts, per, _ = SHAPES[name]
    kw = dict(kw, agc=True, agc_profile=profile)
    x = noise(n, kw["in_format"], 7 + len(name))
    ch = gpu.Chain(**kw)
    outs, at = [], {}
    p_rms = gpu.design_preroll_frames_rms(**kw)
    for a, b in zip((0,) + cuts, cuts + (n,)):
        outs.append(np.concatenate([ch.process(fr(x, p, q)) for p, q in calls_of(name, a, b, per, n, p_rms)]))
        at[b] = (ch.agc_state_raw(), ch.save_state(), ch.tell())
    return kw, x, outs, at


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_three_shards_are_the_single_stream_and_every_seam_certifies(gpu, name):
    _, profile, n, cuts, per, kinds = SHAPES[name]
    kw, x, outs, at = single_stream(name)
    warm, chunk = GEOM[profile]
    p_rms = gpu.design_preroll_frames_rms(**kw)
    p_fir = gpu.design_preroll_frames(**no_agc(kw))
    print("%s: P_fir %d, P_rms %d, warm %d, chunk %d" % (name, p_fir, p_rms, warm, chunk))
    end_prev = None
    for s, (a, b) in enumerate(zip((0,) + cuts, cuts + (n,))):
        ch = gpu.Chain(**kw)
        if s:
            cut_out = gpu.design_out_frames_range(a, 0, **no_agc(kw))[0]
            k = (cut_out - 1) // chunk
            kind = kinds[s - 1]
            print("%s cut %d: output frame %d = chunk %d + %d, trajectory from %d, preroll %d frames (%s)"
                  % (name, a, cut_out, k, cut_out - k * chunk, max(0, k * chunk - warm), min(a, p_rms), kind))
            assert a % 4096 == 0
            assert (cut_out % chunk == 0) == (kind == "on_grid") and (k * chunk - warm <= 0) == (kind == "from_reset")
            pre = min(a, p_rms)
            ch.seek_rms(a, fr(x, a - pre, a))
            got, want, before = words(ch.agc_state_raw()), words(at[a][0]), words(end_prev)
            print("   sought %s\n   single %s\n   shard in front %s" % (got, want, before))
            assert got == before == want and got[2] == cut_out                       # the seam certifies
            assert ch.tell() == at[a][2] == (a, cut_out)
            blob = ch.save_state()
            diff = int((np.frombuffer(blob, np.uint8) != np.frombuffer(at[a][1], np.uint8)).sum()) if len(blob) == len(at[a][1]) else -1
            print("   checkpoint behind the seek: %d bytes, %d differ from the single stream's" % (len(blob), diff))
            assert diff == 0
        # (the middle range in ragged calls, the others whole: none of them the single stream's calls -- but for SAME_CALLS)
        mine = calls_of(name, a, b, per if name in SAME_CALLS else RAGGED if s == 1 else b - a, n, p_rms)
        out = np.concatenate([ch.process(fr(x, p, q)) for p, q in mine])
        diff = int((out.view(np.uint8) != outs[s].view(np.uint8)).sum()) if out.size == outs[s].size else -1
        print("%s range %d [%d, %d): %d output words, %d bytes differ" % (name, s, a, b, out.size, diff))
        assert out.size > 0 and diff == 0
        end_prev = ch.agc_state_raw()
        assert bytes(end_prev) == bytes(at[b][0])
    assert bytes(end_prev) == bytes(at[n][0])                                         # the final AGC state


def test_device_variant_longer_preroll_and_a_chain_that_has_run(gpu):
    kw, x, outs, at = single_stream("local_decim")
    _, _, n, cuts, _, _ = SHAPES["local_decim"]
    a = cuts[1]
    p = gpu.design_preroll_frames_rms(**kw)
    ch = gpu.Chain(**kw)
    ch.process(fr(x, 0, 70_001))                                       # mid-chunk, mid-group: the seek resets first
    pre = fr(x, a - 2 * p - 5, a)
    buf = gpu.DeviceBuffer(pre.nbytes)
    buf.upload(pre)
    ch.seek_rms_device(a, buf.ptr, 2 * p + 5)
    buf.free()
    assert words(ch.agc_state_raw()) == words(at[a][0]) and ch.save_state() == at[a][1]
    assert np.array_equal(np.concatenate(in_calls(ch, x, a, n, RAGGED)), outs[2])
    ch.seek_rms(0)                                                     # frame 0: a fresh chain
    assert ch.tell() == (0, 0) and np.array_equal(ch.process(fr(x, 0, cuts[0])), outs[0])


# --------------------------------------------------------------------------------------------
# the seam that must not certify: loud noise, then digital silence for more than P_rms frames up to and past a cut
# --------------------------------------------------------------------------------------------
SILENT_N, SILENT_FROM, SILENT_TO = 200_000, 60_000, 110_000
SILENT_CUTS = (4096 * 10, 4096 * 20)                                  # 40 960 in the noise, 81 920 with 21 920 zeros in front of it


def silent_stream():
    x = noise(SILENT_N, "cs16", 99, levels=(1.0,))
    x[2 * SILENT_FROM:2 * SILENT_TO] = 0
    return x


def test_a_seam_in_silence_does_not_certify_and_the_range_is_redone_from_the_checkpoint(gpu):
    kw = dict(POINTWISE, agc=True, agc_profile="local")
    x = silent_stream()
    p = gpu.design_preroll_frames_rms(**kw)
    assert SILENT_CUTS[1] - SILENT_FROM > p and SILENT_TO > SILENT_CUTS[1]
    one = gpu.Chain(**kw)
    bounds = (0,) + SILENT_CUTS + (SILENT_N,)
    want, single_at = [], {}
    for a, b in zip(bounds[:-1], bounds[1:]):
        want.append(np.concatenate(in_calls(one, x, a, b, 30_011)))
        single_at[b] = one.agc_state_raw()
    shards, outs, sought, ends, blobs = [], [], [None], [], []
    for s, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
        ch = gpu.Chain(**kw)
        if s:
            ch.seek_rms(a, fr(x, a - min(a, p), a))
            sought.append(words(ch.agc_state_raw()))
        outs.append(np.concatenate(in_calls(ch, x, a, b, b - a)))
        ends.append(words(ch.agc_state_raw()))
        blobs.append(ch.save_state())
        shards.append(ch)
    print("seam 1 (noise): sought %s, shard 0 ended %s" % (sought[1], ends[0]))
    print("seam 2 (silence): sought %s, shard 1 ended %s, single stream %s" % (sought[2], ends[1], words(single_at[SILENT_CUTS[1]])))
    assert sought[1] == ends[0] == words(single_at[SILENT_CUTS[0]])                   # the seam in the noise certifies ...
    assert np.array_equal(outs[0], want[0]) and np.array_equal(outs[1], want[1])      # ... and ranges 0 and 1 stand as they are
    assert ends[1] == words(single_at[SILENT_CUTS[1]])
    # the precondition of this test: in the silence the window cannot know the state
    assert sought[2] != ends[1] and sought[2][2] == ends[1][2]
    # the fallback: range 2 again from the checkpoint of shard 1
    redo = gpu.Chain(**kw)
    redo.load_state(blobs[1])
    again = np.concatenate(in_calls(redo, x, SILENT_CUTS[1], SILENT_N, RAGGED))
    assert np.array_equal(again, want[2])
    assert np.array_equal(np.concatenate([outs[0], outs[1], again]), np.concatenate(want))
    assert bytes(redo.agc_state_raw()) == bytes(single_at[SILENT_N])


# --------------------------------------------------------------------------------------------
# refusals, and the I/Q probe
# --------------------------------------------------------------------------------------------
def test_refusals_leave_the_chain_reset(gpu):
    kw = dict(NRSC5, agc=True, agc_profile="local")
    x = noise(200_000, "cs16", 3)
    a = 4096 * 30
    p = gpu.design_preroll_frames_rms(**kw)
    assert 1 < p < a
    fresh = gpu.Chain(**kw).process(fr(x, 0, 20_000))

    def refused(ch, code, word, call):
        with pytest.raises(gpu.IqgpuError) as e:
            call()
        print(e.value)
        assert e.value.code == code and word in str(e.value)
        assert ch.tell() == (0, 0)

    ch = gpu.Chain(**kw)
    ch.process(fr(x, 0, 33_333))
    refused(ch, EINVAL, "shorter", lambda: ch.seek_rms(a, fr(x, a - (p - 1), a)))
    assert np.array_equal(ch.process(fr(x, 0, 20_000)), fresh)                        # reset: as a fresh chain
    refused(ch, EINVAL, "2^39", lambda: ch.seek_rms((1 << 39) + 4096, fr(x, 0, p)))
    refused(ch, EINVAL, "in front of", lambda: ch.seek_rms(4096, fr(x, 0, 8192)))
    ch.process(fr(x, 0, 5_000))
    rc = ch._lib.iqgpu_chain_seek_rms(ch._h, a, None, p)
    assert rc == EINVAL and b"NULL" in ch._lib.iqgpu_last_error() and ch.tell() == (0, 0)
    assert ch._lib.iqgpu_chain_seek_rms(None, a, None, 0) == EINVAL
    # the seeks of the other families keep refusing a local chain
    for call in (lambda: ch.seek_agc(a, fr(x, a - p, a)), lambda: ch.seek(a, fr(x, a - p, a))):
        with pytest.raises(gpu.IqgpuError) as e:
            call()
        assert e.value.code == EUNSUPPORTED
    assert np.array_equal(ch.process(fr(x, 0, 20_000)), fresh)
    # chains this seek refuses
    for over, code, word in ((dict(agc=False), EINVAL, "no output AGC"), (dict(agc_profile="digital"), EUNSUPPORTED, "iqgpu_chain_seek_agc"),
                             (dict(dc_block=True), EUNSUPPORTED, "DC blocker")):
        other = gpu.Chain(**dict(kw, **over))
        first = other.process(fr(x, 0, 20_000))
        refused(other, code, word, lambda: other.seek_rms(a, fr(x, 0, a)))
        assert np.array_equal(other.process(fr(x, 0, 20_000)), first)


def test_the_iq_probe_takes_no_block_from_the_preroll_and_holds_none_behind_the_seek(gpu):
    kw = dict(NRSC5, agc=True, agc_profile="local")
    x = noise(200_000, "cs16", 3)
    a = 4096 * 30
    p = gpu.design_preroll_frames_rms(**kw)
    ch = gpu.Chain(**kw)
    ch.enable_iq_probe()
    ch.process(fr(x, 0, 8192))
    assert ch.read_iq_probe() is not None
    ch.process(fr(x, 8192, 16384))                                     # a block staged and unread
    ch.seek_rms(a, fr(x, a - p, a))
    assert ch.read_iq_probe() is None                                  # dropped by the seek, none taken from the preroll (p >= 1024)
    ch.process(fr(x, a, a + 500))
    assert ch.read_iq_probe() is None                                  # (a short call leaves the slot as it is)
    ch.process(fr(x, a + 500, a + 8192))
    blk = ch.read_iq_probe()
    ref = gpu.Chain(**kw)
    ref.enable_iq_probe()
    ref.process(fr(x, 0, a + 500))
    ref.read_iq_probe()
    ref.process(fr(x, a + 500, a + 8192))
    assert blk is not None and np.array_equal(blk, ref.read_iq_probe())  # the head of the first long call behind the seek


# --------------------------------------------------------------------------------------------
# the harness: --shards 3 --seamless-rms writes the file --shards 1 writes
# --------------------------------------------------------------------------------------------
HARNESS_ARGS = ["--raw-file-input-rate", "2.4e6", "--raw-file-input-sample-format", "cs16", "--output-rate", "744187.5",
                "--output-sample-format", "cs16", "--freq-shift", "200e3", "--agc-profile", "local", "--chunk-frames", "65536"]


def harness_pair(tmp_path, x):
    fin, one, many = tmp_path / "in.cs16", tmp_path / "one.cs16", tmp_path / "many.cs16"
    x.tofile(fin)
    run("-i", str(fin), *HARNESS_ARGS, "-o", str(one), "--shards", "1")
    info = run("-i", str(fin), *HARNESS_ARGS, "-o", str(many), "--shards", "3", "--seamless-rms", "--devices", "1")
    a, b = np.fromfile(one, np.int16), np.fromfile(many, np.int16)
    print({k: v for k, v in info.items() if k != "per_shard"})
    assert info["seamless_rms"] is True and info["shards"] == 3 and info["seams"] == 2
    assert a.size == b.size == 2 * info["frames_out"] and a.size > 0
    return info, int((a != b).sum())


def test_harness_seamless_rms_on_noise_certifies_every_seam(gpu, tmp_path):
    info, diff = harness_pair(tmp_path, noise(900_000, "cs16", 21))
    print("--shards 3 --seamless-rms against --shards 1: %d differing components" % diff)
    assert diff == 0 and info["seams_certified"] == 2 and info["ranges_redone"] == 0
    assert [ps["certified"] for ps in info["per_shard"]] == [False, True, True]


def test_harness_seamless_rms_redoes_the_range_behind_a_seam_in_silence(gpu, tmp_path):
    x = noise(900_000, "cs16", 22, levels=(1.0,))
    x[2 * 400_000:2 * 700_000] = 0                                     # the second cut (598 016) lies 198 016 zeros into the silence
    info, diff = harness_pair(tmp_path, x)
    print("--shards 3 --seamless-rms over a silent stretch: %d differing components, per shard %s"
          % (diff, [(ps["certified"], ps["redone"]) for ps in info["per_shard"]]))
    assert diff == 0 and info["ranges_redone"] >= 1 and info["per_shard"][2]["redone"] is True
    assert info["seams_certified"] + info["ranges_redone"] == 2
