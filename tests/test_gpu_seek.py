"""Seamless range sharding on the device: a chain put at stream frame a by iqgpu_chain_seek (closed-form position + a discarded
warm-up over the frames in front of a) continues the stream exactly as the chain that ran frames [0, a) does.

The yardstick for bytes is the unchanged per-call path: ONE chain processes [0, a) and then [a, n) in two calls, and the second
call's output is the reference.  A fresh chain after seek(a, raw[a - P:a]) processing [a, n) must give those bytes -- every
routing of the front (one case per kernel family, each asserting front_kernel() so that the case proves what it covered), both
filter kinds on both sides of the resampler, an aligned seam (a multiple of 4096 frames) and a ragged one (a odd: rem != 0 and
phi != 0).  The same frames are also the slice [out_first, out_first + frames_out) of the ORACLE's single stream, to the project's
bars (integer outputs +-1 LSB and >= 99.8 % identical codes, 99.5 % behind a filter; cf32 1e-5).  Chains with the DC blocker are
seamless to 1e-6 of full scale by derivation (include/iqgpu.h); their bar here is the project's: int_close on cs16, 1e-5 on cf32.

Every comparison prints its figure before it asserts (pytest -s shows them)."""
import subprocess

import numpy as np
import pytest

from iq_tool_amd import synth

from shard_support import EHIP, EINVAL, EUNSUPPORTED, EXE, frames, run, set_switches

pytestmark = pytest.mark.gpu
TOL = 1e-5

NRSC5 = dict(in_format="cs16", out_format="cs16", input_rate_hz=2.4e6, target_rate_hz=744187.5, shift_hz=200e3)
CU8_NRSC5 = dict(in_format="cu8", out_format="cu8", input_rate_hz=2.4e6, target_rate_hz=1488375.0)
TEN_TO_2M4 = dict(in_format="cs16", out_format="cs16", input_rate_hz=10e6, target_rate_hz=2.4e6, shift_hz=-300e3)
SIXTY_TO_1M488 = dict(in_format="cu8", out_format="cu8", input_rate_hz=61.44e6, target_rate_hz=1488375.0)
CONFIG3_FILTER = dict(filters=(("passband", 158.5e3, 113e3),), filter_taps=1024)              # 1025 taps, FFT kind, block 2048
CONFIG4_FILTER = dict(filters=(("lowpass", 300e3, 0.0),), filter_taps=4097, filter_impl="fir")
SWITCHES = ("FORCE_FAT", "FAT", "NO_P0", "NO_S2", "FORCE_GENERIC", "FFT_NO_R16", "FFT_LOG2N", "NO_FAT", "NO_CASC2", "CASC2_MIN_RUN")

# name -> (description, IQGPU_<NAME> switches, frames, front kernel of the call behind the ALIGNED seam or None, bar behind a filter)
CASES = {
    "nrsc5_s1": (NRSC5, {}, 1_000_003, "k_front_s1", False),
    "nrsc5_mid": (NRSC5, dict(FORCE_FAT="1"), 1_000_003, "k_front_mid<6,nco>", False),
    "nrsc5_fat": (NRSC5, dict(FORCE_FAT="1", FAT="1"), 1_000_003, "k_front_fat", False),
    "cu8_s0_s1": (CU8_NRSC5, dict(NO_P0="1"), 900_005, "k_front_s1", False),
    "cu8_s0_p0": (CU8_NRSC5, dict(FORCE_FAT="1"), 900_005, "k_front_p0", False),
    "s2": (TEN_TO_2M4, {}, 1_000_003, "k_front_s2", False),
    "s2_two_kernels": (TEN_TO_2M4, dict(NO_S2="1"), 1_000_003, "k_cascade+k_front_s1", False),
    "cascade2": (dict(SIXTY_TO_1M488, out_format="cs16", block_samples=40 * 8192), {}, (1 << 22) + 16384 * 3 + 8, "k_cascade2+k_front_s1", False),
    "fir4097_behind": (dict(SIXTY_TO_1M488, **CONFIG4_FILTER), {}, 1 << 21, None, True),
    "fft1025_behind": (dict(TEN_TO_2M4, **CONFIG3_FILTER), {}, 1 << 20, None, True),
    "interp": (dict(in_format="cs16", out_format="cs16", input_rate_hz=2.0e6, target_rate_hz=2.4e6, shift_hz=150e3), {}, 600_001, "k_front+k_interp", False),
    "no_resample_pre_filter": (dict(in_format="cs16", out_format="cf32", input_rate_hz=2.4e6, no_resample=True, shift_hz=-250e3,
                                    filters=(("passband", -300e3, 100e3),), transition_width_hz=20e3, attenuation_db=70.0,
                                    filter_impl="fft", fft_size=2048), {}, 500_001, "k_front", True),
    "generic": (NRSC5, dict(FORCE_GENERIC="1"), 700_001, "k_front", False),
    "post_nco": (dict(NRSC5, shift_after_resample=True), {}, 1_000_003, None, False),
    "post_nco_behind_fft": (dict(TEN_TO_2M4, shift_after_resample=True, out_format="cf32", **CONFIG3_FILTER), {}, 1 << 20, None, True),
}


def cf(a):
    return np.ascontiguousarray(a).view(np.float32).view(np.complex64)


def int_close(a, b, min_same, what):
    assert a.shape == b.shape, (a.shape, b.shape)
    d = np.abs(a.astype(np.int64) - b.astype(np.int64))
    same = float((d == 0).mean()) if d.size else 1.0
    print("%s: max code difference %d, %.5f of %d codes identical (bar %.4f)" % (what, int(d.max()) if d.size else 0, same, a.size, min_same))
    assert d.size and d.max() <= 1
    assert int((d != 0).sum()) <= max(3, int(np.ceil((1.0 - min_same) * a.size)))


def run_oracle(oracle, raw, **kw):
    kw = dict(kw)
    kw.pop("block_samples", None)
    ft = kw.get("filter_taps", 0)
    if ft and ft % 2 == 0:
        kw["filter_taps"] = ft + 1          # the odd bump of src/config.c:233-236, which make_desc applies on the product's side
    return oracle.Chain(**kw).process(raw)


def seams(gpu, kw):
    """an aligned seam and a ragged one, both behind the chain's whole memory so that the warm-up is what is tested"""
    p = gpu.design_preroll_frames(**kw)
    aligned = (p // 4096 + 2) * 4096
    return p, aligned, aligned + 4096 + 37


@pytest.mark.parametrize("name", sorted(CASES))
def test_seek_continues_the_stream_byte_for_byte(gpu, oracle, monkeypatch, name):
    kw, sw, n, kernel, filtered = CASES[name]
    set_switches(monkeypatch, SWITCHES, sw)
    raw = synth.raw_stream(n, kw["input_rate_hz"], 51, kw["in_format"])
    obpf = 2                                                    # components per output frame
    want = run_oracle(oracle, raw, **kw)
    p, aligned, ragged = seams(gpu, kw)
    info = gpu.Chain(**kw).info()
    S, block = int(info.num_halfband_stages), int(info.filter_block)
    assert ragged + 65536 < n and ragged % 2 == 1 and ragged % (1 << max(S, 1)) != 0
    if name == "fft1025_behind":
        # the seam leaves samples pending in front of the FFT block: resampler outputs in front of it are no multiple of the block
        for a in (aligned, ragged):
            assert block == 2048 and (-(-((a >> S) << 24) // int(info.arb_step))) % block != 0
    for a in (aligned, ragged):
        ref = gpu.Chain(**kw)
        ref.process(frames(kw, raw, 0, a))
        y = ref.process(frames(kw, raw, a, n))
        ch = gpu.Chain(**kw)
        ch.seek(a, frames(kw, raw, a - p, a))
        g = ch.process(frames(kw, raw, a, n))
        print("%s seam %d (preroll %d): %s" % (name, a, p, ch.front_kernel()))
        assert ch.front_kernel() == ref.front_kernel()
        if kernel is not None and a == aligned:
            assert ch.front_kernel() == kernel, ch.front_kernel()
        assert g.size == y.size and g.size > 0
        assert np.array_equal(g.view(np.uint8), y.view(np.uint8)), (name, a, int((g != y).sum()), int(np.flatnonzero(g != y)[0]))
        # ... and it is its slice of the oracle's single stream
        first, count = gpu.design_out_frames_range(a, n - a, **kw)
        assert count * obpf == g.size and (first + count) * obpf == want.size
        w = want[first * obpf:(first + count) * obpf]
        if kw["out_format"] == "cf32":
            err = float(np.abs(cf(g) - cf(w)).max())
            print("%s seam %d: max |delta| against the oracle's slice %.3g" % (name, a, err))
            assert err <= TOL
        else:
            int_close(g, w, 0.995 if filtered else 0.998, "%s seam %d against the oracle's slice" % (name, a))


def test_a_longer_preroll_and_the_device_variant_give_the_same_bytes(gpu):
    kw, n = dict(TEN_TO_2M4, **CONFIG3_FILTER), 1 << 20
    raw = synth.raw_stream(n, kw["input_rate_hz"], 52, kw["in_format"])
    p = gpu.design_preroll_frames(**kw)
    a = 3 * p + 4096 + 37
    ref = gpu.Chain(**kw)
    ref.process(frames(kw, raw, 0, a))
    y = ref.process(frames(kw, raw, a, n))
    ch = gpu.Chain(**kw)
    ch.seek(a, frames(kw, raw, a - 2 * p - 3, a))              # longer than needed is allowed
    assert np.array_equal(ch.process(frames(kw, raw, a, n)), y)
    pre = frames(kw, raw, a - p, a)
    buf = gpu.DeviceBuffer(pre.nbytes)
    buf.upload(pre)
    ch.seek_device(a, buf.ptr, p)                               # ... on a chain that has run: seek resets first
    assert np.array_equal(ch.process(frames(kw, raw, a, n)), y)
    buf.free()


@pytest.mark.parametrize("out_format", ["cs16", "cf32"])
def test_dc_blocker_chain_is_seamless_to_the_derived_bound(gpu, out_format):
    """configs[2]'s front (DC blocker + I/Q correction in front of the 1025-tap FFT filter), 2^23 frames at 10 MS/s, seams BEHIND the
    preroll (~2.2 M frames: the IIR state is approximated, error <= 1e-6 of full scale by derivation) against the two-call reference:
    int_close on cs16, <= 1e-5 on cf32.  A seam inside the preroll warms up from frame 0 and is exact.
    Measured on an MI355X: cf32 max |delta| 6.2e-8 / 6.4e-8 at the two seams; cs16 max 1 LSB, 99.998 % identical codes."""
    kw = dict(in_format="cs16", out_format=out_format, input_rate_hz=10e6, target_rate_hz=2.4e6, dc_block=True, iq_correct=True,
              iq_mag=0.01, iq_phase=-0.005, **CONFIG3_FILTER)
    n = 1 << 23
    raw = synth.raw_stream(n, 10e6, 53, "cs16")
    p, aligned, ragged = seams(gpu, kw)
    assert 2_100_000 < p < 2_300_000 and ragged + (1 << 20) < n
    for a in (aligned, ragged, 1_000_001):
        ref = gpu.Chain(**kw)
        ref.process(frames(kw, raw, 0, a))
        y = ref.process(frames(kw, raw, a, n))
        ch = gpu.Chain(**kw)
        ch.seek(a, frames(kw, raw, max(0, a - p), a))
        g = ch.process(frames(kw, raw, a, n))
        assert g.size == y.size and g.size > 0
        if a < p:
            assert np.array_equal(g.view(np.uint8), y.view(np.uint8)), (a, int((g != y).sum()))
        elif out_format == "cf32":
            err = float(np.abs(cf(g) - cf(y)).max())
            print("dc seam %d (preroll %d): max |delta| against the two-call reference %.3g" % (a, p, err))
            assert err <= TOL
        else:
            int_close(g, y, 0.995, "dc seam %d (preroll %d) against the two-call reference" % (a, p))


def test_seek_drains_submitted_batches_first(gpu):
    kw, n, batch = NRSC5, 1_000_003, 65536
    raw = synth.raw_stream(n, 2.4e6, 54, "cs16")
    p, a = gpu.design_preroll_frames(**kw), 3 * batch + 53_393      # the seam: behind the three batches, odd
    plain = gpu.Chain(**kw)
    want_batches = [plain.process(frames(kw, raw, i * batch, (i + 1) * batch)) for i in range(3)]
    plain.process(frames(kw, raw, 3 * batch, a))
    y = plain.process(frames(kw, raw, a, n))
    ch = gpu.Chain(**kw)
    cap = ch.max_out_frames(batch) * ch.out_bytes
    bufs, flight = [], []
    for i in range(3):
        ib, ob = gpu.PinnedBuffer(batch * ch.in_bytes), gpu.PinnedBuffer(cap)
        ib.array[:] = frames(kw, raw, i * batch, (i + 1) * batch)
        got, t = ch.submit(ib.ptr, batch, ob.ptr, cap)
        bufs.append((ib, ob)); flight.append((t, got, ob))
    ch.seek(a, frames(kw, raw, a - p, a))                       # three batches submitted, none collected
    for (t, got, ob), w in zip(flight, want_batches):
        ch.collect(t)
        assert np.array_equal(ob.array[:got * ch.out_bytes].view(np.int16), w)
    assert np.array_equal(ch.process(frames(kw, raw, a, n)), y)
    for ib, ob in bufs:
        ib.free(); ob.free()


def test_seek_zero_is_a_fresh_chain_and_a_short_preroll_is_refused(gpu):
    kw, n = dict(TEN_TO_2M4, **CONFIG3_FILTER), 400_001
    raw = synth.raw_stream(n, kw["input_rate_hz"], 55, kw["in_format"])
    fresh = gpu.Chain(**kw).process(raw)
    ch = gpu.Chain(**kw)
    ch.process(frames(kw, raw, 0, 123_457))                     # leaves an open group, a phase and samples pending in front of the block
    ch.seek(0)
    assert np.array_equal(ch.process(raw), fresh)
    p, _, a = seams(gpu, kw)
    for short in (0, 1, p - 1):
        with pytest.raises(gpu.IqgpuError) as e:
            ch.seek(a, frames(kw, raw, a - short, a))
        assert e.value.code == EINVAL and "shorter" in str(e.value)
        assert np.array_equal(ch.process(raw), fresh)           # ... and the chain is left reset
    with pytest.raises(gpu.IqgpuError) as e:                    # a preroll cannot start in front of frame 0
        ch.seek(100, frames(kw, raw, 0, 101))
    assert e.value.code == EINVAL
    with pytest.raises(gpu.IqgpuError) as e:
        ch.seek(1 << 63)
    assert e.value.code == EINVAL
    ch.seek(1000, frames(kw, raw, 0, 1000))                     # inside the chain's memory: the warm-up starts at frame 0
    assert np.array_equal(ch.process(frames(kw, raw, 1000, n)), _tail(gpu, kw, raw, 1000, n))


def _tail(gpu, kw, raw, a, n):
    ref = gpu.Chain(**kw)
    ref.process(frames(kw, raw, 0, a))
    return ref.process(frames(kw, raw, a, n))


def test_seek_refuses_a_chain_with_the_output_agc(gpu):
    kw = dict(NRSC5, agc=True)
    raw = synth.raw_stream(300_000, 2.4e6, 56, "cs16")
    fresh = gpu.Chain(**kw).process(raw)
    ch = gpu.Chain(**kw)
    ch.process(raw[:2 * 100_000])
    with pytest.raises(gpu.IqgpuError) as e:
        ch.seek(8192, raw[:2 * 8192])
    assert e.value.code == EUNSUPPORTED and "AGC" in str(e.value)
    ch.seek(0)                                                  # frame 0 is a reset: every chain can do that
    assert np.array_equal(ch.process(raw), fresh)


def test_seek_clears_a_poisoned_handle(gpu, monkeypatch):
    """A call that fails behind its first launch poisons the handle until a reset -- or a seek.  The failure here is a refusal on the
    HOST, before anything of the filter is launched: with the radix-16 transform switched off and a 16384-point transform asked
    for, launch_fftconv's own argument check turns the launch down (the radix-4 kernel stops at 8192 points).  Calls that emit no
    block never reach that check, which is how the handle shows that it works again."""
    set_switches(monkeypatch, SWITCHES, dict(FFT_NO_R16="1", FFT_LOG2N="14"))
    kw = dict(in_format="cs16", out_format="cs16", input_rate_hz=2.4e6, no_resample=True, filters=(("lowpass", 300e3, 0.0),), filter_taps=129,
              filter_impl="fft")
    raw = synth.raw_stream(8192, 2.4e6, 57, "cs16")
    ch = gpu.Chain(**kw)
    block = int(ch.info().filter_block)
    assert block >= 256
    with pytest.raises(gpu.IqgpuError) as e:
        ch.process(raw)
    assert e.value.code == EHIP
    with pytest.raises(gpu.IqgpuError) as e:
        ch.process(raw[:2 * 100])
    assert e.value.code == EHIP and "reset" in str(e.value)
    ch.seek(0)
    assert ch.process(raw[:2 * 100]).size == 0                  # accepted again (100 frames stay pending in front of the block)


# --------------------------------------------------------------------------------------------
# the harness: --shards N --seamless writes the file --shards 1 writes
# --------------------------------------------------------------------------------------------
ARGS = ["--raw-file-input-rate", "2.4e6", "--raw-file-input-sample-format", "cs16", "--output-rate", "744187.5",
        "--output-sample-format", "cs16", "--freq-shift", "200e3"]


def check_seamless_report(gpu, info, shards, n):
    want_pre = gpu.design_preroll_frames(**NRSC5)
    assert info["seamless"] is True and info["shards"] == shards and info["frames_in"] == n
    assert info["frames_out"] == gpu.design_out_frames(n, **NRSC5)
    for s, ps in enumerate(info["per_shard"]):
        assert ps["first_frame"] % 4096 == 0 and ps["frames_out"] == ps["planned_out"]
        assert ps["preroll_frames"] == min(ps["first_frame"], want_pre)
    assert info["per_shard"][0]["first_frame"] == 0 and info["per_shard"][1]["first_frame"] > want_pre


@pytest.mark.parametrize("shards,n,chunk", [(4, 2_000_003, "131072"), (3, 3 * 777_777 + 5, "49152")])
def test_harness_seamless_shards_write_the_single_stream(gpu, tmp_path, shards, n, chunk):
    raw = synth.raw_stream(n, 2.4e6, 58, "cs16")
    fin, one, many, plain = tmp_path / "in.cs16", tmp_path / "one.cs16", tmp_path / "many.cs16", tmp_path / "plain.cs16"
    raw.tofile(fin)
    run("-i", str(fin), "-o", str(one), *ARGS, "--shards", "1", "--chunk-frames", chunk)
    info = run("-i", str(fin), "-o", str(many), *ARGS, "--shards", str(shards), "--seamless", "--devices", "1", "--chunk-frames", chunk)
    check_seamless_report(gpu, info, shards, n)
    a, b = np.fromfile(one, np.int16), np.fromfile(many, np.int16)
    assert a.size == b.size and a.size == 2 * info["frames_out"]
    assert np.array_equal(a, b), (int((a != b).sum()), int(np.flatnonzero(a != b)[0]))
    assert np.array_equal(a, gpu.Chain(**NRSC5).process(raw))
    # ... which the independent-stream default is not: it restarts phase, group and histories at every seam
    info = run("-i", str(fin), "-o", str(plain), *ARGS, "--shards", str(shards), "--devices", "1", "--chunk-frames", chunk)
    assert "seamless" not in info and "preroll_frames" not in info["per_shard"][0]
    c = np.fromfile(plain, np.int16)
    assert c.size != a.size or not np.array_equal(a, c)


def test_harness_seamless_synthetic_hash_is_one_stream(gpu, tmp_path):
    n, seed = 2_000_003, 40
    one, many = tmp_path / "one.cs16", tmp_path / "many.cs16"
    run("--synthetic", str(n), "--synthetic-hash", str(seed), "-o", str(one), *ARGS, "--shards", "1", "--chunk-frames", "131072")
    info = run("--synthetic", str(n), "--synthetic-hash", str(seed), "-o", str(many), *ARGS, "--shards", "4", "--seamless", "--devices", "1",
               "--chunk-frames", "131072")
    check_seamless_report(gpu, info, 4, n)
    a, b = np.fromfile(one, np.int16), np.fromfile(many, np.int16)
    assert np.array_equal(a, b)
    # ONE stream of seed SEED indexed by the global frame number
    assert np.array_equal(a, gpu.Chain(**NRSC5).process(synth.hash_stream(n, seed, "cs16", 0)))


def test_harness_refuses_seamless_with_an_agc_option(gpu, tmp_path):
    r = subprocess.run([EXE, "--synthetic", "1000000", "--synthetic-hash", "1", *ARGS, "--shards", "2", "--seamless", "--agc-profile", "digital"],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "AGC" in r.stderr
