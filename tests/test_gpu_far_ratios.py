"""Resampling ratios beyond 2^+-5.5 on the device: chains with S = 6 .. 9 half-band stages in either direction.

iqgpu_chain_create accepts every ratio in [0.001, 1000]; the other GPU tests stop at S = 5.  A decimating chain with S >= 6 has
more leading stages than the wave kernels take (kCascMaxK) and runs on the generic workgroup kernel k_front: S + 1 level buffers in
LDS, groups of 64 .. 512 frames, warm-ups of many 2048-frame tiles, a `rem` carry that spans whole calls.  An interpolating one runs
k_interp with 32 .. 4 resampler outputs per tile, a rebuilt prefix (ext[0]) longer than the tile and bursts of 2^S frames per
resampler output.  Every case asserts what it covered (num_halfband_stages, interp, front_kernel()), so that a routing change
cannot make it pass on another kernel.

The synthetic stream has tones at -150, +30 and +200 kHz; the decimating cases shift the +30 kHz tone into their narrow output
band and assert that the oracle's output peaks at >= 0.2 of full scale: a comparison of noise around zero would prove nothing.

Bars (DESIGN.md "Parity contract"): cf32 max |delta| <= 1e-5; integer outputs +-1 LSB and >= 99.8 % identical codes.  For the
integer outputs of the interpolating cases the float32 accumulation itself costs about that much, so the bar there is derived from
the oracle: f = fraction of identical codes between its float-accumulator build and its double build on the same input, bar
min(0.998, f - 0.001), never below 0.995 (the margin because the kernel's summation order differs from both builds); the +-1 LSB
limit is unconditional.

Every comparison prints its figure before it asserts (pytest -s shows them); the figures measured on an MI355X are in DESIGN.md
section 1."""
import numpy as np
import pytest

from iq_tool_amd import synth

pytestmark = pytest.mark.gpu
TOL = 1e-5
SEED = 71

# name -> (S, description without the output format, frames, output formats of the parity test)
DOWN = {
    "D6": (6, dict(in_format="cs16", input_rate_hz=2.4e6, target_rate_hz=24e3, shift_hz=-27e3), 1 << 20, ("cs16", "cf32")),
    "D7": (7, dict(in_format="cs16", input_rate_hz=10e6, target_rate_hz=48e3, shift_hz=-25e3), 1 << 21, ("cs16", "cf32")),
    "D8": (8, dict(in_format="cu8", input_rate_hz=20e6, target_rate_hz=48e3, shift_hz=-25e3), 1 << 22, ("cu8", "cf32")),
    "D9": (9, dict(in_format="cs16", input_rate_hz=20e6, target_rate_hz=20.2e3, shift_hz=-28e3, dc_block=True), 1 << 22, ("cs16",)),
    "D9f": (9, dict(in_format="cf32", input_rate_hz=20e6, target_rate_hz=20.2e3, shift_hz=-28e3), 1 << 22, ("cf32",)),
}
UP = {
    "U6": (6, dict(in_format="cs16", input_rate_hz=24e3, target_rate_hz=2.4e6), 12000, ("cs16",)),
    "U6p": (6, dict(in_format="cs16", input_rate_hz=24e3, target_rate_hz=2.4e6, shift_hz=300e3, shift_after_resample=True), 12000, ("cf32",)),
    "U8": (8, dict(in_format="cu8", input_rate_hz=5e3, target_rate_hz=2.4e6), 3000, ("cs16",)),
    "U9": (9, dict(in_format="cs16", input_rate_hz=2.4e3, target_rate_hz=2.39e6), 1500, ("cf32",)),
}
CASES = dict(DOWN, **UP)
STAGE_M = {"D6": [3, 3, 3, 3, 5, 10], "D7": [3, 3, 3, 3, 3, 5, 10], "D8": [3] * 6 + [5, 10], "D9": [3] * 7 + [5, 10], "D9f": [3] * 7 + [5, 10]}
PARITY = [(name, fmt) for name in CASES for fmt in CASES[name][3]]
IN_BYTES = {"cu8": 2, "cs16": 4, "cf32": 8}


def cf(a):
    return np.ascontiguousarray(a).view(np.float32).view(np.complex64) if a.dtype != np.complex64 else a


def int_close(a, b, min_same, what):
    assert a.shape == b.shape, (a.shape, b.shape)
    d = np.abs(a.astype(np.int64) - b.astype(np.int64))
    same = float((d == 0).mean()) if d.size else 1.0
    print("%s: max code difference %d, %.5f of %d codes identical (bar %.4f)" % (what, int(d.max()) if d.size else 0, same, a.size, min_same))
    assert d.size and d.max() <= 1
    assert int((d != 0).sum()) <= max(3, int(np.ceil((1.0 - min_same) * a.size)))
    return same


def run_oracle(oracle, raw, L=None, **kw):
    kw = dict(kw)
    kw.pop("block_samples", None)
    return oracle.Chain(L=L, **kw).process(raw)


def frames(kw, raw, a, b):
    bpf = IN_BYTES[kw["in_format"]]
    return np.ascontiguousarray(raw).view(np.uint8)[a * bpf:b * bpf]


def desc(name, out_format):
    return dict(CASES[name][1], out_format=out_format)


# ---- every stream, every oracle output and every one-call device output is made once and shared; none of them is written to ----
_raw, _want, _fast, _one = {}, {}, {}, {}


def raw_of(kw, n):
    key = (kw["in_format"], kw["input_rate_hz"], n)
    if key not in _raw:
        _raw[key] = synth.raw_stream(n, kw["input_rate_hz"], SEED, kw["in_format"])
        _raw[key].setflags(write=False)
    return _raw[key]


def _key(kw, n):
    return (tuple(sorted(kw.items())), n)


def want_of(oracle, kw, n):
    k = _key(kw, n)
    if k not in _want:
        _want[k] = run_oracle(oracle, raw_of(kw, n), **kw)
        _want[k].setflags(write=False)
    return _want[k]


def float_build_fraction(oracle, kw, n):
    """f: identical codes between the oracle's float-accumulator build and its double build on this input"""
    k = _key(kw, n)
    if k not in _fast:
        a, b = run_oracle(oracle, raw_of(kw, n), L=oracle.lib(fast=True), **kw), want_of(oracle, kw, n)
        assert a.shape == b.shape
        d = np.abs(a.astype(np.int64) - b.astype(np.int64))
        assert d.max() <= 1
        _fast[k] = float((d == 0).mean())
    return _fast[k]


def check_routing(ch, name):
    """what the case covered: S, the direction and the kernel of the call the chain made last"""
    S, up = CASES[name][0], name in UP
    info = ch.info()
    assert int(info.num_halfband_stages) == S and bool(info.interp) == up, (name, int(info.num_halfband_stages), int(info.interp))
    if not up:
        assert [int(info.stage_m[g]) for g in range(S)] == STAGE_M[name], name
    assert ch.front_kernel() == ("k_front+k_interp" if up else "k_front"), (name, ch.front_kernel())
    return info


def one_call(gpu, name, out_format):
    k = (name, out_format)
    if k not in _one:
        kw, n = desc(name, out_format), CASES[name][2]
        ch = gpu.Chain(**kw)
        want_n = ch.next_out_frames(n)
        got = ch.process(raw_of(kw, n))
        assert got.size == 2 * want_n and want_n <= ch.max_out_frames(n)
        check_routing(ch, name)
        got.setflags(write=False)
        _one[k] = got
    return _one[k]


def integer_bar(oracle, name, kw, n):
    if name in DOWN:
        return 0.998
    f = float_build_fraction(oracle, kw, n)
    bar = max(0.995, min(0.998, f - 0.001))
    print("%s: oracle float build against double build f = %.5f -> bar %.5f" % (name, f, bar))
    return bar


def compare(oracle, name, kw, n, got, want, what):
    assert got.size == want.size and got.size > 0, (what, got.size, want.size)
    if kw["out_format"] == "cf32":
        err = float(np.abs(cf(got) - cf(want)).max())
        print("%s: max |delta| %.3g (bar %.0e), peak %.3f" % (what, err, TOL, float(np.abs(cf(want)).max())))
        assert float(np.abs(cf(want)).max()) < 1.0
        assert err <= TOL
    else:
        int_close(got, want, integer_bar(oracle, name, kw, n), what)


# --------------------------------------------------------------------------------------------
# 1. parity with the oracle, one call; 3. the count law
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,out_format", PARITY)
def test_one_call_matches_the_oracle(gpu, oracle, name, out_format):
    kw, n = desc(name, out_format), CASES[name][2]
    want = want_of(oracle, kw, n)
    if name in DOWN:
        # the +30 kHz tone (amplitude 0.25) is inside the output band
        if out_format == "cf32":
            peak = float(np.abs(cf(want)).max())
        elif out_format == "cu8":
            peak = float(np.abs(want.astype(np.float64) - 127.5).max()) / 127.5
        else:
            peak = float(np.abs(want.astype(np.float64)).max()) / 32767.0
        print("%s %s: oracle output peak %.3f of full scale, %d frames" % (name, out_format, peak, want.size // 2))
        assert peak >= 0.2
        assert want.size // 2 >= 4000 and n // 2048 >= 512
    else:
        assert want.size // 2 >= 580 * 2048
    got = one_call(gpu, name, out_format)
    compare(oracle, name, kw, n, got, want, "%s %s one call" % (name, out_format))


@pytest.mark.parametrize("name", sorted(CASES))
def test_count_law(gpu, oracle, name):
    S, _, n, fmts = CASES[name]
    kw = desc(name, fmts[0])
    total = one_call(gpu, name, fmts[0]).size // 2
    info = gpu.Chain(**kw).info()
    assert int(info.num_halfband_stages) == S
    if name in DOWN:
        law = -(-((n >> S) << 24) // int(info.arb_step))
    else:
        law = want_of(oracle, kw, n).size // 2
        assert total % (1 << S) == 0
    print("%s: %d frames in, %d out (law %d)" % (name, n, total, law))
    assert total == law
    assert total == gpu.design_out_frames(n, **kw)


# --------------------------------------------------------------------------------------------
# 2. any split gives the same bytes
# --------------------------------------------------------------------------------------------
def run_schedule(gpu, name, kw, raw, n, sizes):
    """a fresh chain over [0, n) in calls of the given sizes (the last one takes the rest): every call emits exactly what
    next_out_frames announced and no more than max_out_frames allows"""
    ch = gpu.Chain(**kw)
    outs, pos, counts = [], 0, []
    for k in list(sizes) + [None]:
        k = n - pos if k is None else k
        assert 0 < k <= n - pos
        ahead, cap = ch.next_out_frames(k), ch.max_out_frames(k)
        y = ch.process(frames(kw, raw, pos, pos + k))
        assert y.size == 2 * ahead, (name, pos, k, y.size // 2, ahead)
        assert ahead <= cap, (name, pos, k, ahead, cap)
        outs.append(y); counts.append(ahead)
        pos += k
    assert pos == n
    check_routing(ch, name)
    return np.concatenate(outs), counts


def decimating_schedule(S):
    return [1, (1 << S) - 1, 1, (1 << S) + 1, 3, 16384, 2047, 2049, 100000]


@pytest.mark.parametrize("name,out_format,extra", [
    ("D6", "cs16", {}), ("D8", "cu8", {}), ("D9f", "cf32", {}),
    ("U6", "cs16", {}), ("U6", "cs16", dict(block_samples=2048)), ("U9", "cf32", {})])
def test_any_split_gives_the_same_bytes(gpu, name, out_format, extra):
    S, _, n, _ = CASES[name]
    kw = desc(name, out_format)
    base = one_call(gpu, name, out_format)
    sizes = decimating_schedule(S) if name in DOWN else [1, 1, 2, 7, 1000]
    got, counts = run_schedule(gpu, name, dict(kw, **extra), raw_of(kw, n), n, sizes)
    print("%s %s %s: frames per call %s" % (name, out_format, extra, counts))
    if name in DOWN:
        assert counts[0] == 0                                   # one frame is less than a decimation group
        assert sum(sizes[:5]) < int(gpu.Chain(**kw).info().history_samples)   # ... and the first calls are shorter than the chain's history
    else:
        assert counts[0] > 0 and all(c % (1 << S) == 0 for c in counts)
    assert got.size == base.size
    assert np.array_equal(got.view(np.uint8), base.view(np.uint8)), (name, int((got != base).sum()), int(np.flatnonzero(got != base)[0]))


def test_split_of_the_dc_blocker_chain_is_within_one_code(gpu):
    """D9 carries the DC blocker: its per-run carry is a rounded closed form, so partitions differ in the last bit only
    (the rule of test_block_samples_does_not_change_results for DC chains)"""
    S, _, n, _ = CASES["D9"]
    kw = desc("D9", "cs16")
    base = one_call(gpu, "D9", "cs16")
    got, counts = run_schedule(gpu, "D9", kw, raw_of(kw, n), n, decimating_schedule(S))
    assert counts[0] == 0 and got.size == base.size
    d = np.abs(got.astype(np.int64) - base.astype(np.int64))
    print("D9 ragged schedule against one call: max code difference %d, %d of %d codes differ" % (int(d.max()), int((d != 0).sum()), d.size))
    assert d.max() <= 1


# --------------------------------------------------------------------------------------------
# 4. seek: a fresh chain put at frame a continues the stream byte for byte
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,out_format", [("D8", "cu8"), ("U6", "cs16")])
def test_seek_continues_the_stream_byte_for_byte(gpu, oracle, name, out_format):
    S, _, n, _ = CASES[name]
    kw = desc(name, out_format)
    p = gpu.design_preroll_frames(**kw)
    aligned = (p // 4096 + 2) * 4096
    ragged = aligned + 4096 + 37
    if n <= ragged + 65536:
        n = ragged + 65536 + 1                                  # (U6: the table's 12000 frames end in front of the seams)
    assert p > 0 and aligned > p and ragged + 65536 < n
    if name in DOWN:
        assert ragged % (1 << S) != 0
    raw = raw_of(kw, n)
    want = want_of(oracle, kw, n)
    for a in (aligned, ragged):
        ref = gpu.Chain(**kw)
        ref.process(frames(kw, raw, 0, a))
        y = ref.process(frames(kw, raw, a, n))
        ch = gpu.Chain(**kw)
        ch.seek(a, frames(kw, raw, a - p, a))
        g = ch.process(frames(kw, raw, a, n))
        print("%s seam %d (preroll %d): %s" % (name, a, p, ch.front_kernel()))
        check_routing(ch, name)
        check_routing(ref, name)
        assert g.size == y.size and g.size > 0
        assert np.array_equal(g.view(np.uint8), y.view(np.uint8)), (name, a, int((g != y).sum()), int(np.flatnonzero(g != y)[0]))
        first, count = gpu.design_out_frames_range(a, n - a, **kw)
        assert count * 2 == g.size and (first + count) * 2 == want.size
        compare(oracle, name, kw, n, g, want[first * 2:(first + count) * 2], "%s seam %d against the oracle's slice" % (name, a))


# --------------------------------------------------------------------------------------------
# 5. the output AGC on chunks of ~164 output frames (16384 input frames x 0.01)
# --------------------------------------------------------------------------------------------
AGC_FRAMES = 7_680_000                                          # 3.2 s: the digital profile locks at 2 s of output time


@pytest.mark.parametrize("out_format", ["cs16", "cf32"])
def test_digital_agc_on_very_short_chunks(gpu, oracle, out_format):
    kw = dict(desc("D6", out_format), agc=True, agc_profile="digital")
    n = AGC_FRAMES
    raw = raw_of(kw, n)
    och = oracle.Chain(**kw)
    want = och.process(raw)
    assert och.agc.locked
    ch = gpu.Chain(**kw)
    cut = 16384 * 200
    got = np.concatenate([ch.process(frames(kw, raw, 0, cut)), ch.process(frames(kw, raw, cut, n))])
    check_routing(ch, "D6")
    assert got.size == want.size and got.size // 2 == gpu.design_out_frames(n, **kw)
    if out_format == "cf32":
        err = float(np.abs(cf(got) - cf(want)).max())
        print("D6 digital AGC cf32: max |delta| %.3g (bar %.0e), peak %.3f" % (err, 20 * TOL, float(np.abs(cf(want)).max())))
        assert err <= 20 * TOL
    else:
        int_close(got, want, 0.995, "D6 digital AGC cs16")
    st = ch.agc_state()
    print("D6 digital AGC: gain %.7g, oracle %.7g, locked %s" % (st["gain"], och.agc.gain, st["locked"]))
    assert st["locked"]
    assert abs(st["gain"] - och.agc.gain) <= 1e-5 * och.agc.gain


def test_local_agc_on_very_short_chunks(gpu, oracle):
    kw = dict(desc("D6", "cf32"), agc=True, agc_profile="local")
    n = AGC_FRAMES
    raw = raw_of(kw, n)
    och = oracle.Chain(**kw)
    want = och.process(raw)
    ch = gpu.Chain(**kw)
    cuts = [0, 100000, 100000 + 16384, 3_000_000, n]
    got = np.concatenate([ch.process(frames(kw, raw, a, b)) for a, b in zip(cuts[:-1], cuts[1:])])
    check_routing(ch, "D6")
    assert got.size == want.size
    err, peak = float(np.abs(cf(got) - cf(want)).max()), float(np.abs(cf(want)).max())
    print("D6 local AGC cf32: max |delta| %.3g (bar %.3g), peak %.3f" % (err, 2e-5 * max(1.0, peak), peak))
    assert err <= 2e-5 * max(1.0, peak)
    st = ch.agc_state()
    print("D6 local AGC: gain %.7g, oracle %.7g" % (st["gain"], och.agc.gain))
    assert abs(st["gain"] - och.agc.gain) <= 1e-5 * och.agc.gain
    assert abs(st["peak_memory"] - och.agc.y2_prime) <= 1e-5 * och.agc.y2_prime
    assert st["samples_seen"] == och.agc.samples_seen
