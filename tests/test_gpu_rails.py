"""Saturating, rail-valued and non-finite samples through every fused kernel's own unpack and integer epilogue.

The other GPU tests feed synth.raw_stream (peak ~0.85 of full scale) or synth.hash_stream (quarter scale): no rail code goes into a
fused unpack, hardly any output reaches a clamp, no NaN or Inf enters a chain.  Here one case per kernel family (shapes and
IQGPU_<NAME> switch sets of test_gpu_seek.CASES, each asserting front_kernel()) runs four stimuli, every output in one call and in
one ragged three-way split (the same bytes; behind the overlap-save filter within one code, both held to the same checks):

 1. overdriven: synth.raw_stream through a chain gain of 2.5 and more;
 2. rails: every input component is one of {format minimum, 0 / mid code, format maximum}, drawn with a seeded generator;
 3. constant rails, no oracle: I = maximum code, Q = minimum code on every frame, gain 1.25, no shift -- behind the chain's memory
    every output frame IS (maximum code, minimum code) of the output format; then I and Q swapped;
 4. non-finite containment: one NaN frame and one +Inf frame in a cf32 stream damage only the outputs inside the chain's memory
    behind them; everything else is the clean stream's bytes, and reset() recovers: the chain then emits what a chain that never
    saw them emits after a reset.

The comparator of 1. and 2. takes the oracle's pre-pack float tap (oracle.Chain.process(raw, want_cf32=True)).  A component is
DECIDED when the tap, scaled as the format scales it, lies a whole code or more beyond the clamp value: that is more than the cf32
parity bar lets the device differ (1e-5 x amplitude 2 x 32767 = 0.66 code), so there the device code must EQUAL the rail code, no
exception.  Everywhere else the project's rule holds: never more than +-1 code apart, identical codes >= min(bar, f - 0.001) and
never below 0.99, with bar = 0.998 (0.995 behind a user filter) and f = identical codes between the oracle's float-accumulator
build and its double build on the same input -- taken over the same undecided components, since the decided ones agree trivially
and would only flatter it (the figure over all components is printed beside it).  Each stimulus is asserted to be hard before the
device runs: >= 10 % of the components decided, >= 10 % strictly inside the range.

What the kernels' own conditions make of the issue's table:
  * k_front_fat, k_front_p0 and k_cascade2 take chains with gain 1.0 only.  Stimuli 1 and 3 need a gain, so there the cu8_s0_p0
    and cascade2 shapes run -- and assert -- the kernels their routing falls back to (k_front_s1's S0 instantiation,
    k_cascade+k_front_s1); nrsc5_fat would fall back to k_front_mid's gain instantiation, which nrsc5_mid covers, and is left to
    stimulus 2.
  * at gain 1.0 independent draws leave most of their power outside a decimating chain's output band and the output never reaches
    a clamp.  So in stimulus 2 every drawn code is HELD for a few frames (HOLD: about the decimation ratio): the stream keeps unit
    scale, as the parity bars assume, and its power stays in band.  A raised gain instead would scale the float32 rounding noise
    with it.  sc16q11's 16-bit rails are |x| = 16: its gain is 1 / 16, for the same reason.
  * fft1025_behind's filter is a band-pass that none of the synthetic tones and no constant input passes.  The family here keeps
    the shape (10 MS/s -> 2.4 MS/s, 1025 taps, overlap-save blocks of 2048 behind the resampler) with a 500 kHz low-pass (the
    chain's -300 kHz shift puts the stream's 0 Hz inside it).
  * no DC blocker (a rail becomes IIR state) and no AGC (it rescales the signal away from the clamp).

Every case prints its kernel, its decided share, its identical-code share and f before it asserts (pytest -s shows them); the
figures measured on an MI355X are in DESIGN.md section 1."""
import numpy as np
import pytest

from iq_tool_amd import synth
from shard_support import set_switches
from test_gpu_seek import CASES as SEEK_CASES, SWITCHES

pytestmark = pytest.mark.gpu
TOL = 1e-5
SEED = 91

ALL_IN = ("cs16", "cu8", "cs8", "cu16", "sc16q11", "cs24", "cs32")
IN_BYTES = {"cu8": 2, "cs8": 2, "cs16": 4, "cu16": 4, "sc16q11": 4, "cs24": 6, "cs32": 8, "cf32": 8}
# output format -> (scale, offset, clamp low = minimum code, clamp high = maximum code): v = x * scale + offset
OUT = {"cs16": (32767.0, 0.0, -32768, 32767), "cs8": (127.0, 0.0, -128, 127),
       "cu8": (127.0, 127.5, 0, 255), "cu16": (32767.0, 32767.5, 0, 65535)}
# input format -> (minimum code, 0 / mid code, maximum code, numpy type of a component)
RAILS = {"cs16": (-32768, 0, 32767, np.int16), "sc16q11": (-32768, 0, 32767, np.int16), "cu16": (0, 32768, 65535, np.uint16),
         "cu8": (0, 128, 255, np.uint8), "cs8": (-128, 0, 127, np.int8),
         "cs24": (-8388608, 0, 8388607, None), "cs32": (-2147483648, 0, 2147483647, np.int32)}
LOWPASS_1025 = dict(filters=(("lowpass", 500e3, 0.0),), filter_taps=1024, filter_impl="fft")     # 1025 taps, FFT kind, block 2048


def _family(case, kernel, outs, rails_in=None, gain_kernel=None, hold=1, over_gain=2.5, filtered=False, **override):
    kw, sw, n, _, _ = SEEK_CASES[case]
    kw = dict(kw, **override)
    return dict(kw=kw, sw=sw, n=n, kernel=kernel, outs=outs, rails_in=rails_in or (kw["in_format"],), gain_kernel=gain_kernel,
                hold=hold, over_gain=over_gain, filtered=filtered)


S2_OR_TWO = ("k_front_s2", "k_cascade+k_front_s1")     # in front of the filter: either (the same bytes); the filter is the subject
# kernel: front_kernel() of the one-call run at gain 1.0 (ending in a comma: a prefix; a tuple: any of them); gain_kernel: ... of a chain with a gain (None: not run);
# outs: the family's native integer output format and one of cs16 / cu8 / cs8 / cu16 that test_gpu_seek.CASES does not give it;
# hold: frames a drawn rail code is held in stimulus 2; over_gain: the chain gain of stimulus 1
FAMILIES = {
    "nrsc5_s1": _family("nrsc5_s1", "k_front_s1", ("cs16", "cu8"), ALL_IN, "k_front_s1", hold=4, over_gain=3.5),
    "nrsc5_mid": _family("nrsc5_mid", "k_front_mid<6,", ("cs16", "cs8"), None, "k_front_mid<6,", hold=4, over_gain=3.5),
    "nrsc5_fat": _family("nrsc5_fat", "k_front_fat", ("cs16",), hold=4),
    "cu8_s0_p0": _family("cu8_s0_p0", "k_front_p0", ("cu8", "cs16"), None, "k_front_s1", hold=2),
    "s2": _family("s2", "k_front_s2", ("cs16", "cu16"), None, "k_front_s2", hold=6),
    "cascade2": _family("cascade2", "k_cascade2+k_front_s1", ("cs16", "cu8"), None, "k_cascade+k_front_s1", hold=48),
    "interp": _family("interp", "k_front+k_interp", ("cs16", "cu16"), None, "k_front+k_interp", hold=2),
    "generic": _family("generic", "k_front", ("cs16", "cs8"), ALL_IN, "k_front", hold=4, over_gain=3.5),
    "fft1025_behind": _family("fft1025_behind", S2_OR_TWO, ("cs16", "cu8"), None, S2_OR_TWO, hold=24, over_gain=4.0, filtered=True,
                              **LOWPASS_1025),
}


def frames(kw, raw, a, b):
    bpf = IN_BYTES[kw["in_format"]]
    return np.ascontiguousarray(raw).view(np.uint8)[a * bpf:b * bpf]


def three_way(n):
    """a ragged three-way split: both cuts odd"""
    a, b = (n // 3) | 1, ((2 * n) // 3 + 36) | 1
    return [a, b - a, n - b]


# ---- streams, oracle taps and one-call device outputs are made once, shared and never written to ----
_raw, _taps = {}, {}


def raw_of(kind, fmt, rate, n, hold=1):
    key = (kind, fmt, rate, n, hold)
    if key not in _raw:
        _raw[key] = synth.raw_stream(n, rate, SEED, fmt) if kind == "over" else rails_stream(n, fmt, SEED, hold)
        _raw[key].setflags(write=False)
    return _raw[key]


def rails_stream(n, fmt, seed, hold=1, const=None):
    """n frames whose every component is the format's minimum, 0 / mid or maximum code: drawn with a seeded generator and held
    for `hold` frames; or, with const = (i, q) (indices into RAILS[fmt]), the same two codes on every frame"""
    lo, mid, hi, dt = RAILS[fmt]
    codes = np.array([lo, mid, hi], np.int64)
    if const is not None:
        c = np.tile(codes[list(const)], n)
    else:
        pick = np.random.default_rng([int(seed), int(hold)]).integers(0, 3, size=(-(-n // hold), 2))
        c = np.repeat(codes[pick], hold, axis=0)[:n].reshape(-1)
    if fmt == "cs24":                                  # 3 little-endian bytes per component
        b = np.empty((c.size, 3), np.uint8)
        b[:, 0] = c & 0xff; b[:, 1] = (c >> 8) & 0xff; b[:, 2] = (c >> 16) & 0xff
        return b.reshape(-1)
    return c.astype(dt)


def oracle_desc(kw):
    kw = dict(kw)
    kw.pop("block_samples", None)
    ft = kw.get("filter_taps", 0)
    if ft and ft % 2 == 0:
        kw["filter_taps"] = ft + 1          # the odd bump of src/config.c:233-236, which make_desc applies on the product's side
    return kw


def taps_of(oracle, kw, raw, key):
    """(tap of the double build, tap of the float-accumulator build): the chain's output in front of the pack.  The tap does not
    depend on the output format: the codes of any format are oracle.from_cf32(tap, format), which is what the chain itself calls."""
    if key not in _taps:
        okw = oracle_desc(kw)
        codes, tap = oracle.Chain(**okw).process(raw, want_cf32=True)
        assert np.array_equal(codes, oracle.from_cf32(tap, okw["out_format"]))
        _, fast = oracle.Chain(L=oracle.lib(fast=True), **okw).process(raw, want_cf32=True)
        assert fast.size == tap.size and tap.size > 0
        tap.setflags(write=False); fast.setflags(write=False)
        _taps[key] = (tap, fast)
    return _taps[key]


def classify(tap, fmt):
    """(decided high, decided low, strictly inside the range) per component of the pre-pack tap"""
    scale, off, lo, hi = OUT[fmt]
    v = np.ascontiguousarray(tap).view(np.float32).astype(np.float64) * scale + off
    return v >= hi + 1.0, v <= lo - 1.0, (v > lo) & (v < hi)


def assert_stimulus_is_hard(tap, fmt, what):
    """on the CPU, from the oracle alone: the stimulus reaches the clamp AND leaves the rounding something to do"""
    up, down, inside = classify(tap, fmt)
    decided = float((up | down).mean())
    print("%s: %.4f of %d components decided (%.4f high, %.4f low), %.4f strictly inside the range"
          % (what, decided, up.size, float(up.mean()), float(down.mean()), float(inside.mean())))
    assert decided >= 0.10, (what, decided)
    assert float(inside.mean()) >= 0.10, (what, float(inside.mean()))
    assert up.any() and down.any(), what


def cf(a):
    return np.ascontiguousarray(a).view(np.float32).view(np.complex64)


def compare(oracle, got, tap, fast_tap, fmt, filtered, what):
    """THE comparator: device codes (or cf32 frames) against the oracle's pre-pack tap"""
    if fmt == "cf32":
        assert got.size == 2 * tap.size and tap.size > 0, (what, got.size, tap.size)
        scale = max(1.0, float(np.abs(tap).max()))
        err = float(np.abs(cf(got) - tap).max())
        print("%s: cf32 max |delta| %.3g (bar %.3g)" % (what, err, 2 * TOL * scale))
        assert err <= 2 * TOL * scale
        return
    lo, hi = OUT[fmt][2], OUT[fmt][3]
    want, fast = oracle.from_cf32(tap, fmt), oracle.from_cf32(fast_tap, fmt)
    assert got.size == want.size and got.dtype == want.dtype, (what, got.size, want.size, got.dtype, want.dtype)
    up, down, _ = classify(tap, fmt)
    rest = ~(up | down)
    assert (want[up] == hi).all() and (want[down] == lo).all() and (fast[up] == hi).all() and (fast[down] == lo).all(), what
    wrong = int((got[up] != hi).sum()) + int((got[down] != lo).sum())
    df = np.abs(fast.astype(np.int64) - want.astype(np.int64))
    assert df.max() <= 1, (what, int(df.max()))
    f, f_all = float((df[rest] == 0).mean()), float((df == 0).mean())
    bar = max(0.99, min(0.995 if filtered else 0.998, f - 0.001))
    d = np.abs(got.astype(np.int64) - want.astype(np.int64))
    same = float((d[rest] == 0).mean())
    print("%s: decided %.4f of %d components, %d of them off the rail; undecided: max code difference %d, identical %.5f "
          "(bar %.5f; f %.5f, over all components %.5f)"
          % (what, 1.0 - float(rest.mean()), d.size, wrong, int(d[rest].max()), same, bar, f, f_all))
    assert wrong == 0, (what, wrong, np.flatnonzero((up & (got != hi)) | (down & (got != lo)))[:8])
    assert d[rest].max() <= 1, (what, int(d[rest].max()))
    assert int((d[rest] != 0).sum()) <= max(3, int(np.ceil((1.0 - bar) * int(rest.sum())))), (what, same, bar)


def kernel_is(ch, prefix):
    name = ch.front_kernel()
    if isinstance(prefix, tuple):
        assert name in prefix, (name, prefix)
    else:
        assert name == prefix or (prefix.endswith(",") and name.startswith(prefix)), (name, prefix)
    return name


def run_device(gpu, kw, raw, n, kernel, what, info_check=None):
    """(one call, asserting the kernel it took; the ragged three-way split): the same bytes -- except behind the overlap-save
    filter, whose transform windows start at each call's first sample, so that another schedule rounds a few sums the other way:
    there never more than one code apart, and the caller holds both outputs to the same checks"""
    ch = gpu.Chain(**kw)
    one = ch.process(raw)
    name = kernel_is(ch, kernel)
    if info_check is not None:
        info_check(ch.info())
    ch = gpu.Chain(**kw)
    pos, parts = 0, []
    for k in three_way(n):
        parts.append(ch.process(frames(kw, raw, pos, pos + k))); pos += k
    assert pos == n
    split = np.concatenate(parts)
    differ = int((split.view(np.uint8) != one.view(np.uint8)).sum()) if split.size == one.size else -1
    print("%s: %s, %d frames in, %d out; three-way split %s: %d bytes differ" % (what, name, n, one.size // 2, three_way(n), differ))
    assert split.size == one.size and split.size > 0, (what, split.size, one.size)
    if info_check is None:
        assert differ == 0, (what, differ)
    else:
        assert np.abs(split.astype(np.int64) - one.astype(np.int64)).max() <= 1, what
    return one, split


def filter_check(fam):
    if not fam["filtered"]:
        return None

    def check(info):        # the overlap-save filter behind the resampler: 1025 taps in blocks of 2048
        assert (int(info.filter_post_resample), int(info.filter_ntaps), int(info.filter_block)) == (1, 1025, 2048)
        assert int(info.filter_impl) in (3, 4)                  # IQGPU_FI_FFT_SYMMETRIC / _ASYMMETRIC
    return check


# --------------------------------------------------------------------------------------------
# 1. overdriven: the synthetic stream through a chain gain
# --------------------------------------------------------------------------------------------
OVER = [(name, fmt) for name, fam in FAMILIES.items() if fam["gain_kernel"] for fmt in fam["outs"]]


@pytest.mark.parametrize("name,out_format", OVER)
def test_overdriven_chain_clamps_as_the_oracle(gpu, oracle, monkeypatch, name, out_format):
    fam = FAMILIES[name]
    n = fam["n"]
    kw = dict(fam["kw"], out_format=out_format, gain=fam["over_gain"])
    raw = raw_of("over", kw["in_format"], kw["input_rate_hz"], n)
    tap, fast = taps_of(oracle, dict(kw, out_format=fam["outs"][0]), raw, ("over", name))
    what = "%s overdriven x%.1f -> %s" % (name, kw["gain"], out_format)
    assert_stimulus_is_hard(tap, out_format, what)
    set_switches(monkeypatch, SWITCHES, fam["sw"])
    for i, got in enumerate(run_device(gpu, kw, raw, n, fam["gain_kernel"], what, filter_check(fam))[:2 if fam["filtered"] else 1]):
        compare(oracle, got, tap, fast, out_format, fam["filtered"], what + (", three-way split" if i else ""))


# --------------------------------------------------------------------------------------------
# 2. rails: every input component is the format's minimum, 0 / mid or maximum code
# --------------------------------------------------------------------------------------------
def _rails_cases():
    out = []
    for name, fam in FAMILIES.items():
        native = fam["kw"]["in_format"]
        out += [(name, native, fmt) for fmt in fam["outs"]]
        # the other input formats the family accepts, its two output formats in turn
        out += [(name, fi, fam["outs"][i % len(fam["outs"])]) for i, fi in enumerate(f for f in fam["rails_in"] if f != native)]
    return out


@pytest.mark.parametrize("name,in_format,out_format", _rails_cases())
def test_rail_codes_in_clamp_as_the_oracle(gpu, oracle, monkeypatch, name, in_format, out_format):
    fam = FAMILIES[name]
    n = fam["n"]
    kw = dict(fam["kw"], in_format=in_format, out_format=out_format, gain=1.0 / 16.0 if in_format == "sc16q11" else 1.0)
    raw = raw_of("rails", in_format, kw["input_rate_hz"], n, fam["hold"])
    lo, mid, hi, _ = RAILS[in_format]
    if in_format != "cs24":
        assert set(np.unique(raw).tolist()) == {lo, mid, hi}
    tap, fast = taps_of(oracle, dict(kw, out_format=fam["outs"][0]), raw, ("rails", name, in_format))
    what = "%s rails %s (held %d) -> %s" % (name, in_format, fam["hold"], out_format)
    assert_stimulus_is_hard(tap, out_format, what)
    set_switches(monkeypatch, SWITCHES, fam["sw"])
    for i, got in enumerate(run_device(gpu, kw, raw, n, fam["kernel"], what, filter_check(fam))[:2 if fam["filtered"] else 1]):
        compare(oracle, got, tap, fast, out_format, fam["filtered"], what + (", three-way split" if i else ""))


# --------------------------------------------------------------------------------------------
# 3. constant rails: exact by construction, no oracle, no tolerance
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,out_format", OVER)
def test_constant_rails_give_the_rail_codes(gpu, monkeypatch, name, out_format):
    """I = maximum code and Q = minimum code on every frame is the constant (g, -g), 1.24 <= g <= 1.25 at gain 1.25; the chain's
    gain at 0 Hz is 1 to within its filters' ripple (1e-3 at the resampler's 60 dB, less for the 1025-tap low-pass), so behind its
    memory every output is beyond +-1.2: (maximum code, minimum code) of the output format, every frame.  Then swapped."""
    fam = FAMILIES[name]
    n = fam["n"]
    kw = dict(fam["kw"], out_format=out_format, gain=1.25)
    kw.pop("shift_hz", None)
    fmt_in = kw["in_format"]
    lo, hi = OUT[out_format][2], OUT[out_format][3]
    memory = gpu.design_preroll_frames(**kw)
    first, count = gpu.design_out_frames_range(memory, n - memory, **kw)
    assert 0 < memory < n // 8 and count > 1000
    set_switches(monkeypatch, SWITCHES, fam["sw"])
    for const, (want_i, want_q) in (((2, 0), (hi, lo)), ((0, 2), (lo, hi))):
        raw = rails_stream(n, fmt_in, SEED, const=const)
        what = "%s constant %s (%s, %s) x1.25 -> %s" % (name, fmt_in, "max" if const[0] else "min", "max" if const[1] else "min", out_format)
        for got in run_device(gpu, kw, raw, n, fam["gain_kernel"], what, filter_check(fam)):
            assert got.size == 2 * (first + count), (what, got.size, first, count)
            tail = got[2 * first:].reshape(-1, 2)
            off = int((tail[:, 0] != want_i).sum()) + int((tail[:, 1] != want_q).sum())
            print("%s: memory %d frames, outputs from %d on: %d of %d codes off (%d, %d)" % (what, memory, first, off, tail.size, want_i, want_q))
            assert off == 0, (what, off, tail[np.flatnonzero((tail[:, 0] != want_i) | (tail[:, 1] != want_q))[:4]])


# --------------------------------------------------------------------------------------------
# 4. a NaN frame and a +Inf frame damage only the outputs inside the chain's memory behind them
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,out_format", [("nrsc5_s1", "cf32"), ("generic", "cs16"), ("fft1025_behind", "cs16")])
def test_non_finite_frames_stay_inside_the_chains_memory(gpu, oracle, monkeypatch, name, out_format):
    fam = FAMILIES[name]
    n = fam["n"]
    kw = dict(fam["kw"], in_format="cf32", out_format=out_format)
    clean = synth.complex_signal(n, kw["input_rate_hz"], SEED)
    assert np.isfinite(clean.view(np.float32)).all()
    p_nan, p_inf = n // 4 + 3, (3 * n) // 5 + 1
    dirty = clean.copy()
    dirty[p_nan] = complex(np.nan, np.nan)
    dirty[p_inf] = complex(np.inf, np.inf)
    memory = gpu.design_preroll_frames(**kw)
    block = 2048 if fam["filtered"] else 0
    out_at = lambda p: gpu.design_out_frames_range(p, 1, **kw)[0]
    spans = [(out_at(p), out_at(p + memory) + block) for p in (p_nan, p_inf)]
    total = gpu.design_out_frames(n, **kw)
    assert 0 < spans[0][0] < spans[0][1] < spans[1][0] < spans[1][1] < total, (spans, total)
    keep = np.ones(total, bool)
    for a, b in spans:
        keep[a:b + 1] = False
    assert keep.mean() > 0.9
    set_switches(monkeypatch, SWITCHES, fam["sw"])
    # calls that end a few frames behind each non-finite frame: it then sits in the history the next call starts from
    cuts = [0, p_nan + 5, p_inf + 16, n]

    def run(x, schedule):
        ch = gpu.Chain(**kw)
        y = np.concatenate([ch.process(frames(kw, x, a, b)) for a, b in zip(schedule[:-1], schedule[1:])])
        return ch, y.reshape(total, -1)

    ch, want = run(clean, [0, n])
    # what a chain that never saw a non-finite sample emits after a reset: the clean stream from frame 0 -- behind the
    # block-quantised filter with the last stream's pending samples (less than a block) in front, which reset() keeps queued as the
    # reference's does (src/filter.c:417-436), so there seek(0), which starts a stream, gives the clean bytes
    one_call = want.reshape(-1).copy()
    ch.reset()
    after_reset = ch.process(clean)
    if not fam["filtered"]:
        assert np.array_equal(after_reset.view(np.uint8), one_call.view(np.uint8))
    name_k = kernel_is(ch, fam["kernel"])
    if fam["filtered"]:
        filter_check(fam)(ch.info())
    tap, fast = taps_of(oracle, dict(kw, out_format=fam["outs"][0]), clean, ("clean", name))
    compare(oracle, want.reshape(-1), tap, fast, out_format, fam["filtered"], "%s clean cf32 stream -> %s" % (name, out_format))
    for schedule in ([0, n], cuts):
        if schedule is cuts:
            _, want = run(clean, schedule)                  # (the same chain on the clean stream in the same calls)
        ch, got = run(dirty, schedule)
        a, b = got.view(np.uint8)[keep], want.view(np.uint8)[keep]
        differ = int((a != b).any(axis=1).sum())
        touched = int((got.view(np.uint8) != want.view(np.uint8)).any(axis=1).sum())
        print("%s (%s) -> %s, calls %s: NaN at %d, +Inf at %d, memory %d: spans %s; %d output frames differ from the clean stream, "
              "%d of them outside the spans" % (name, name_k, out_format, schedule, p_nan, p_inf, memory, spans, touched, differ))
        assert differ == 0, (name, schedule, np.flatnonzero(keep)[np.flatnonzero((a != b).any(axis=1))[:8]])
        assert touched > 0                                   # (the frames did go through the chain)
        ch.reset()
        again = ch.process(clean)
        assert again.size == after_reset.size and np.array_equal(again.view(np.uint8), after_reset.view(np.uint8)), (name, schedule, again.size)
        ch.seek(0)
        again = ch.process(clean)
        assert again.size == one_call.size and np.array_equal(again.view(np.uint8), one_call.view(np.uint8)), (name, schedule, again.size)
