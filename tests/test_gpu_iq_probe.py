"""The I/Q optimiser's probe on the device: k_iq_probe (kernels.hip) -- a second implementation of unpack . gain -> [DC] -> [I/Q] ->
[pre-resampler NCO] -- and the host rules that decide which call's head it takes (include/iqgpu.h, iqgpu_chain_enable_iq_probe):

  1. read_iq_probe() is the pre-processed head of the first ORDINARY stream call (process, process_device, submit) of at least 1024
     frames since the previous read, with the I/Q factors that call used (a submitted batch: those at its submit());
  2. the preroll inside seek / seek_agc / seek_dc, and measure / measure_device / measure_submit / dc_measure*, neither take a block
     nor occupy the slot;
  3. reset(), every seek* and load_state() drop a staged or held block: None until the next qualifying call;
  4. a call shorter than 1024 frames leaves the slot alone.

References: a pure unpack . gain block is ops.convert_block_to_cf32 of the same frames, bit for bit (that entry point is pinned to
the reference's sample_convert.c by test_gpu_parity); everything with DC, I/Q or NCO is the oracle's no_resample, cf32-out chain on
the same stream (pre_processor_apply_chain), to the project's cf32 bar: TOL = 1e-5 times max(1, peak |want|).

Every stream is at most 16384 frames.  Every comparison prints its figure before it asserts (pytest -s shows them)."""
import functools

import numpy as np
import pytest

from iq_tool_amd import synth
from test_gpu_parity import FORMATS, TOL

pytestmark = pytest.mark.gpu

RATE = 2.4e6
N = 16384
SEED = 23
SHIFT = 0.21 * RATE
# a stream cut into ragged calls: blocks are taken on calls 1, 2, 3 and 5 (0-based 0, 1, 2, 4); the 1023-frame call takes none
CALLS = (1024, 4097, 1500, 1023, 8192)
STARTS = tuple(int(v) for v in np.cumsum((0,) + CALLS[:-1]))
# the resamplers behind the pre-processing: name -> (target rate, IQGPU_<NAME> switches, front_kernel() of every call of CALLS).
# 2.4 MS/s -> 744187.5 has one half-band stage, -> 250 kS/s three; calls this short stay off k_front_mid / k_front_s2.
SHAPES = {"s1": (744187.5, {}, "k_front_s1"), "s3": (250e3, {}, "k_cascade+k_front_s1"), "generic": (744187.5, dict(FORCE_GENERIC="1"), "k_front")}
INT_FORMATS = [f for f in FORMATS if f != "cf32"]
# the pre-processing switches, each alone and all together
SWITCHES = {
    "dc": dict(dc_block=True),
    "iq": dict(iq_correct=True, iq_mag=0.05, iq_phase=-0.05),
    "iq0": dict(iq_correct=True, iq_mag=0.0, iq_phase=0.0),
    "shift+": dict(shift_hz=+SHIFT),
    "shift-": dict(shift_hz=-SHIFT),
    "post": dict(shift_hz=+SHIFT, shift_after_resample=True),
    "all": dict(dc_block=True, iq_correct=True, iq_mag=0.05, iq_phase=-0.05, shift_hz=+SHIFT, gain=1.7),
}
ALL = SWITCHES["all"]


def cf(a):
    return np.ascontiguousarray(a).view(np.float32).view(np.complex64) if a.dtype != np.complex64 else a


@functools.lru_cache(maxsize=None)
def stream(fmt, kind="synth"):
    """N frames as bytes (read only): the synthetic stream, or the counter-hash stream that exercises every code bit"""
    raw = synth.hash_stream(N, SEED, fmt) if kind == "hash" else synth.raw_stream(N, RATE, SEED, fmt)
    b = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
    b.setflags(write=False)
    return b


def frames(raw, bpf, a, b):
    return raw[a * bpf:b * bpf]


def pre_kw(fmt, sw):
    """the oracle's chain that stops behind the pre-processor: no resampler, cf32 out; a shift behind the resampler is not its business"""
    kw = dict(in_format=fmt, out_format="cf32", input_rate_hz=RATE, target_rate_hz=RATE, no_resample=True)
    kw.update({k: v for k, v in sw.items() if k not in ("agc", "agc_chunk_frames")})
    if kw.pop("shift_after_resample", False):
        kw.pop("shift_hz")
    return kw


_want = {}


def want_of(oracle, fmt, sw, kind="synth"):
    """the single stream's pre-processed samples, computed once per (format, switches) and left unchanged"""
    key = (fmt, kind, tuple(sorted(sw.items())))
    if key not in _want:
        w = cf(oracle.Chain(**pre_kw(fmt, sw)).process(stream(fmt, kind)))
        assert w.size == N
        w.setflags(write=False)
        _want[key] = w
    return _want[key]


def close(got, want, what):
    assert got is not None, what + ": no block"
    peak = float(np.abs(want).max())
    err = float(np.abs(got - want).max())
    bar = TOL * max(1.0, peak)
    print("%s: max |delta| %.3g (bar %.3g, peak %.3f)" % (what, err, bar, peak))
    assert np.isfinite(err) and err <= bar, what


def take(ch, what=""):
    b = ch.read_iq_probe()
    assert b is not None, what + ": read_iq_probe() returned None"
    return b.copy()


def chain(gpu, fmt="cs16", target=SHAPES["s1"][0], out_format="cf32", **sw):
    ch = gpu.Chain(in_format=fmt, out_format=out_format, input_rate_hz=RATE, target_rate_hz=target, **sw)
    ch.enable_iq_probe()
    assert ch.read_iq_probe() is None
    return ch


# --------------------------------------------------------------------------------------------
# A. unpack . gain, bit for bit: every format of unpack_one, three gains
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gain", [1.0, 0.37, -2.5])
@pytest.mark.parametrize("fmt", FORMATS)
def test_unpack_and_gain_bit_for_bit(gpu, fmt, gain):
    from iq_tool_amd import ops
    raw = stream(fmt, "synth" if fmt == "cf32" else "hash")       # (hash_stream has no cf32)
    ch = chain(gpu, fmt, gain=gain)
    bpf = ch.in_bytes
    ch.process(frames(raw, bpf, 0, 2048))
    got = take(ch, fmt)
    want = ops.convert_block_to_cf32(frames(raw, bpf, 0, 1024), fmt, gain)
    assert np.abs(want).max() > 0.0
    assert np.array_equal(got.view(np.float32), want.view(np.float32)), (fmt, gain)
    # ... and at a stream position that is no multiple of anything (the chain's second call, 1025 frames)
    ch.process(frames(raw, bpf, 2048, 3073))
    got = take(ch, fmt)
    want = ops.convert_block_to_cf32(frames(raw, bpf, 2048, 3072), fmt, gain)
    assert np.array_equal(got.view(np.float32), want.view(np.float32)), (fmt, gain, "second call")


RAIL_CODES = {"cs8": (-128, 0, 127, np.int8), "cu8": (0, 128, 255, np.uint8), "cs16": (-32768, 0, 32767, np.int16),
              "cu16": (0, 32768, 65535, np.uint16), "sc16q11": (-32768, 0, 32767, np.int16), "cs24": (-8388608, 0, 8388607, None),
              "cs32": (-2147483648, 0, 2147483647, np.int32), "cu32": (0, 2147483648, 4294967295, np.uint32)}


def rail_frames(n, fmt):
    """n frames whose components are the format's minimum, mid and maximum codes only (every pair of them occurs)"""
    lo, mid, hi, dt = RAIL_CODES[fmt]
    c = np.array([lo, mid, hi], np.int64)[np.random.default_rng(SEED).integers(0, 3, 2 * n)]
    c[:18] = np.array([lo, mid, hi], np.int64)[np.array([(i, q) for i in range(3) for q in range(3)]).reshape(-1)]
    if fmt == "cs24":
        b = np.empty((c.size, 3), np.uint8)
        b[:, 0] = c & 0xff; b[:, 1] = (c >> 8) & 0xff; b[:, 2] = (c >> 16) & 0xff
        return b.reshape(-1)
    return c.astype(dt).view(np.uint8)


@pytest.mark.parametrize("fmt", INT_FORMATS)
def test_unpack_of_minimum_mid_and_maximum_codes(gpu, fmt):
    from iq_tool_amd import ops
    raw = rail_frames(1024, fmt)
    for gain in (1.0, -2.5):
        ch = chain(gpu, fmt, gain=gain)
        ch.process(raw)                                           # exactly 1024 frames
        got = take(ch, fmt)
        want = ops.convert_block_to_cf32(raw, fmt, gain)
        assert np.array_equal(got.view(np.float32), want.view(np.float32)), (fmt, gain)
        assert np.unique(want.real).size == 3 and np.unique(want.imag).size == 3


# --------------------------------------------------------------------------------------------
# B. each switch alone and all together, on ragged calls, in front of two resampler shapes
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("fmt", ["cs16", "cu8", "cs24"])
@pytest.mark.parametrize("case", sorted(SWITCHES))
def test_each_switch_on_ragged_calls(gpu, oracle, monkeypatch, case, fmt, shape):
    from iq_tool_amd import ops
    sw = SWITCHES[case]
    target, env, kernel = SHAPES[shape]
    monkeypatch.delenv("IQGPU_FORCE_GENERIC", raising=False)
    for k, v in env.items():
        monkeypatch.setenv("IQGPU_" + k, v)
    raw = stream(fmt)
    want = want_of(oracle, fmt, sw)
    ch = chain(gpu, fmt, target, **sw)
    bpf = ch.in_bytes
    held = None
    for k, (a, n) in enumerate(zip(STARTS, CALLS)):
        ch.process(frames(raw, bpf, a, a + n))
        assert ch.front_kernel() == kernel, (case, fmt, shape, k, ch.front_kernel())
        if n < 1024:
            # rule 4: the slot is left alone -- the held block stays, and the NEXT call's head is taken
            assert np.array_equal(ch.read_iq_probe(), held), (case, fmt, shape, k)
            continue
        held = take(ch, "call %d" % k)
        close(held, want[a:a + 1024], "%s %s %s call %d at frame %d" % (case, fmt, shape, k, a))
        if case == "iq0":
            # factors (0, 0): the unpacked samples themselves (values: 0 * re may turn a -0.0 into +0.0)
            assert np.array_equal(held, ops.convert_block_to_cf32(frames(raw, bpf, a, a + 1024), fmt, sw.get("gain", 1.0)))
    if "shift_hz" in sw and not sw.get("shift_after_resample"):
        # the case is about the mixer: the unmixed stream is far outside the bar
        plain = want_of(oracle, fmt, {k: v for k, v in sw.items() if k != "shift_hz"})
        assert np.abs(plain[STARTS[4]:STARTS[4] + 1024] - want[STARTS[4]:STARTS[4] + 1024]).max() > 1000 * TOL
    if sw.get("dc_block"):
        # ... and about the carried DC state: a blocker started at the fifth call is far outside the bar
        # (moduli: the mixer's phase at that position is not the point here)
        fresh = cf(oracle.Chain(**pre_kw(fmt, sw)).process(frames(raw, bpf, STARTS[4], STARTS[4] + 1024)))
        assert np.abs(np.abs(fresh) - np.abs(want[STARTS[4]:STARTS[4] + 1024])).max() > 100 * TOL


def test_probe_is_what_the_chain_itself_computes(gpu):
    """k_iq_probe against the chain's own kernels: a no_resample twin with cf32 output emits exactly the pre-processed stream (k_front:
    its DC blocker scans in double, the probe runs 1024 float steps from the float of that state)"""
    raw = stream("cs16")
    ch = chain(gpu, "cs16", **ALL)
    twin = gpu.Chain(in_format="cs16", out_format="cf32", input_rate_hz=RATE, no_resample=True, **ALL)
    for k, (a, n) in enumerate(zip(STARTS, CALLS)):
        ch.process(frames(raw, 4, a, a + n))
        own = cf(twin.process(frames(raw, 4, a, a + n)))
        assert own.size == n
        if n >= 1024:
            close(take(ch), own[:1024], "probe against the no_resample twin, call %d" % k)


def test_calls_of_exactly_1024_and_of_1023_frames(gpu, oracle):
    raw = stream("cs16")
    want = want_of(oracle, "cs16", ALL)
    ch = chain(gpu, "cs16", **ALL)
    ch.process(frames(raw, 4, 0, 1023))
    assert ch.read_iq_probe() is None                            # nothing taken, nothing staged
    ch.process(frames(raw, 4, 1023, 2047))                       # exactly 1024 frames, at an odd position
    b = take(ch)
    close(b, want[1023:2047], "the 1024-frame call at frame 1023")
    ch.process(frames(raw, 4, 2047, 3070))
    assert np.array_equal(ch.read_iq_probe(), b)
    ch.process(frames(raw, 4, 3070, 5000))
    close(take(ch), want[3070:4094], "the call behind the second 1023-frame call")


# --------------------------------------------------------------------------------------------
# C. entry points: the block is the one process() takes on the same data, and the oracle's to the bar
# --------------------------------------------------------------------------------------------
def process_blocks(gpu, raw, cuts, kw=None, **sw):
    """the blocks a twin chain takes through process() on calls raw[cuts[k]:cuts[k + 1]], read after every call (so that the slot is
    free for the next one; None for a call of less than 1024 frames)"""
    if kw is not None:
        ch = gpu.Chain(**kw)
        ch.enable_iq_probe()
    else:
        ch = chain(gpu, "cs16", **sw)
    out = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        ch.process(frames(raw, ch.in_bytes, a, b))
        out.append(take(ch) if b - a >= 1024 else None)
    return out


def test_process_device_takes_the_block_process_takes(gpu, oracle):
    raw = stream("cs16")
    want = want_of(oracle, "cs16", ALL)
    cuts = list(STARTS) + [STARTS[-1] + CALLS[-1]]
    twin = process_blocks(gpu, raw, cuts, **ALL)
    ch = chain(gpu, "cs16", out_format="cs16", **ALL)
    cap = ch.max_out_frames(max(CALLS)) * ch.out_bytes
    d_out = gpu.DeviceBuffer(cap)
    held = None
    for k, (a, n) in enumerate(zip(STARTS, CALLS)):
        d_in = gpu.DeviceBuffer(n * 4)                            # (every call at an aligned address, as process() stages it)
        d_in.upload(frames(raw, 4, a, a + n))
        ch.process_device(d_in.ptr, n, d_out.ptr, cap)
        blk = ch.read_iq_probe()                                  # waits for the staged copy: no synchronize() in front of it
        ch.synchronize()
        d_in.free()
        if n < 1024:
            assert twin[k] is None and np.array_equal(blk, held)
            continue
        held = blk.copy()
        assert np.array_equal(held, twin[k]), k
        close(held, want[a:a + 1024], "process_device call %d" % k)
    d_out.free()


class Batch:
    def __init__(self, gpu, ch, raw, a, b):
        self.a, self.n = a, b - a
        self.inp = gpu.chain.PinnedBuffer(self.n * ch.in_bytes)
        self.inp.array[:] = frames(raw, ch.in_bytes, a, b)
        self.cap = ch.max_out_frames(self.n) * ch.out_bytes
        self.out = gpu.chain.PinnedBuffer(self.cap)
        self.ticket = None

    def submit(self, ch):
        _, self.ticket = ch.submit(self.inp.ptr, self.n, self.out.ptr, self.cap)
        return self


def test_submit_block_of_batch_0_while_later_batches_are_in_flight(gpu, oracle):
    raw = stream("cs16")
    want = want_of(oracle, "cs16", ALL)
    cuts = [0, 2048, 6145, 9000, 16384]
    twin = process_blocks(gpu, raw, cuts, **ALL)
    ch = chain(gpu, "cs16", out_format="cs16", **ALL)
    b = [Batch(gpu, ch, raw, lo, hi).submit(ch) for lo, hi in zip(cuts[:-1], cuts[1:])]
    ch.collect(b[0].ticket)                                       # batches 1 .. 3 stay uncollected
    blk = take(ch, "batch 0")
    assert np.array_equal(blk, twin[0])
    close(blk, want[0:1024], "batch 0 of four submitted")
    # the slot is free again: the next batch to be launched gives the next block -- batch 1 unless the pipeline had launched it
    # already while the slot was taken; in either case a batch of THIS stream, at its own position
    for x in b[1:]:
        ch.collect(x.ticket)
    nxt = take(ch, "behind batch 0")
    at = [k for k in (1, 2, 3) if np.array_equal(nxt, twin[k])]
    print("block behind batch 0: of batch %s" % at)
    assert len(at) == 1
    close(nxt, want[cuts[at[0]]:cuts[at[0]] + 1024], "batch %d" % at[0])


def test_submit_block_carries_the_factors_of_its_own_batch(gpu, oracle):
    raw = stream("cs16")
    fa, fb, fc = (0.05, -0.05), (-0.03, 0.02), (0.5, 0.5)
    ch = chain(gpu, "cs16", out_format="cs16", **ALL)              # created with fa
    b0 = Batch(gpu, ch, raw, 0, 4096).submit(ch)
    ch.set_iq_factors(*fb)
    b1 = Batch(gpu, ch, raw, 4096, 8192).submit(ch)
    ch.set_iq_factors(*fc)                                        # what the chain holds while both batches run
    # the oracle's pre-processor with the factors changed where the stream's were
    o = oracle.Chain(**pre_kw("cs16", ALL))
    w0 = cf(o.process(frames(raw, 4, 0, 4096)))
    o.set_iq_factors(*fb)
    w1 = cf(o.process(frames(raw, 4, 4096, 8192)))
    ch.collect(b0.ticket)
    close(take(ch, "batch 0"), w0[:1024], "batch 0, factors as of its submit")
    ch.collect(b1.ticket)                                         # launched now, with the slot free
    blk = take(ch, "batch 1")
    close(blk, w1[:1024], "batch 1, factors as of its submit")
    # ... and not the ones the chain held while the batch ran
    o2 = oracle.Chain(**pre_kw("cs16", ALL))
    o2.process(frames(raw, 4, 0, 4096))
    o2.set_iq_factors(*fc)
    assert np.abs(blk - cf(o2.process(frames(raw, 4, 4096, 5120)))).max() > 0.01


def test_submit_first_qualifying_batch_wins(gpu, oracle):
    raw = stream("cs16")
    want = want_of(oracle, "cs16", ALL)
    cuts = [0, 1000, 3000, 5048, 9000]                            # batch 0 is too short; 1, 2 and 3 qualify
    ch = chain(gpu, "cs16", out_format="cs16", **ALL)
    b = [Batch(gpu, ch, raw, lo, hi).submit(ch) for lo, hi in zip(cuts[:-1], cuts[1:])]
    for x in b:
        ch.collect(x.ticket)
    blk = take(ch)
    close(blk, want[1000:2024], "the first batch of at least 1024 frames")
    assert np.array_equal(ch.read_iq_probe(), blk)                # one read frees the slot; nothing ran since
    twin = process_blocks(gpu, raw, cuts[:3], **ALL)
    assert twin[0] is None and np.array_equal(blk, twin[1])


# the NRSC-5 preset shape with the digital AGC, at a thousandth of its rates: time is samples / rate, so the 2 s lock falls inside a
# 16384-frame stream.  Chunks of 512 frames (the smallest the fused front kernel takes behind one half-band stage).
K_AGC = 1e-3
AGC_KW = dict(in_format="cs16", out_format="cs16", input_rate_hz=RATE * K_AGC, target_rate_hz=744187.5 * K_AGC, shift_hz=200e3 * K_AGC,
              iq_correct=True, iq_mag=0.05, iq_phase=-0.05, gain=1.7)
AGC_ON = dict(agc=True, agc_chunk_frames=512)


def agc_pre_want(oracle, raw):
    kw = dict(AGC_KW, out_format="cf32", target_rate_hz=AGC_KW["input_rate_hz"], no_resample=True)
    return cf(oracle.Chain(**kw).process(raw))


def test_fused_agc_chain_takes_the_head_of_the_whole_call(gpu, oracle):
    """process_device_impl cuts the call that holds the AGC's lock at the locking chunk: unfused kernels in front, the fused front
    kernel behind.  Call 2 below starts 2.03 s into the stream, so its first chunk locks and the cut falls 512 frames into it: no
    piece but the whole call decides whether and where the block is taken."""
    raw = stream("cs16")
    want = agc_pre_want(oracle, raw)
    cuts = [0, 4864, 8960, 13056]
    out_at = lambda n: gpu.design_out_frames_range(0, n, **AGC_KW)[1]      # (the closed form of the chain in front of its AGC)
    rate_out = AGC_KW["target_rate_hz"]
    assert out_at(4864 - 256) / rate_out <= 2.0 < out_at(4864) / rate_out      # no chunk of call 1 starts behind 2 s; call 2 does
    twin = process_blocks(gpu, raw, cuts, kw=AGC_KW)             # the chain without the AGC
    ch = gpu.Chain(**dict(AGC_KW, **AGC_ON))
    ch.enable_iq_probe()
    locked = []
    for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        ch.process(frames(raw, 4, a, b))
        blk = take(ch, "AGC chain call %d" % k)
        locked.append(ch.agc_state()["locked"])
        assert np.array_equal(blk, twin[k]), k                    # what the chain without the AGC takes
        close(blk, want[a:a + 1024], "AGC chain call %d (locked behind it: %s)" % (k, locked[-1]))
    assert locked == [False, True, True]


# --------------------------------------------------------------------------------------------
# D. calls that stay out (rule 2) and calls that drop the block (rule 3)
# --------------------------------------------------------------------------------------------
NO_DC = dict(iq_correct=True, iq_mag=0.05, iq_phase=-0.05, shift_hz=+SHIFT, gain=1.7)
FIRST, PREROLL = 6001, 3072                                   # (the shape's own memory is 2050 frames)


def test_seek_preroll_stays_out_and_the_held_block_is_dropped(gpu, oracle):
    raw = stream("cs16")
    want = want_of(oracle, "cs16", NO_DC)
    ch = chain(gpu, "cs16", **NO_DC)
    assert gpu.design_preroll_frames(in_format="cs16", out_format="cf32", input_rate_hz=RATE, target_rate_hz=SHAPES["s1"][0], **NO_DC) <= PREROLL
    ch.process(frames(raw, 4, 0, 2048))
    assert take(ch) is not None                                   # a block is held
    ch.process(frames(raw, 4, 2048, 4096))                        # ... and another one staged behind it
    ch.seek(FIRST, frames(raw, 4, FIRST - PREROLL, FIRST))        # a preroll of 3072 frames: long enough to be taken for a call
    assert ch.read_iq_probe() is None
    ch.process(frames(raw, 4, FIRST, FIRST + 2048))
    close(take(ch), want[FIRST:FIRST + 1024], "first call behind seek(%d)" % FIRST)
    # seek(0): no preroll at all; the block dropped all the same
    ch.seek(0)
    assert ch.read_iq_probe() is None
    ch.process(frames(raw, 4, 0, 1024))
    close(take(ch), want[0:1024], "first call behind seek(0)")


def test_seek_dc_preroll_stays_out_and_the_walked_state_shows(gpu, oracle):
    sw = dict(NO_DC, dc_block=True)
    raw = stream("cs16")
    want = want_of(oracle, "cs16", sw)
    ch = chain(gpu, "cs16", **sw)
    at = FIRST - PREROLL
    from iq_tool_amd.chain import DC_ROW
    rows = np.zeros(1, DC_ROW)
    rows[0] = ch.dc_measure(0, frames(raw, 4, 0, at))
    st, _ = ch.dc_advance(None, rows)
    assert ch.read_iq_probe() is None                             # dc_measure of 2929 frames took nothing
    ch.process(frames(raw, 4, 0, 2048))
    held = take(ch)
    ch.seek_dc(FIRST, frames(raw, 4, at, FIRST), 1024, st)        # the preroll in three calls of 1024 frames
    assert ch.read_iq_probe() is None
    ch.process(frames(raw, 4, FIRST, FIRST + 2048))
    blk = take(ch)
    assert not np.array_equal(blk, held)
    close(blk, want[FIRST:FIRST + 1024], "first call behind seek_dc(%d)" % FIRST)
    # the reference is sensitive to the state: a blocker that starts from zero at the preroll is far outside the bar
    zero = cf(oracle.Chain(**pre_kw("cs16", sw)).process(frames(raw, 4, at, FIRST + 1024)))[PREROLL:]
    assert np.abs(np.abs(zero) - np.abs(want[FIRST:FIRST + 1024])).max() > 100 * TOL


def test_seek_agc_preroll_stays_out(gpu, oracle):
    raw = stream("cs16")
    want = agc_pre_want(oracle, raw)
    ch = gpu.Chain(**dict(AGC_KW, agc=True))
    ch.enable_iq_probe()
    ch.process(frames(raw, 4, 0, 2048))
    assert take(ch) is not None
    ch.seek_agc(FIRST, frames(raw, 4, FIRST - PREROLL, FIRST))
    assert ch.read_iq_probe() is None
    ch.process(frames(raw, 4, FIRST, FIRST + 2048))
    close(take(ch), want[FIRST:FIRST + 1024], "first call behind seek_agc(%d)" % FIRST)


def test_measure_calls_leave_a_held_block_and_a_free_slot_alone(gpu, oracle):
    raw = stream("cs16")
    want = agc_pre_want(oracle, raw)
    ch = gpu.Chain(**dict(AGC_KW, agc=True))
    ch.enable_iq_probe()
    ch.process(frames(raw, 4, 0, 2048))
    held = take(ch)
    close(held, want[0:1024], "the held block")
    assert ch.measure(frames(raw, 4, 2048, 4096)).size == 1       # 2048 frames: would qualify
    assert np.array_equal(ch.read_iq_probe(), held)
    d_in = gpu.DeviceBuffer(2048 * 4)
    d_in.upload(frames(raw, 4, 4096, 6144))
    assert ch.measure_device(d_in.ptr, 2048).size == 1
    d_in.free()
    assert np.array_equal(ch.read_iq_probe(), held)
    inp, rows = gpu.chain.PinnedBuffer(2048 * 4), gpu.chain.PinnedBuffer(16)
    inp.array[:] = frames(raw, 4, 6144, 8192)
    got, ticket = ch.measure_submit(inp.ptr, 2048, rows.ptr, 1)
    ch.collect(ticket)
    assert got == 1 and np.array_equal(ch.read_iq_probe(), held)
    # the slot was free all along: the next ordinary call's head is taken
    ch.process(frames(raw, 4, 8192, 10240))
    close(take(ch), want[8192:9216], "the ordinary call behind three measuring calls")


def test_dc_measure_leaves_a_held_block_and_a_free_slot_alone(gpu, oracle):
    sw = dict(NO_DC, dc_block=True)
    raw = stream("cs16")
    want = want_of(oracle, "cs16", sw)
    ch = chain(gpu, "cs16", **sw)
    ch.process(frames(raw, 4, 0, 2048))
    held = take(ch)
    ch.dc_measure(2048, frames(raw, 4, 2048, 4096))
    d_in = gpu.DeviceBuffer(2048 * 4)
    d_in.upload(frames(raw, 4, 2048, 4096))
    ch.dc_measure_device(2048, d_in.ptr, 2048)
    d_in.free()
    assert np.array_equal(ch.read_iq_probe(), held)
    ch.process(frames(raw, 4, 2048, 4096))                        # dc_measure does not move the stream
    close(take(ch), want[2048:3072], "the ordinary call behind dc_measure")


@pytest.mark.parametrize("pending", [False, True])
def test_reset_drops_the_block(gpu, oracle, pending):
    sw = dict(NO_DC, dc_block=True)
    raw = stream("cs16")
    want = want_of(oracle, "cs16", sw)
    ch = chain(gpu, "cs16", **sw)
    ch.process(frames(raw, 4, 0, 4096))
    if not pending:
        assert take(ch) is not None                               # held; else: staged and never read
    ch.reset()
    assert ch.read_iq_probe() is None
    ch.process(frames(raw, 4, 0, 1023))
    assert ch.read_iq_probe() is None
    ch.process(frames(raw, 4, 1023, 3000))
    close(take(ch), want[1023:2047], "first qualifying call behind reset()")


@pytest.mark.parametrize("pending", [False, True])
def test_load_state_drops_the_block(gpu, oracle, pending):
    sw = dict(NO_DC, dc_block=True)
    raw = stream("cs16")
    want = want_of(oracle, "cs16", sw)
    twin = chain(gpu, "cs16", **sw)
    twin.process(frames(raw, 4, 0, 5001))
    blob = twin.save_state()
    ch = chain(gpu, "cs16", **sw)
    ch.process(frames(raw, 4, 0, 2048))
    if not pending:
        assert take(ch) is not None
    ch.load_state(blob)
    assert ch.read_iq_probe() is None
    ch.process(frames(raw, 4, 5001, 7049))
    close(take(ch), want[5001:6025], "first call behind load_state() at frame 5001")
    # the chain that saved goes on as if it had not been asked: its block is still the head of its own call
    close(take(twin), want[0:1024], "the saving chain's block")


# --------------------------------------------------------------------------------------------
# E. the closed loop on a second shape: cu8, DC blocker + I/Q correction + pre-resampler shift
# --------------------------------------------------------------------------------------------
def test_service_loop_on_a_cu8_dc_shift_chain(gpu, oracle):
    """test_service_loop_feeds_the_chain_like_the_reference_threads's loop (tests/test_iq_optimizer.py) with calls of 8192 frames:
    the two halves of one 16384-frame stream in turn, twelve calls, the stream clock stepped so that every call may run.  The
    oracle's pre-processor carries DC state and NCO phase over the whole stream, as the chain does."""
    n_call, calls = 8192, 12
    raw = stream("cu8")
    sw = dict(dc_block=True, iq_correct=True, shift_hz=+SHIFT)
    kw = dict(in_format="cu8", out_format="cf32", input_rate_hz=RATE, target_rate_hz=744187.5, **sw)
    g, o = gpu.Chain(**kw), oracle.Chain(**kw)
    pre = oracle.Chain(**pre_kw("cu8", sw))
    g.enable_iq_probe()
    go, oo = gpu.IqOptimizer(seed=11), oracle.IqOptimizer(seed=11)
    t = 10.0
    updates = 0
    for i in range(calls):
        seg = frames(raw, 2, (i % 2) * n_call, (i % 2 + 1) * n_call)
        a, b = cf(g.process(seg)), cf(o.process(seg))
        assert a.shape == b.shape and np.abs(a - b).max() <= TOL * max(1.0, float(np.abs(b).max())), i
        blk = cf(pre.process(seg))[:1024]                         # the reference's block: pre-processor output, this call's factors
        upd = go.service(g, t)
        if oo.run(blk, t):
            m, p = oo.factors()
            o.set_iq_factors(m, p); pre.set_iq_factors(m, p)
            assert upd
            updates += 1
        else:
            assert not upd
        (gm, gp), (om, op) = go.factors(), oo.factors()
        print("call %d: gpu (%.7f, %.7f) oracle (%.7f, %.7f)" % (i, gm, gp, om, op))
        assert max(abs(gm - om), abs(gp - op)) <= 2 * 0.05 * 1e-4 + 1e-7
        t += 0.65                                                 # every call may run (500 ms interval)
    assert updates >= calls - 1
