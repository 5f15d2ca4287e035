"""Seamless range sharding of chains with the digital output AGC (include/iqgpu.h, ABI v8): a measure pass yields one row per AGC
chunk (the peak in front of the gain, the chunk's frames), a walk over the rows in front of a seam yields the AGC state there, and
a chain put at the seam by seek_agc with that state continues the stream byte for byte.

Streams are cheap because time is samples_seen / target_rate: the preset RATIOS at an input rate of 96 kHz put the 2 s lock at
192 000 input frames and the 4 s hang at 384 000, so a stream of 45 calls of 65 536 frames (30.7 s) walks the whole state machine:
scanning, the locking chunk (the chunk that starts at frame 196 608 = 2.048 s), the locked phase, a fade to 0.3 of the level at
10 s (weak chunks: the hang interval until 14 s, then the gain creeps chunk by chunk), a burst at 24 s that ratchets.

The yardstick is the unchanged ordinary path: ONE chain processes the stream in calls of B frames.  Nothing here is compared with
what the new entry points say about themselves: states are compared with iqgpu_chain_get_agc_state of the ordinary chain, bytes
with the ordinary chain's bytes, peaks with the oracle's stream in front of the AGC.

Every comparison prints its figure before it asserts (pytest -s shows them)."""

import numpy as np
import pytest

from iq_tool_amd import synth

from shard_support import ECAPACITY, EINVAL, EUNSUPPORTED, fr, run, set_switches

pytestmark = pytest.mark.gpu
TOL = 1e-5
RATE = 96e3                                     # 2.4 MS/s scaled by 0.04: every preset ratio below is the preset's
K = RATE / 2.4e6
CHUNK = 16384
B = 4 * CHUNK                                   # frames per call
N_CALLS = 45
N = N_CALLS * B
T_FADE, T_BURST, T_BURST_END = 10.0, 24.0, 24.5
# seams, all on the call grid: in front of the lock, AT the locking chunk, locked, inside the hang interval, while the gain creeps,
# behind the ratchet
SEAMS = dict(scanning=2 * B, locking_chunk=3 * B, locked=10 * B, hang=17 * B, creeping=25 * B, behind_ratchet=38 * B)
SWITCHES = ("FORCE_FAT", "FAT", "NO_P0", "NO_S2", "FORCE_GENERIC", "AGC_NOFUSE", "NO_FAST", "NO_CASC2", "MEASURE_ROUTE")

NRSC5 = dict(in_format="cs16", out_format="cs16", input_rate_hz=RATE, target_rate_hz=744187.5 * K, shift_hz=200e3 * K, agc=True)
CU8_NRSC5 = dict(in_format="cu8", out_format="cu8", input_rate_hz=RATE, target_rate_hz=1488375.0 * K, agc=True)
USB = dict(in_format="cs16", out_format="cs16", input_rate_hz=RATE, target_rate_hz=744187.5 * K, agc=True,
           filters=(("passband", 158.5e3 * K, 113e3 * K),))
AM = dict(in_format="cs16", out_format="cs16", input_rate_hz=RATE, target_rate_hz=46511.71875 * K, agc=True)
INTERP = dict(in_format="cs16", out_format="cs16", input_rate_hz=RATE, target_rate_hz=2.4e6 * K * 1.2, shift_hz=150e3 * K, agc=True)
# name -> (description, IQGPU_<NAME> switches, what the front kernel's name starts with on the calls behind the lock)
ROUTINGS = {
    "nrsc5_cs16_mid": (NRSC5, dict(FORCE_FAT="1"), "k_front_mid"),
    "cu8_nrsc5_p0": (CU8_NRSC5, dict(FORCE_FAT="1"), "k_front_p0"),
    "usb_filter_epilogue": (USB, dict(FORCE_FAT="1"), "k_front_mid<6,nonco,cf32>"),
    "am_cascade": (AM, {}, "k_cascade"),
    "interp": (INTERP, {}, "k_front+k_interp"),
    "agc_nofuse": (NRSC5, dict(AGC_NOFUSE="1"), "k_front_s1"),
}


def stream(fmt, seed=61):
    """the synthetic stream under the envelope of the module docstring (frame times at 96 kHz)"""
    raw = synth.raw_stream(N, 2.4e6, seed, "cs16").astype(np.float64).reshape(-1, 2)
    env = np.full(N, 0.5)
    env[int(T_FADE * RATE):] = 0.15
    env[int(T_BURST * RATE):int(T_BURST_END * RATE)] = 0.65
    env[int(T_BURST_END * RATE):] = 0.5
    cs16 = np.clip(np.rint(raw * env[:, None]), -32768, 32767).astype(np.int16).reshape(-1)
    if fmt == "cu8":
        return ((cs16.astype(np.int32) >> 8) + 128).astype(np.uint8)
    return cs16


def no_agc(kw, **over):
    d = dict(kw, **over)
    d["agc"] = False
    return d


def state_bytes(st):
    return bytes(st)


def show(st):
    return dict(locked=st.locked, peak_memory=st.peak_memory, gain=st.current_gain, last_strong=st.last_strong_peak_time, seen=st.samples_seen)


def single_stream(gpu, kw, x, upto=N):
    """the ordinary path: one chain, calls of B frames; outputs per call and the AGC state behind every call"""
    ch = gpu.Chain(**kw)
    outs, states = [], {}
    for a in range(0, upto, B):
        outs.append(ch.process(fr(x, a, a + B)))
        if a + B in SEAMS.values() or a + B == upto:
            states[a + B] = ch.agc_state_raw()
    return ch, outs, states


def measured_table(gpu, kw, x, upto=N):
    """the measure pass over [0, upto) in the same calls: rows per call"""
    ch = gpu.Chain(**kw)
    return ch, [ch.measure(fr(x, a, a + B)) for a in range(0, upto, B)]


def cf(a):
    return np.ascontiguousarray(a).view(np.float32).view(np.complex64)


def int_close(a, b, min_same, what):
    assert a.shape == b.shape, (a.shape, b.shape)
    d = np.abs(a.astype(np.int64) - b.astype(np.int64))
    same = float((d == 0).mean()) if d.size else 1.0
    print("%s: max code difference %d, %.5f of %d codes identical (bar %.4f)" % (what, int(d.max()) if d.size else 0, same, a.size, min_same))
    assert d.size and d.max() <= 1
    assert int((d != 0).sum()) <= max(3, int(np.ceil((1.0 - min_same) * a.size)))


# --------------------------------------------------------------------------------------------
# 1. the table is exact
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ROUTINGS))
def test_walked_table_is_the_ordinary_chains_state(gpu, oracle, monkeypatch, name):
    kw, sw, _ = ROUTINGS[name]
    set_switches(monkeypatch, SWITCHES, sw)
    x = stream(kw["in_format"])
    _, _, states = single_stream(gpu, kw, x)
    m, per_call = measured_table(gpu, kw, x)
    rows = np.concatenate(per_call)
    assert rows.size == N // CHUNK and all(r.size == B // CHUNK for r in per_call)
    st, gains = m.agc_advance(m.agc_initial_state(), rows, gains=True)
    # the state machine went through every phase (the walk's own gains say so; they are checked against the ordinary output below
    # and in the seam test)
    t_of = lambda sec: int(sec * RATE) // CHUNK
    assert gains[t_of(20.0)] > gains[t_of(13.0)], "no creep behind the hang time"
    if name != "am_cascade":
        # (the AM shape's narrow output makes weak chunks the rule even in front of the fade: its last healthy chunk lies further
        #  back, so its creep starts inside what is the hang interval of the other shapes, and 1.3 times a weak chunk's peak stays
        #  below the ratchet threshold: that routing is here for its kernels, the other five for the whole state machine)
        assert gains[t_of(13.0)] == gains[t_of(10.5)], "no hang interval"
        assert gains[t_of(26.0)] < gains[t_of(23.0)], "no ratchet at the burst"
    for a in sorted(states):
        got = m.agc_advance(m.agc_initial_state(), rows[:a // CHUNK])
        print("%s frame %d: walked %s ordinary %s" % (name, a, show(got), show(states[a])))
        assert state_bytes(got) == state_bytes(states[a]), (name, a)
    # the walk does not depend on how the rows are grouped into calls of agc_advance
    st2 = m.agc_initial_state()
    for r in per_call:
        st2 = m.agc_advance(st2, r)
    assert state_bytes(st2) == state_bytes(st)
    # ... and the locking chunk is where the seam test puts its seam
    a = SEAMS["locking_chunk"]
    before = m.agc_advance(m.agc_initial_state(), rows[:a // CHUNK])
    after = m.agc_advance(before, rows[a // CHUNK:a // CHUNK + 1])
    assert before.locked == 0 and after.locked == 1

    # against the oracle's stream in front of the AGC: chunk lengths exactly, per-chunk peaks to the cf32 bar
    okw = no_agc(kw, out_format="cf32")
    want = cf(oracle.Chain(**okw).process(x))
    ends = [gpu.design_out_frames_range(0, (c + 1) * CHUNK, **okw)[1] for c in range(rows.size)]
    lens = np.diff([0] + ends)
    assert np.array_equal(rows["frames_out"], lens)
    worst = 0.0
    for c in range(rows.size):
        if lens[c]:
            pk = float(np.abs(want[ends[c] - lens[c]:ends[c]].astype(np.complex128)).max())
            worst = max(worst, abs(np.sqrt(rows["peak2"][c]) - pk))
    print("%s: per-chunk peaks against the oracle's pre-AGC stream, worst |delta| %.3g (bar %.0e)" % (name, worst, TOL))
    assert worst <= TOL


@pytest.mark.parametrize("name", sorted(ROUTINGS))
def test_walked_gains_are_the_gains_the_ordinary_path_applied(gpu, monkeypatch, name):
    """cf32 out: the ordinary chain's output is (the stream in front of the AGC) * gain[chunk], one float product per component;
    the stream in front of the AGC comes from the same chain without the AGC"""
    kw, sw, _ = ROUTINGS[name]
    kw = dict(kw, out_format="cf32")
    set_switches(monkeypatch, SWITCHES, sw)
    x = stream(kw["in_format"])
    _, outs, _ = single_stream(gpu, kw, x)
    y = np.concatenate(outs).view(np.float32)
    pre = gpu.Chain(**no_agc(kw))
    xin = np.concatenate([pre.process(fr(x, a, a + B)) for a in range(0, N, B)]).view(np.float32)
    m, per_call = measured_table(gpu, kw, x)
    rows = np.concatenate(per_call)
    _, gains = m.agc_advance(m.agc_initial_state(), rows, gains=True)
    assert y.size == xin.size == 2 * int(rows["frames_out"].sum())
    g = np.repeat(gains.astype(np.float32), 2 * rows["frames_out"].astype(np.int64))
    bad = int((y.view(np.uint32) != (xin * g).view(np.uint32)).sum())
    print("%s: %d of %d output components differ from pre-AGC * walked gain" % (name, bad, y.size))
    assert bad == 0
    # the peak of a row is the peak of those samples, bit for bit
    p2 = xin.astype(np.float64).reshape(-1, 2)
    p2 = p2[:, 0] * p2[:, 0] + p2[:, 1] * p2[:, 1]
    ends = np.cumsum(rows["frames_out"].astype(np.int64))
    want = np.array([p2[e - l:e].max() if l else 0.0 for e, l in zip(ends, rows["frames_out"])])
    assert np.array_equal(rows["peak2"].view(np.uint64), want.view(np.uint64))


@pytest.mark.parametrize("name", ["nrsc5_cs16_mid", "cu8_nrsc5_p0", "am_cascade"])
def test_both_routes_of_the_measure_pass_give_the_same_rows(gpu, monkeypatch, name):
    """k_front_s1<.., AGC> into a sink (the default of chains without a half-band stage) against the unfused route (the default of
    the others), each forced by the "measure_route" switch: calls on the chunk grid, then a ragged pair (an open group, a phase, a
    first chunk that starts inside a tile)"""
    kw, sw, _ = ROUTINGS[name]
    x = stream(kw["in_format"])
    set_switches(monkeypatch, SWITCHES, dict(sw, MEASURE_ROUTE="unfused"))
    a, per_a = measured_table(gpu, kw, x, 20 * B)
    set_switches(monkeypatch, SWITCHES, dict(sw, MEASURE_ROUTE="s1"))
    b, per_b = measured_table(gpu, kw, x, 20 * B)
    print("%s: measure on %s / %s" % (name, a.front_kernel(), b.front_kernel()))
    assert b.front_kernel().endswith("k_front_s1") and (name == "am_cascade" or a.front_kernel() != b.front_kernel())
    ra, rb = np.concatenate(per_a), np.concatenate(per_b)
    assert ra.size == rb.size == 20 * B // CHUNK and np.array_equal(ra.view(np.uint8), rb.view(np.uint8))
    cuts = [20 * B, 21 * B + 3 * CHUNK + 1235, 23 * B + 77, 24 * B]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        qa, qb = a.measure(fr(x, lo, hi)), b.measure(fr(x, lo, hi))
        assert qa.size == qb.size == -(-(hi - lo) // CHUNK) and np.array_equal(qa.view(np.uint8), qb.view(np.uint8)), (name, lo, hi)
    # ... and a chain that has measured that way processes on as any other: nothing of the ordinary path's AGC was touched
    set_switches(monkeypatch, SWITCHES, dict(sw, MEASURE_ROUTE="unfused"))
    ref = gpu.Chain(**kw)
    ref.measure(fr(x, 0, 24 * B))
    assert np.array_equal(b.process(fr(x, 24 * B, 28 * B)), ref.process(fr(x, 24 * B, 28 * B)))


def test_default_route_of_the_measure_pass_per_shape(gpu, monkeypatch):
    """the faster route measured per shape: k_front_s1<.., AGC> without a half-band stage, the unfused kernels with one"""
    for name, want in (("cu8_nrsc5_p0", "k_front_s1"), ("nrsc5_cs16_mid", "k_front_mid<6,nco,cf32>")):
        kw, sw, _ = ROUTINGS[name]
        set_switches(monkeypatch, SWITCHES, sw)
        ch = gpu.Chain(**kw)
        ch.measure(fr(stream(kw["in_format"]), 0, B))
        assert ch.front_kernel() == want, (name, ch.front_kernel())


# --------------------------------------------------------------------------------------------
# 2. seams are invisible
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ROUTINGS))
def test_seek_agc_continues_the_stream_byte_for_byte(gpu, monkeypatch, name):
    kw, sw, family = ROUTINGS[name]
    set_switches(monkeypatch, SWITCHES, sw)
    x = stream(kw["in_format"])
    ref, outs, _ = single_stream(gpu, kw, x)
    final = ref.agc_state_raw()
    p = gpu.design_preroll_frames(**no_agc(kw))
    m, per_call = measured_table(gpu, kw, x, max(SEAMS.values()))
    rows = np.concatenate(per_call)
    assert family and ref.front_kernel().startswith(family), ref.front_kernel()
    for what, a in sorted(SEAMS.items(), key=lambda kv: kv[1]):
        entry = m.agc_advance(m.agc_initial_state(), rows[:a // CHUNK])
        ch = gpu.Chain(**kw)
        pre = min(a, p)
        ch.seek_agc(a, fr(x, a - pre, a), entry)
        got = np.concatenate([ch.process(fr(x, b, b + B)) for b in range(a, N, B)])
        want = np.concatenate(outs[a // B:])
        first, count = gpu.design_out_frames_range(a, N - a, **no_agc(kw))
        assert got.size == want.size == 2 * count and count > 0
        diff = int((got.view(np.uint8) != want.view(np.uint8)).sum())
        print("%s seam %s at %d (preroll %d, entry %s): %s, %d differing bytes" % (name, what, a, pre, show(entry), ch.front_kernel(), diff))
        assert diff == 0, (name, what, int(np.flatnonzero(got != want)[0]))
        assert ch.front_kernel() == ref.front_kernel()
        assert state_bytes(ch.agc_state_raw()) == state_bytes(final)


def test_seek_agc_device_variant_longer_preroll_and_a_chain_that_has_run(gpu, monkeypatch):
    kw, sw, _ = ROUTINGS["nrsc5_cs16_mid"]
    set_switches(monkeypatch, SWITCHES, sw)
    x = stream("cs16")
    a, end = SEAMS["locked"], SEAMS["locked"] + 6 * B
    _, outs, _ = single_stream(gpu, kw, x, end)
    want = np.concatenate(outs[a // B:])
    m, per_call = measured_table(gpu, kw, x, a)
    entry = m.agc_advance(m.agc_initial_state(), np.concatenate(per_call))
    p = gpu.design_preroll_frames(**no_agc(kw))
    ch = gpu.Chain(**kw)
    ch.process(fr(x, 0, 5 * B + 777))                            # a chain that has run, mid-chunk: seek_agc resets first
    pre = fr(x, a - 3 * p - 5, a)
    buf = gpu.DeviceBuffer(pre.nbytes)
    buf.upload(pre)
    ch.seek_agc_device(a, buf.ptr, 3 * p + 5, entry)
    got = np.concatenate([ch.process(fr(x, b, b + B)) for b in range(a, end, B)])
    buf.free()
    assert np.array_equal(got, want)
    # entry None at frame 0 is a fresh chain
    ch.seek_agc(0)
    assert np.array_equal(ch.process(fr(x, 0, B)), outs[0])


# --------------------------------------------------------------------------------------------
# 3. DC blocker + AGC: the bars of the DC seek tests
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_format", ["cs16", "cf32"])
def test_dc_blocker_chain_with_agc_is_seamless_to_the_project_bars(gpu, out_format):
    """NRSC-5 cs16 with the DC blocker and the digital AGC (no shipped preset has the pair; the commented hd-radio-isolate example
    does).  The DC state behind a seek is approximate (iqgpu.h: <= 1e-6 of full scale behind the warm-up), so peaks, gains and
    samples are too: cf32 <= 1e-5, cs16 +-1 LSB with >= 99.8 % identical codes -- the bars test_gpu_seek.py uses for DC chains.
    Measured on an MI355X: preroll 23 159 frames; cf32 max |delta| 1.2e-7 / 4.7e-8 at the two seams; cs16 no
    differing code in 1 422 490 / 812 852."""
    kw = dict(NRSC5, out_format=out_format, dc_block=True)
    x = stream("cs16")
    _, outs, _ = single_stream(gpu, kw, x)
    p = gpu.design_preroll_frames(**no_agc(kw))
    m, per_call = measured_table(gpu, kw, x, max(SEAMS.values()))
    rows = np.concatenate(per_call)
    for what in ("locked", "creeping"):
        a = SEAMS[what]
        # the measuring chain of a shard starts behind a seek as well: rows [a0, a) from a chain that was put at a0
        a0 = SEAMS["scanning"]
        ms = gpu.Chain(**kw)
        ms.seek_agc(a0, fr(x, a0 - min(a0, p), a0))
        tail = np.concatenate([ms.measure(fr(x, b, b + B)) for b in range(a0, a, B)])
        entry = m.agc_advance(m.agc_initial_state(), np.concatenate([rows[:a0 // CHUNK], tail]))
        ch = gpu.Chain(**kw)
        pre = min(a, p)
        ch.seek_agc(a, fr(x, a - pre, a), entry)
        got = np.concatenate([ch.process(fr(x, b, b + B)) for b in range(a, N, B)])
        want = np.concatenate(outs[a // B:])
        assert got.size == want.size and got.size > 0
        if out_format == "cf32":
            err = float(np.abs(cf(got) - cf(want)).max())
            print("dc + agc seam %s at %d (preroll %d): max |delta| %.3g" % (what, a, pre, err))
            assert err <= TOL
        else:
            int_close(got, want, 0.998, "dc + agc seam %s at %d (preroll %d)" % (what, a, pre))


# --------------------------------------------------------------------------------------------
# 4. measure leaves the AGC alone and moves the stream
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nrsc5_cs16_mid", "usb_filter_epilogue", "interp"])
def test_measure_leaves_the_agc_state_and_advances_the_stream(gpu, monkeypatch, name):
    kw, sw, _ = ROUTINGS[name]
    kw = dict(kw, out_format="cf32")
    set_switches(monkeypatch, SWITCHES, sw)
    x = stream(kw["in_format"])
    a, b = 5 * B + 3 * CHUNK + 1234, 9 * B + 77                # ragged: an open group, a phase, samples pending in front of a block
    ch = gpu.Chain(**kw)
    ch.process(fr(x, 0, 2 * B))
    st0 = ch.agc_state_raw()
    ch.measure(fr(x, 2 * B, 3 * B))
    assert state_bytes(ch.agc_state_raw()) == state_bytes(st0)
    # position and histories: a fresh AGC chain measures [0, a) and processes [a, b); its twin without the AGC processes both.  The
    # first gives the second's samples times the gains of a fresh AGC over that call's own rows
    ch = gpu.Chain(**kw)
    ch.measure(fr(x, 0, a))
    assert state_bytes(ch.agc_state_raw()) == state_bytes(ch.agc_initial_state())
    y = ch.process(fr(x, a, b)).view(np.float32)
    twin = gpu.Chain(**no_agc(kw))
    twin.process(fr(x, 0, a))
    xin = twin.process(fr(x, a, b)).view(np.float32)
    m = gpu.Chain(**kw)
    m.measure(fr(x, 0, a))
    rows = m.measure(fr(x, a, b))
    _, gains = m.agc_advance(m.agc_initial_state(), rows, gains=True)
    assert y.size == xin.size == 2 * int(rows["frames_out"].sum()) and y.size > 0
    g = np.repeat(gains, 2 * rows["frames_out"].astype(np.int64))
    assert np.array_equal(y.view(np.uint32), (xin * g).view(np.uint32))


# --------------------------------------------------------------------------------------------
# 5. refusals
# --------------------------------------------------------------------------------------------
def test_refusals(gpu):
    x = stream("cs16")
    one = fr(x, 0, B)
    for profile in ("dx", "local"):
        ch = gpu.Chain(**dict(NRSC5, agc_profile=profile))
        for call in (lambda: ch.measure(one), lambda: ch.seek_agc(B, fr(x, 0, B)),
                     lambda: ch.agc_advance(ch.agc_initial_state(), np.zeros(1, gpu.chain.AGC_ROW))):
            with pytest.raises(gpu.IqgpuError) as e:
                call()
            assert e.value.code == EUNSUPPORTED and "digital" in str(e.value)
    ch = gpu.Chain(**dict(NRSC5, agc_clock="wall"))
    with pytest.raises(gpu.IqgpuError) as e:
        ch.measure(one)
    assert e.value.code == EUNSUPPORTED and "WALL" in str(e.value)
    with pytest.raises(gpu.IqgpuError) as e:
        ch.seek_agc(B, fr(x, 0, B))
    assert e.value.code == EUNSUPPORTED
    plain = gpu.Chain(**no_agc(NRSC5))
    for call in (lambda: plain.measure(one), lambda: plain.seek_agc(B, fr(x, 0, B)), plain.agc_initial_state):
        with pytest.raises(gpu.IqgpuError) as e:
            call()
        assert e.value.code == EINVAL and "no output AGC" in str(e.value)
    # a table that is too short, a preroll that is too short
    import ctypes as C
    ch = gpu.Chain(**NRSC5)
    # hand-made tables the walk cannot take: 64 rows that hold 2^31 frames, a negative peak, a NaN
    big = np.zeros(64, gpu.chain.AGC_ROW); big["frames_out"] = 1 << 25; big["peak2"] = 0.01
    for bad in (big, np.array([(-1.0, 100, 0)], gpu.chain.AGC_ROW), np.array([(np.nan, 100, 0)], gpu.chain.AGC_ROW)):
        with pytest.raises(gpu.IqgpuError) as e:
            ch.agc_advance(ch.agc_initial_state(), bad)
        assert e.value.code == EINVAL
    big["frames_out"][63] -= 1
    assert ch.agc_advance(ch.agc_initial_state(), big).samples_seen == (1 << 31) - 1
    rows = np.zeros(B // CHUNK - 1, gpu.chain.AGC_ROW)
    got = C.c_size_t(7)
    rc = ch._lib.iqgpu_chain_measure(ch._h, one.ctypes.data_as(C.c_void_p), B, rows.ctypes.data_as(C.c_void_p), rows.size, C.byref(got))
    assert rc == ECAPACITY and got.value == 0
    assert np.array_equal(ch.process(one), gpu.Chain(**NRSC5).process(one))       # ... and nothing was consumed
    p = gpu.design_preroll_frames(**no_agc(NRSC5))
    assert p > 1
    with pytest.raises(gpu.IqgpuError) as e:
        ch.seek_agc(10 * B, fr(x, 10 * B - (p - 1), 10 * B))
    assert e.value.code == EINVAL and "shorter" in str(e.value)
    assert np.array_equal(ch.process(one), gpu.Chain(**NRSC5).process(one))       # the chain is left reset
    # the v7 calls keep refusing AGC chains
    with pytest.raises(gpu.IqgpuError) as e:
        ch.seek(10 * B, fr(x, 10 * B - p, 10 * B))
    assert e.value.code == EUNSUPPORTED


# --------------------------------------------------------------------------------------------
# 6. the harness: --shards 4 --seamless-agc writes the file --shards 1 writes
# --------------------------------------------------------------------------------------------
HARNESS = {
    "nrsc5_cs16": (["--raw-file-input-rate", "96e3", "--raw-file-input-sample-format", "cs16", "--output-rate", "29767.5",
                    "--output-sample-format", "cs16", "--freq-shift", "8000"], "cs16", np.int16),
    "cu8_nrsc5": (["--raw-file-input-rate", "96e3", "--raw-file-input-sample-format", "cu8", "--output-rate", "59535",
                   "--output-sample-format", "cu8"], "cu8", np.uint8),
}


def check_report(info, shards, n, chunk):
    assert info["seamless_agc"] is True and info["shards"] == shards and info["frames_in"] == n
    grid = np.lcm.reduce([4096, CHUNK, chunk])
    at = 0
    for s, ps in enumerate(info["per_shard"]):
        assert ps["first_frame"] == at and ps["first_frame"] % grid == 0 and ps["frames_out"] == ps["planned_out"]
        assert ps["agc_rows"] == (-(-ps["frames_in"] // CHUNK) if s < shards - 1 else 0)
        assert ps["measure_seconds"] >= 0.0
        at += ps["frames_in"]
    assert at == n
    assert info["per_shard"][0]["entry"]["locked"] == 0 and info["per_shard"][-1]["entry"]["locked"] == 1
    seen = [ps["entry"]["samples_seen"] for ps in info["per_shard"]]
    assert seen[0] == 0 and seen == sorted(seen) and seen[1] > 0


@pytest.mark.parametrize("shape", sorted(HARNESS))
def test_harness_seamless_agc_synthetic_is_the_single_stream(gpu, tmp_path, shape):
    args, fmt, dt = HARNESS[shape]
    n, chunk = 3_000_003, 65536
    one, many = tmp_path / "one.raw", tmp_path / "many.raw"
    common = ["--synthetic", str(n), "--synthetic-hash", "40", *args, "--agc-profile", "digital", "--chunk-frames", str(chunk)]
    run(*common, "-o", str(one), "--shards", "1")
    info = run(*common, "-o", str(many), "--shards", "4", "--seamless-agc", "--devices", "1")
    check_report(info, 4, n, chunk)
    a, b = np.fromfile(one, dt), np.fromfile(many, dt)
    assert a.size == b.size == 2 * info["frames_out"] and a.size > 0
    diff = int((a != b).sum())
    print("%s: --shards 4 --seamless-agc against --shards 1, %d differing components of %d" % (shape, diff, a.size))
    assert diff == 0


def test_harness_seamless_agc_on_a_file_with_fade_and_burst(gpu, tmp_path):
    """the enveloped stream of the library tests from a file: shards that start in the locked phase and twice inside the creep, the
    last one with the ratchet burst in its own range"""
    args, _, _ = HARNESS["nrsc5_cs16"]
    x = stream("cs16")
    fin, one, many = tmp_path / "in.cs16", tmp_path / "one.cs16", tmp_path / "many.cs16"
    x.tofile(fin)
    common = ["-i", str(fin), *args, "--agc-profile", "digital", "--chunk-frames", str(B)]
    run(*common, "-o", str(one), "--shards", "1")
    info = run(*common, "-o", str(many), "--shards", "4", "--seamless-agc", "--devices", "1")
    check_report(info, 4, N, B)
    gains = [ps["entry"]["current_gain"] for ps in info["per_shard"]]
    assert gains[3] > gains[2] > gains[1] > 0                        # shards 2 and 3 start at 15.0 s and 22.5 s: inside the creep
    a, b = np.fromfile(one, np.int16), np.fromfile(many, np.int16)
    assert a.size == b.size and np.array_equal(a, b), int((a != b).sum())
    ch = gpu.Chain(**NRSC5)
    assert np.array_equal(a, np.concatenate([ch.process(fr(x, p, p + B)) for p in range(0, N, B)]))
