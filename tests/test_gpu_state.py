"""Checkpoint / resume on the device (include/iqgpu.h): iqgpu_chain_save_state copies everything a chain carries from call to call
into a blob, iqgpu_chain_load_state puts it into a chain of the same description, and that chain continues the stream BYTE FOR BYTE
-- the same kernels on the same state in the same calls, so there is no tolerance anywhere in this file.

The yardstick is the unchanged ordinary path: ONE chain (A) processes the stream in calls; a second one (B) runs the calls in front
of a cut, saves and is destroyed; a fresh one (C) loads and runs the calls behind the cut, which must be A's bytes.  The shapes are
the scaled ones of the seek tests: the preset RATIOS at an input rate of 96 kHz, where the digital AGC's scan, lock, hang and creep
phases fall within 45 calls (the 2 s lock at 192 000 input frames, a fade at 10 s, the 4 s hang behind it, then the creep).  Every
call is 4 AGC chunks + 37 frames long, so at every cut the open decimation group, the resampler phase, the samples pending in front
of an FFT block and the chunk grid of the dx / local profiles are all in mid-stride, and the last AGC chunk of a call is 37 frames.

Every shape asserts the front kernel of its first call: the history layout that is saved is the specialised kernel's."""
import ctypes as C
import functools

import numpy as np
import pytest

from iq_tool_amd import synth

from shard_support import ECAPACITY, EHIP, EINVAL, EUNSUPPORTED, set_switches

pytestmark = pytest.mark.gpu
RATE = 96e3
K = RATE / 2.4e6                                # the 2.4 MS/s presets
K10 = RATE / 10e6                               # BASELINE configs[2]: 10 MS/s -> 2.4 MS/s
K61 = RATE / 61.44e6                            # BASELINE configs[3]: 61.44 MS/s -> 1.488375 MS/s
CHUNK = 16384
L = 4 * CHUNK + 37                              # frames per call
N_CALLS = 45
T_FADE, T_BURST, T_BURST_END = 10.0, 24.0, 24.5
# cuts are call indices: C starts with call k.  The locking chunk is the 37-frame chunk that starts at frame 196 682 (2.049 s): the
# last one of call 2; calls 15 .. 21 lie in the hang interval behind the fade, the gain creeps from 14 s on (call 21)
AGC_CUTS = dict(scanning=1, locking_chunk=2, locked=10, hang=17, creeping=25)
PLAIN_CUTS = dict(early=1, middle=5)
SWITCHES = ("FORCE_FAT", "FORCE_GENERIC", "NO_FAST", "AGC_NOFUSE", "FFT_NO_R16", "FFT_LOG2N")

NRSC5 = dict(in_format="cs16", out_format="cs16", input_rate_hz=RATE, target_rate_hz=744187.5 * K, shift_hz=200e3 * K)
CU8_NRSC5 = dict(in_format="cu8", out_format="cu8", input_rate_hz=RATE, target_rate_hz=1488375.0 * K)
USB = dict(in_format="cs16", out_format="cs16", input_rate_hz=RATE, target_rate_hz=744187.5 * K, agc=True,
           filters=(("passband", 158.5e3 * K, 113e3 * K),))
AM = dict(in_format="cs16", out_format="cs16", input_rate_hz=RATE, target_rate_hz=46511.71875 * K, agc=True)
INTERP = dict(in_format="cs16", out_format="cs16", input_rate_hz=RATE, target_rate_hz=2.4e6 * K * 1.2, shift_hz=150e3 * K)
# DC blocker + frozen I/Q factors + S = 2 + the 1025-tap FFT band-pass behind the resampler (block 2048)
CONFIG3 = dict(in_format="cs16", out_format="cs16", input_rate_hz=RATE, target_rate_hz=2.4e6 * K10, dc_block=True, iq_correct=True,
               iq_mag=0.013, iq_phase=-0.021, filters=(("passband", 158.5e3 * K10, 113e3 * K10),), filter_taps=1024)
# cu8, S = 5, the 4097-tap real FIR behind the resampler at its full length: a call emits 1588 frames, so the filter's history spans
# more than two calls
CONFIG4 = dict(in_format="cu8", out_format="cu8", input_rate_hz=RATE, target_rate_hz=1488375.0 * K61,
               filters=(("lowpass", 300e3 * K61, 0.0),), filter_taps=4097, filter_impl="fir")
PRE_FILTER = dict(in_format="cs16", out_format="cf32", input_rate_hz=RATE, no_resample=True, shift_hz=-250e3 * K,
                  filters=(("passband", -300e3 * K, 100e3 * K),), transition_width_hz=20e3 * K, attenuation_db=70.0,
                  filter_impl="fft", fft_size=2048)
POST_NCO = dict(NRSC5, shift_after_resample=True, out_format="cf32")
# name -> (description, IQGPU_<NAME> switches, calls, cuts, what the front kernel's name starts with after the FIRST call)
SHAPES = {
    "nrsc5_mid": (NRSC5, dict(FORCE_FAT="1"), 12, PLAIN_CUTS, "k_front_mid<6,nco>"),
    "cu8_nrsc5_p0": (CU8_NRSC5, dict(FORCE_FAT="1"), 12, PLAIN_CUTS, "k_front_p0"),
    "usb_filter_epilogue": (USB, dict(FORCE_FAT="1"), N_CALLS, AGC_CUTS, "k_front_mid<6,nonco,cf32>"),
    "am_cascade": (AM, {}, N_CALLS, AGC_CUTS, "k_cascade"),
    "interp": (INTERP, {}, 12, PLAIN_CUTS, "k_front+k_interp"),
    # (the first call starts on a decimation group, so it takes the fused two-stage kernel; the later ones, with an open group,
    #  k_cascade + k_front_s1: both write the histories that are saved)
    "config3_like": (CONFIG3, {}, 12, PLAIN_CUTS, "k_front_s2"),
    "config4_like": (CONFIG4, {}, 8, dict(early=1, middle=4), "k_cascade"),
    "no_resample_pre_filter": (PRE_FILTER, {}, 12, PLAIN_CUTS, "k_front"),
    "post_nco_cf32": (POST_NCO, {}, 12, PLAIN_CUTS, "k_front_s1"),          # (k_front_mid has no post NCO)
    "nrsc5_agc": (dict(NRSC5, agc=True), dict(FORCE_FAT="1"), N_CALLS, AGC_CUTS, "k_front_mid<6,nco"),
    # what the seek calls refuse
    "dc_agc": (dict(NRSC5, agc=True, dc_block=True), {}, N_CALLS, AGC_CUTS, "k_front_s1"),      # (k_front_mid has no DC blocker)
    "agc_local": (dict(NRSC5, agc=True, agc_profile="local"), dict(FORCE_FAT="1"), 12, PLAIN_CUTS, "k_front_mid<6,nco"),
    # (dx: every call costs the 260 000-sample warm-up of its chunks, ~50 ms: six calls.  Their 122 000 output frames stay below that
    #  window, so the blob holds a partly filled one)
    "agc_dx": (dict(NRSC5, agc=True, agc_profile="dx"), dict(FORCE_FAT="1"), 6, dict(early=1, middle=3), "k_front_mid<6,nco"),
}


@functools.lru_cache(maxsize=None)
def stream(fmt, seed=71):
    """N_CALLS calls of the synthetic stream under the envelope of the module docstring (frame times at 96 kHz)"""
    n = N_CALLS * L
    raw = synth.raw_stream(n, 2.4e6, seed, "cs16").astype(np.float64).reshape(-1, 2)
    env = np.full(n, 0.5)
    env[int(T_FADE * RATE):] = 0.15
    env[int(T_BURST * RATE):int(T_BURST_END * RATE)] = 0.65
    env[int(T_BURST_END * RATE):] = 0.5
    cs16 = np.clip(np.rint(raw * env[:, None]), -32768, 32767).astype(np.int16).reshape(-1)
    if fmt == "cu8":
        return ((cs16.astype(np.int32) >> 8) + 128).astype(np.uint8)
    return cs16


def call(x, i, j=None):
    """the frames of calls [i, j) of an interleaved stream (two components a frame in every input format used here)"""
    return x[2 * i * L:2 * (i + 1 if j is None else j) * L]


def raw_bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same(a, b):
    return a.dtype == b.dtype and a.size == b.size and np.array_equal(raw_bytes(a), raw_bytes(b))


_REF = {}


def reference(gpu, name, extra=()):
    """chain A, once per (shape, switches): the output of every call, tell() behind every call, the first call's front kernel.  The
    caller has set the switches."""
    key = (name, tuple(sorted(extra)))
    if key not in _REF:
        kw, _, n, _, _ = SHAPES[name]
        x = stream(kw["in_format"])
        a = gpu.Chain(**kw)
        outs, tells, first = [], [], None
        for i in range(n):
            outs.append(a.process(call(x, i)))
            tells.append(a.tell())
            first = first or a.front_kernel()
        a.close()
        _REF[key] = dict(outs=outs, tells=tells, first=first)
    return _REF[key]


def observe(ch, kw):
    """what the state calls report of a chain, every bit of it"""
    return (ch.tell(), bytes(ch.agc_state_raw()) if kw.get("agc") else None, ch.dc_state().tobytes() if kw.get("dc_block") else None)


def run_to_cut_and_save(gpu, kw, x, k, ref):
    """chain B: calls [0, k), the blob, what it reported at the save; destroyed"""
    b = gpu.Chain(**kw)
    for i in range(k):
        assert same(b.process(call(x, i)), ref["outs"][i])
    blob, seen = b.save_state(), observe(b, kw)
    assert seen[0] == ref["tells"][k - 1]
    b.close()
    return blob, seen


def continue_and_compare(c, kw, x, k, n, ref, what):
    for i in range(k, n):
        got = c.process(call(x, i))
        assert got.size == ref["outs"][i].size, (what, i, got.size, ref["outs"][i].size)        # frames_out of the call
        assert same(got, ref["outs"][i]), (what, "call %d" % i, int((raw_bytes(got) != raw_bytes(ref["outs"][i])).sum()))
        assert c.tell() == ref["tells"][i]


def continuation(gpu, name, ref, cuts=None):
    kw, _, n, shape_cuts, family = SHAPES[name]
    x = stream(kw["in_format"])
    print("%s: first call on %s, blob %d bytes" % (name, ref["first"], gpu.design_state_size(**kw)))
    assert ref["first"].startswith(family), (name, ref["first"])
    for what, k in sorted((cuts or shape_cuts).items(), key=lambda kv: kv[1]):
        blob, seen = run_to_cut_and_save(gpu, kw, x, k, ref)
        c = gpu.Chain(**kw)
        c.load_state(blob)
        assert observe(c, kw) == seen, (name, what)
        continue_and_compare(c, kw, x, k, n, ref, "%s cut %s" % (name, what))
        c.close()
    return x


# --------------------------------------------------------------------------------------------
# 1. continuation
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_a_loaded_chain_continues_the_stream_byte_for_byte(gpu, monkeypatch, name):
    kw, sw, n, cuts, _ = SHAPES[name]
    set_switches(monkeypatch, SWITCHES, sw)
    ref = reference(gpu, name, sw.items())
    assert sum(o.size for o in ref["outs"]) > 0 and ref["tells"][-1][0] == n * L
    x = continuation(gpu, name, ref)
    if cuts is AGC_CUTS and kw.get("agc_profile", "digital") == "digital":
        # the cuts stand where their names say: in front of the lock, with the locking chunk in the next call, locked, and the gain
        # that stood still through the hang interval creeps by the last one
        st = {}
        b = gpu.Chain(**kw)
        for i in range(max(cuts.values())):
            b.process(call(x, i))
            st[i + 1] = b.agc_state_raw()
        show = {w: (st[k].locked, st[k].current_gain) for w, k in cuts.items()}
        print("%s: (locked, gain) at the cuts %s" % (name, show))
        assert st[cuts["scanning"]].locked == 0 and st[cuts["locking_chunk"]].locked == 0 and st[cuts["locked"]].locked == 1
        if not kw.get("filters") and name != "am_cascade":
            # (behind a filter or the AM shape's ratio the 37-frame chunk may emit nothing, and an empty chunk locks nothing: there
            #  the lock falls into the call behind; the AM shape's creep starts inside the other shapes' hang interval)
            assert st[cuts["locking_chunk"] + 1].locked == 1
            assert st[cuts["creeping"]].current_gain > st[cuts["hang"]].current_gain == st[cuts["hang"] - 1].current_gain


# --------------------------------------------------------------------------------------------
# 2. save is invisible   3. the blob is a function of the state
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nrsc5_agc", "config3_like", "agc_local", "interp", "am_cascade"])
def test_a_chain_that_saves_after_every_call_writes_the_same_bytes(gpu, monkeypatch, name):
    kw, sw, n, _, _ = SHAPES[name]
    set_switches(monkeypatch, SWITCHES, sw)
    ref = reference(gpu, name, sw.items())
    x = stream(kw["in_format"])
    ch = gpu.Chain(**kw)
    n = min(n, 14)
    for i in range(n):
        assert same(ch.process(call(x, i)), ref["outs"][i]), (name, i)
        assert len(ch.save_state()) == ch.state_size()
    assert ch.tell() == ref["tells"][n - 1]


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_the_blob_is_a_deterministic_function_of_the_state(gpu, monkeypatch, name):
    kw, sw, n, _, _ = SHAPES[name]
    set_switches(monkeypatch, SWITCHES, sw)
    x = stream(kw["in_format"])
    k = min(n, 4)
    one, two = gpu.Chain(**kw), gpu.Chain(**kw)
    fresh = one.save_state()
    assert fresh == two.save_state() and gpu.state_inspect(fresh)["frames_in"] == 0
    for i in range(k):
        one.process(call(x, i))
    if not kw.get("filters"):
        # the twin gets there by another road: unrelated calls, then a reset (with a filter a reset keeps the samples pending in
        # front of an FFT block, which is another state: there the twin is fresh)
        two.process(call(x, 0, 2)[:2 * 50001])
        two.reset()
    for i in range(k):
        two.process(call(x, i))
    blob = one.save_state()
    assert blob == one.save_state()                            # twice in a row
    assert blob == two.save_state()                            # two chains, one state
    assert blob != fresh
    info = gpu.state_inspect(blob)
    print("%s: blob %d bytes, fingerprint %016x" % (name, len(blob), info["fingerprint"]))
    assert one.state_size() == gpu.design_state_size(**kw) == len(blob) == info["bytes"] and len(blob) % 16 == 0
    assert (info["frames_in"], info["frames_out"]) == one.tell() and info["frames_in"] == k * L and info["format_version"] == 1
    assert info["fingerprint"] == gpu.state_inspect(fresh)["fingerprint"]


# --------------------------------------------------------------------------------------------
# 4. batches in flight   6. pipelined continuation
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nrsc5_agc", "usb_filter_epilogue", "config3_like"])
def test_save_behind_batches_in_flight(gpu, monkeypatch, name):
    """three batches submitted and not collected: save runs them to their end first, so the blob is the one of a twin that processed
    the same three calls one by one; the tickets are collected afterwards as usual"""
    kw, sw, n, _, _ = SHAPES[name]
    set_switches(monkeypatch, SWITCHES, sw)
    ref = reference(gpu, name, sw.items())
    x = stream(kw["in_format"])
    a, twin = gpu.Chain(**kw), gpu.Chain(**kw)
    for i in range(4):                                         # (the digital AGC has locked by then: the batches run the fused path)
        a.process(call(x, i)), twin.process(call(x, i))
    cap = a.max_out_frames(L) * a.out_bytes
    slots = [(gpu.PinnedBuffer(L * a.in_bytes), gpu.PinnedBuffer(cap)) for _ in range(3)]
    flight = []
    for j, (ib, ob) in enumerate(slots):
        ib.array[:] = raw_bytes(call(x, 4 + j))
        flight.append(a.submit(ib.ptr, L, ob.ptr, cap))
    assert a.tell() == ref["tells"][6]                         # what submit has promised
    blob = a.save_state()
    for j in range(3):
        twin.process(call(x, 4 + j))
    assert blob == twin.save_state()
    for j, ((got, t), (_, ob)) in enumerate(zip(flight, slots)):
        a.collect(t)
        want = raw_bytes(ref["outs"][4 + j])
        assert got * a.out_bytes == want.size and np.array_equal(ob.array[:want.size], want), (name, j)
    assert same(a.process(call(x, 7)), ref["outs"][7])


@pytest.mark.parametrize("name", ["nrsc5_agc", "usb_filter_epilogue", "interp"])
def test_a_loaded_chain_continues_through_submit_and_collect(gpu, monkeypatch, name):
    kw, sw, n, cuts, _ = SHAPES[name]
    set_switches(monkeypatch, SWITCHES, sw)
    ref = reference(gpu, name, sw.items())
    x = stream(kw["in_format"])
    k, n = 3, min(n, 16)
    blob, _ = run_to_cut_and_save(gpu, kw, x, k, ref)
    c = gpu.Chain(**kw)
    c.load_state(blob)
    got = c.process_pipelined(call(x, k, n), L)
    want = np.concatenate(ref["outs"][k:n])
    assert same(got, want), (name, int((raw_bytes(got)[:want.nbytes] != raw_bytes(want)[:got.nbytes]).sum()))
    assert c.tell() == ref["tells"][n - 1]


# --------------------------------------------------------------------------------------------
# 5. the target need not be fresh
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nrsc5_agc", "config3_like", "agc_local", "am_cascade", "interp"])
def test_load_into_a_chain_that_has_run(gpu, monkeypatch, name):
    kw, sw, n, _, _ = SHAPES[name]
    set_switches(monkeypatch, SWITCHES, sw)
    ref = reference(gpu, name, sw.items())
    x = stream(kw["in_format"])
    k, n = 3, min(n, 12)
    blob, seen = run_to_cut_and_save(gpu, kw, x, k, ref)
    c = gpu.Chain(**kw)
    c.process(call(x, 7, 9)[:2 * 70001])                       # other data in other calls: every history, position word and
    c.process(call(x, 9)[:2 * 12345])                          # ping-pong index stands somewhere else
    c.load_state(blob)
    assert observe(c, kw) == seen
    continue_and_compare(c, kw, x, k, n, ref, name + " into a used chain")
    c.load_state(blob)                                         # ... and again, from behind the stream it has just continued
    continue_and_compare(c, kw, x, k, n, ref, name + " a second time")


def test_load_clears_a_poisoned_handle_and_save_refuses_one(gpu, monkeypatch):
    """The failure is a refusal on the HOST (test_gpu_seek.py: with the radix-16 transform switched off and a 16384-point transform
    asked for, launch_fftconv's own argument check turns the launch down), which poisons the handle.  Calls that emit no block never
    reach that check: the state that is loaded, and compared, is 100 frames pending in front of the block."""
    set_switches(monkeypatch, SWITCHES, dict(FFT_NO_R16="1", FFT_LOG2N="14"))
    kw = dict(in_format="cs16", out_format="cs16", input_rate_hz=2.4e6, no_resample=True, filters=(("lowpass", 300e3, 0.0),), filter_taps=129,
              filter_impl="fft")
    raw = synth.raw_stream(8192, 2.4e6, 57, "cs16")
    good = gpu.Chain(**kw)
    assert good.process(raw[:2 * 100]).size == 0
    blob = good.save_state()
    assert good.process(raw[2 * 100:2 * 150]).size == 0
    after = good.save_state()
    for reset_first in (False, True):
        ch = gpu.Chain(**kw)
        with pytest.raises(gpu.IqgpuError) as e:
            ch.process(raw)
        assert e.value.code == EHIP
        with pytest.raises(gpu.IqgpuError) as e:
            ch.save_state()
        assert e.value.code == EHIP and "reset" in str(e.value)
        if reset_first:
            ch.reset()
        ch.load_state(blob)
        assert ch.tell() == (100, 0) and ch.save_state() == blob
        assert ch.process(raw[2 * 100:2 * 150]).size == 0 and ch.save_state() == after


# --------------------------------------------------------------------------------------------
# 7. routing switches
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("switch", ["FORCE_GENERIC", "NO_FAST", "AGC_NOFUSE"])
@pytest.mark.parametrize("name", ["nrsc5_mid", "nrsc5_agc"])
def test_continuation_under_the_routing_switches(gpu, monkeypatch, name, switch):
    kw, _, n, cuts, _ = SHAPES[name]
    sw = {switch: "1"}
    set_switches(monkeypatch, SWITCHES, sw)
    ref = reference(gpu, name, sw.items())
    x = stream(kw["in_format"])
    print("%s under %s: first call on %s" % (name, switch, ref["first"]))
    assert ref["first"] == "k_front" if switch == "FORCE_GENERIC" else ref["first"].startswith("k_front")
    for what, k in sorted(cuts.items(), key=lambda kv: kv[1]):
        blob, seen = run_to_cut_and_save(gpu, kw, x, k, ref)
        c = gpu.Chain(**kw)
        c.load_state(blob)
        assert observe(c, kw) == seen
        continue_and_compare(c, kw, x, k, n, ref, "%s under %s cut %s" % (name, switch, what))


def test_a_blob_is_refused_under_another_switch_snapshot(gpu, monkeypatch):
    kw = SHAPES["nrsc5_agc"][0]
    x = stream("cs16")
    set_switches(monkeypatch, SWITCHES, {})
    saver = gpu.Chain(**kw)
    saver.process(call(x, 0))
    blob = saver.save_state()
    for sw in (dict(FORCE_GENERIC="1"), dict(NO_FAST="1"), dict(AGC_NOFUSE="1"), dict(FORCE_FAT="1")):
        set_switches(monkeypatch, SWITCHES, sw)
        other, twin = gpu.Chain(**kw), gpu.Chain(**kw)
        with pytest.raises(gpu.IqgpuError) as e:
            other.load_state(blob)
        assert e.value.code == EINVAL and "fingerprint" in str(e.value) and "switches" in str(e.value), sw
        assert same(other.process(call(x, 0)), twin.process(call(x, 0)))
    set_switches(monkeypatch, SWITCHES, {})
    gpu.Chain(**kw).load_state(blob)                           # the snapshot it was saved under takes it


# --------------------------------------------------------------------------------------------
# 8. the I/Q factors in force travel with the state
# --------------------------------------------------------------------------------------------
def test_iq_factors_set_mid_stream_are_restored(gpu, monkeypatch):
    kw, sw, n, _, _ = SHAPES["config3_like"]
    set_switches(monkeypatch, SWITCHES, sw)
    ref = reference(gpu, "config3_like", sw.items())
    x = stream("cs16")
    mag, phase = 0.031, 0.047

    def run(ch, lo, hi):
        outs = []
        for i in range(lo, hi):
            if i == 2:
                ch.set_iq_factors(mag, phase)
            outs.append(ch.process(call(x, i)))
        return outs

    a = gpu.Chain(**kw)
    want = run(a, 0, n)
    assert same(want[1], ref["outs"][1]) and not same(want[2], ref["outs"][2])       # the factors reach the output
    b = gpu.Chain(**kw)
    run(b, 0, 5)
    blob = b.save_state()
    b.close()
    c = gpu.Chain(**kw)                                        # created with the description's factors
    c.load_state(blob)
    got = run(c, 5, n)
    for i in range(5, n):
        assert same(got[i - 5], want[i]), i
    # ... and they are no part of the fingerprint: a chain described with other factors takes the blob and continues with the blob's
    d = gpu.Chain(**dict(kw, iq_mag=0.5, iq_phase=0.5))
    d.load_state(blob)
    assert same(d.process(call(x, 5)), want[5])


# --------------------------------------------------------------------------------------------
# 9. tell
# --------------------------------------------------------------------------------------------
def test_tell_and_seek_then_restore(gpu, monkeypatch):
    kw, sw, n, _, _ = SHAPES["nrsc5_mid"]
    set_switches(monkeypatch, SWITCHES, sw)
    ref = reference(gpu, "nrsc5_mid", sw.items())
    x = stream("cs16")
    fi = fo = 0
    for i in range(n):
        fi, fo = fi + L, fo + ref["outs"][i].size // 2
        assert ref["tells"][i] == (fi, fo)
    assert fo == gpu.design_out_frames(n * L, **kw)
    ch = gpu.Chain(**kw)
    assert ch.tell() == (0, 0)
    ch.process(call(x, 0))
    assert ch.tell() == ref["tells"][0]
    ch.reset()
    assert ch.tell() == (0, 0)
    # a seek puts the counters on the stream: first_frame and the index of the stream's output frame there
    a = 5 * L
    p = gpu.design_preroll_frames(**kw)
    ch.seek(a, x[2 * (a - p):2 * a])
    assert ch.tell() == (a, gpu.design_out_frames_range(a, L, **kw)[0]) == ref["tells"][4]
    # seek and restore agree: the sought chain's state, loaded into a fresh chain, continues the single stream
    blob = ch.save_state()
    assert gpu.state_inspect(blob)["frames_in"] == a
    c = gpu.Chain(**kw)
    c.load_state(blob)
    continue_and_compare(c, kw, x, 5, n, ref, "seek, save, load")
    continue_and_compare(ch, kw, x, 5, n, ref, "the sought chain itself")
    ch.seek(0)
    assert ch.tell() == (0, 0)


# --------------------------------------------------------------------------------------------
# 10. refusals: every one leaves the chain exactly as it was
# --------------------------------------------------------------------------------------------
def test_refusals_leave_the_chain_as_it_was(gpu, monkeypatch):
    name = "usb_filter_epilogue"
    kw, sw, n, _, _ = SHAPES[name]
    set_switches(monkeypatch, SWITCHES, sw)
    ref = reference(gpu, name, sw.items())
    x = stream("cs16")
    ch = gpu.Chain(**kw)
    for i in range(4):
        ch.process(call(x, i))
    blob = ch.save_state()
    size = len(blob)

    def other(**over):
        o = gpu.Chain(**dict(kw, **over))
        o.process(call(x, 0))
        return o.save_state()

    def patched(at, value):
        b = bytearray(blob)
        b[at:at + len(value)] = value
        return bytes(b)

    refused = {
        "another ratio": (other(target_rate_hz=kw["target_rate_hz"] * 1.01), "fingerprint"),
        "another output format": (other(out_format="cf32"), "fingerprint"),
        "another filter tap count": (other(filter_taps=64), "fingerprint"),
        "another AGC chunk": (other(agc_chunk_frames=8192), "fingerprint"),
        "no AGC": (other(agc=False), "fingerprint"),
        "truncated by a section": (blob[:-16], "truncated"),
        "truncated inside the header": (blob[:40], "header"),
        "empty": (b"", "header"),
        "a flipped byte in the body": (patched(size // 2, bytes([blob[size // 2] ^ 0x10])), "checksum"),
        "a flipped byte in the last word": (patched(size - 1, bytes([blob[size - 1] ^ 0x01])), "checksum"),
        "format_version 2": (patched(8, (2).to_bytes(4, "little")), "format_version"),
        "no magic": (patched(0, b"IQGPUST2"), "magic"),
    }
    at = 4
    for what, (bad, word) in refused.items():
        with pytest.raises(gpu.IqgpuError) as e:
            ch.load_state(bad)
        print("%s: %s" % (what, e.value))
        assert e.value.code == EINVAL and word in str(e.value), what
        if word == "fingerprint":                              # a sound blob, of another chain
            assert gpu.state_inspect(bad)["bytes"] == len(bad)
        else:
            with pytest.raises(gpu.IqgpuError):
                gpu.state_inspect(bad)
        # the chain continues with the bytes it would have written anyway
        assert same(ch.process(call(x, at)), ref["outs"][at]), what
        assert ch.tell() == ref["tells"][at]
        at += 1
    assert at <= n
    lib, h = ch._lib, ch._h
    buf, got = C.create_string_buffer(size), C.c_size_t(0)
    assert lib.iqgpu_chain_save_state(h, buf, size - 1, C.byref(got)) == ECAPACITY and got.value == size
    got.value = 0
    assert lib.iqgpu_chain_save_state(h, None, 0, C.byref(got)) == ECAPACITY and got.value == size         # the size query
    assert lib.iqgpu_chain_save_state(h, None, size, C.byref(got)) == EINVAL
    assert lib.iqgpu_chain_save_state(h, buf, size, None) == EINVAL
    assert lib.iqgpu_chain_load_state(h, None, size) == EINVAL
    a, b = C.c_uint64(0), C.c_uint64(0)
    assert lib.iqgpu_chain_tell(h, None, C.byref(b)) == EINVAL and lib.iqgpu_chain_tell(h, C.byref(a), None) == EINVAL
    assert same(ch.process(call(x, at)), ref["outs"][at])
    # the blob itself is still good, whatever was tried with it
    ch.load_state(blob)
    continue_and_compare(ch, kw, x, 4, 7, ref, "after the refusals")
    # a wall clock does not travel
    wall = gpu.Chain(**dict(kw, agc_clock="wall"))
    wall.process(call(x, 0))
    with pytest.raises(gpu.IqgpuError) as e:
        wall.save_state()
    assert e.value.code == EUNSUPPORTED and "WALL" in str(e.value)
    with pytest.raises(gpu.IqgpuError) as e:
        wall.load_state(blob)
    assert e.value.code == EINVAL
