"""The measure pass of seamless AGC sharding through the pipeline (iqgpu_chain_measure_submit / iqgpu_chain_collect, ABI v9).

The yardstick is the unchanged synchronous call: two chains of one description are fed the same batches, one through
iqgpu_chain_measure, its twin through measure_submit, and everything the second yields -- rows, stream position, histories, the
bytes of what it processes afterwards -- is compared bit for bit with the first.  All chains run the digital profile on the sample
clock with agc_chunk_frames = 4096 (the harness case: its default of 16384, it has no option for it).

Every comparison prints its figure before it asserts (pytest -s shows them)."""
import ctypes as C

import numpy as np
import pytest

from iq_tool_amd import synth

from shard_support import ECAPACITY, EINVAL, EUNSUPPORTED, fr, run

pytestmark = pytest.mark.gpu
CHUNK = 4096
B = 3 * CHUNK
TAIL = 8192                                      # the process call behind the batches
SWITCHES = ("FORCE_FAT", "FAT", "NO_P0", "NO_S2", "FORCE_GENERIC", "AGC_NOFUSE", "NO_FAST", "NO_CASC2", "MEASURE_ROUTE")
# 11 batches on 8 slots: slots are reused; one ragged batch (the batches behind it start off the chunk grid, with an open
# decimation group and a phase) and one empty one
BATCHES = [B, B, B, B + 1000, B, B, 0, B, B, B, B]
T = sum(BATCHES)


def shapes(k):
    """the preset ratios at an input rate of k * 2.4 MS/s (time is samples_seen / target_rate: a low rate puts the 2 s lock early)"""
    nrsc5 = dict(in_format="cs16", out_format="cs16", input_rate_hz=2.4e6 * k, target_rate_hz=744187.5 * k, shift_hz=200e3 * k,
                 agc=True, agc_profile="digital", agc_clock="samples", agc_chunk_frames=CHUNK)
    return {
        "nrsc5_cs16": nrsc5,                                                                   # unfused route (k_front_mid family)
        "cu8_nrsc5": dict(nrsc5, in_format="cu8", out_format="cu8", target_rate_hz=1488375.0 * k, shift_hz=0.0),   # s1 route
        "nrsc5_fft_lowpass": dict(nrsc5, filters=(("lowpass", 100e3 * k, 0.0),), filter_taps=129, filter_impl="fft"),
        "nrsc5_dc_block": dict(nrsc5, dc_block=True),
    }


SHAPES = shapes(0.04)


@pytest.fixture(autouse=True)
def no_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv("IQGPU_" + k, raising=False)


def stream(fmt, n, seed=83):
    return synth.raw_stream(n, 2.4e6, seed, fmt)


def no_agc(kw):
    return dict(kw, agc=False)


def bits(rows):
    """peak2 as its 64-bit pattern, and frames_out"""
    return rows["peak2"].view(np.uint64).copy(), rows["frames_out"].copy()


def same_rows(a, b):
    return a.size == b.size and np.array_equal(bits(a)[0], bits(b)[0]) and np.array_equal(bits(a)[1], bits(b)[1])


class Batch:
    """one batch's pinned buffers: the input frames, and a table that starts as 0xff bytes"""

    def __init__(self, gpu, ch, frames, cap_rows=None, out_bytes=0):
        frames = np.ascontiguousarray(frames).view(np.uint8).reshape(-1)
        self.n = frames.size // ch.in_bytes
        self.cap = -(-self.n // CHUNK) if cap_rows is None else cap_rows
        self.inp = gpu.chain.PinnedBuffer(max(frames.size, 1))
        self.inp.array[:frames.size] = frames
        self.rows = gpu.chain.PinnedBuffer(max(self.cap, 1) * 16)
        self.rows.array[:] = 0xFF
        self.out = gpu.chain.PinnedBuffer(out_bytes) if out_bytes else None
        self.got = self.ticket = None

    def measure_submit(self, ch):
        self.got, self.ticket = ch.measure_submit(self.inp.ptr, self.n, self.rows.ptr, self.cap)
        assert self.got == -(-self.n // CHUNK)                  # exact when the call returns
        return self

    def submit(self, ch):
        self.got, self.ticket = ch.submit(self.inp.ptr, self.n, self.out.ptr, self.out.nbytes)
        return self

    def table(self):
        return self.rows.array[:self.got * 16].view(np.dtype([("peak2", np.float64), ("frames_out", np.uint32), ("reserved", np.uint32)])).copy()

    def output(self, ch):
        return self.out.array[:self.got * ch.out_bytes].copy()


def run_late(ch, batches, submit):
    """every batch submitted with the pipeline as full as it gets: the first eight without a collect, then one collect (the oldest
    ticket) in front of every further submit, the rest at the end -- each batch is collected at least seven submits after its own"""
    depth = ch._lib.iqgpu_chain_pipeline_depth()
    flight = []
    for b in batches:
        if len(flight) == depth:
            ch.collect(flight.pop(0).ticket)
        flight.append(submit(b))
    assert len(flight) == depth or len(batches) < depth
    for b in flight:
        ch.collect(b.ticket)


def cuts():
    at = np.concatenate([[0], np.cumsum(BATCHES)])
    return list(zip(at[:-1], at[1:]))


@pytest.fixture(scope="module")
def measured(gpu):
    """per shape: the stream, the synchronous chain and its rows per batch, the pipelined twin and its rows per batch -- computed
    once, then only read (the two chains are continued by the one test that says so)"""
    cache = {}

    def get(name):
        if name not in cache:
            kw = SHAPES[name]
            x = stream(kw["in_format"], T + TAIL)
            sync = gpu.Chain(**kw)
            want = [sync.measure(fr(x, a, b)) for a, b in cuts()]
            kernel_sync = sync.front_kernel()
            pipe = gpu.Chain(**kw)
            batches = [Batch(gpu, pipe, fr(x, a, b)) for a, b in cuts()]
            run_late(pipe, batches, lambda b: b.measure_submit(pipe))
            cache[name] = dict(kw=kw, x=x, sync=sync, pipe=pipe, want=want, got=[b.table() for b in batches],
                               kernels=(kernel_sync, pipe.front_kernel()))
        return cache[name]
    return get


# --------------------------------------------------------------------------------------------
# 1. the rows are the synchronous call's rows, bit for bit
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_rows_are_the_synchronous_calls_rows(gpu, measured, name):
    m = measured(name)
    print("%s: measure on %s / %s" % (name, *m["kernels"]))
    assert m["kernels"][0] == m["kernels"][1] and m["kernels"][0]
    if name == "cu8_nrsc5":
        assert m["kernels"][0].endswith("k_front_s1")             # the s1 route (the others: the chain's unfused kernels)
    total = 0
    for i, (n, want, got) in enumerate(zip(BATCHES, m["want"], m["got"])):
        assert want.size == got.size == -(-n // CHUNK), (name, i)
        bad = int((bits(want)[0] != bits(got)[0]).sum()) + int((bits(want)[1] != bits(got)[1]).sum())
        print("%s batch %d (%d frames): %d rows, %d differing fields" % (name, i, n, got.size, bad))
        assert bad == 0, (name, i)
        assert np.all(got["reserved"] == 0)
        total += int(got["frames_out"].sum())
    # the rows stand for the whole stream: their lengths add up to what the chain without the AGC emits for [0, T)
    assert total == gpu.design_out_frames_range(0, T, **no_agc(m["kw"]))[1] and total > 0
    assert np.concatenate(m["got"])["peak2"].max() > 0.0
    if name == "nrsc5_fft_lowpass":
        print("%s: frames_out per row %s" % (name, np.concatenate(m["got"])["frames_out"].tolist()))


# --------------------------------------------------------------------------------------------
# 2. the stream position and the histories advance identically
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_position_and_histories_advance_as_in_the_synchronous_call(gpu, measured, name):
    m = measured(name)
    kw, x, sync, pipe = m["kw"], m["x"], m["sync"], m["pipe"]
    tail = fr(x, T, T + TAIL)
    # no seek in between: both chains carry the fresh AGC state (measuring leaves it alone) and whatever position and histories
    # their 11 batches left
    assert bytes(sync.agc_state_raw()) == bytes(pipe.agc_state_raw()) == bytes(sync.agc_initial_state())
    a, b = sync.process(tail), pipe.process(tail)
    diff = int((a.view(np.uint8) != b.view(np.uint8)).sum()) if a.size == b.size else -1
    print("%s: %d frames processed behind the batches, %d differing bytes" % (name, a.size // 2, diff))
    assert a.size > 0 and diff == 0
    # ... and with the stream's AGC state there: the walk over each chain's own rows, installed by seek_agc at frame T behind its preroll
    p = min(T, gpu.design_preroll_frames(**no_agc(kw)))
    outs = []
    for ch, rows in ((sync, m["want"]), (pipe, m["got"])):
        entry = ch.agc_advance(ch.agc_initial_state(), np.concatenate(rows))
        ch.seek_agc(T, fr(x, T - p, T), entry)
        outs.append(ch.process(tail))
    assert outs[0].size > 0 and np.array_equal(outs[0].view(np.uint8), outs[1].view(np.uint8))
    if not kw.get("dc_block"):
        # (the DC state behind a seek is approximate, iqgpu.h; every other chain continues the ONE stream byte for byte)
        one = gpu.Chain(**kw)
        for lo, hi in cuts():
            one.process(fr(x, lo, hi))
        want = one.process(tail)
        diff = int((want.view(np.uint8) != outs[1].view(np.uint8)).sum()) if want.size == outs[1].size else -1
        print("%s: against the chain that processed the same calls, %d differing bytes of %d" % (name, diff, want.nbytes))
        assert diff == 0


# --------------------------------------------------------------------------------------------
# 3. process and measure batches mixed on one pipeline
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nrsc5_cs16", "cu8_nrsc5"])
def test_mixed_pipeline(gpu, name):
    """submit, measure_submit, submit, ... against process, measure, process, ... at a tenth of the other cases' rate: the lock
    (2 s of OUTPUT, which only process batches emit) falls into the second process batch, so the later ones run the fused AGC
    whose verdict the measure batch behind each has to see resolved"""
    kw = shapes(0.004)[name]
    n_batches = 12
    x = stream(kw["in_format"], n_batches * B, seed=84)
    twin, ch = gpu.Chain(**kw), gpu.Chain(**kw)
    want = [(twin.process if i % 2 == 0 else twin.measure)(fr(x, i * B, (i + 1) * B)) for i in range(n_batches)]
    assert twin.agc_state()["locked"]
    cap = ch.max_out_frames(B) * ch.out_bytes
    batches = [Batch(gpu, ch, fr(x, i * B, (i + 1) * B), out_bytes=cap if i % 2 == 0 else 0) for i in range(n_batches)]
    run_late(ch, batches, lambda b: b.submit(ch) if b.out is not None else b.measure_submit(ch))
    for i, (b, w) in enumerate(zip(batches, want)):
        if i % 2 == 0:
            got = b.output(ch)
            diff = int((got != w.view(np.uint8)).sum()) if got.size == w.nbytes else -1
            print("%s batch %d (process): %d bytes, %d differ" % (name, i, got.size, diff))
            assert got.size > 0 and diff == 0, (name, i)
        else:
            print("%s batch %d (measure): %d rows" % (name, i, b.got))
            assert same_rows(b.table(), w) and b.got == B // CHUNK, (name, i)
    assert bytes(ch.agc_state_raw()) == bytes(twin.agc_state_raw())


# --------------------------------------------------------------------------------------------
# 4. refusals touch nothing
# --------------------------------------------------------------------------------------------
def raw_measure_submit(ch, b, cap):
    got, ticket = C.c_size_t(7), C.c_uint64(7)
    rc = ch._lib.iqgpu_chain_measure_submit(ch._h, C.c_void_p(b.inp.ptr), b.n, C.c_void_p(b.rows.ptr), cap, C.byref(got), C.byref(ticket))
    return rc, got.value, ticket.value


def test_refusals_touch_nothing(gpu):
    kw = SHAPES["nrsc5_cs16"]
    x = stream("cs16", 11 * B, seed=85)
    twin, ch = gpu.Chain(**kw), gpu.Chain(**kw)
    want = [twin.measure(fr(x, i * B, (i + 1) * B)) for i in range(10)]
    b = [Batch(gpu, ch, fr(x, i * B, (i + 1) * B)) for i in range(10)]
    # a table one row short
    rc, got, ticket = raw_measure_submit(ch, b[0], B // CHUNK - 1)
    assert rc == ECAPACITY and got == 0 and ticket == 0 and b"rows" in ch._lib.iqgpu_last_error()
    assert np.all(b[0].rows.array == 0xFF)
    ch.collect(b[0].measure_submit(ch).ticket)
    assert same_rows(b[0].table(), want[0])
    # a ninth batch with eight in flight
    for i in range(1, 9):
        b[i].measure_submit(ch)
    rc, got, ticket = raw_measure_submit(ch, b[9], b[9].cap)
    assert rc == EINVAL and got == 0 and ticket == 0 and b"in flight" in ch._lib.iqgpu_last_error()
    for i in range(1, 9):
        ch.collect(b[i].ticket)
        assert same_rows(b[i].table(), want[i]), i
    assert np.all(b[9].rows.array == 0xFF)
    ch.collect(b[9].measure_submit(ch).ticket)
    assert same_rows(b[9].table(), want[9])
    # chains the two-pass scheme does not cover: refused before anything is touched -- what they process next is a fresh chain's
    one = fr(x, 0, B)
    for over, code, word in ((dict(agc=False), EINVAL, b"no output AGC"), (dict(agc_profile="local"), EUNSUPPORTED, b"digital"),
                             (dict(agc_clock="wall"), EUNSUPPORTED, b"WALL")):
        d = dict(kw, **over)
        bad = gpu.Chain(**d)
        rc, got, ticket = raw_measure_submit(bad, Batch(gpu, bad, one), B // CHUNK)
        assert rc == code and got == 0 and ticket == 0 and word in bad._lib.iqgpu_last_error(), over
        if over.get("agc_clock") != "wall":                       # (two wall-clock chains do not read the same time)
            assert np.array_equal(bad.process(one), gpu.Chain(**d).process(one))
    with pytest.raises(gpu.IqgpuError) as e:
        ch.collect(ch._lib.iqgpu_chain_pipeline_depth() * 100)
    assert e.value.code == EINVAL


def test_measure_pipelined_is_measure_per_batch(gpu):
    """the Python convenience loop, with more batches than slots and a short last one"""
    kw = SHAPES["cu8_nrsc5"]
    x = stream("cu8", 10 * B + 5000, seed=86)
    got = gpu.Chain(**kw).measure_pipelined(x, B)
    twin = gpu.Chain(**kw)
    want = np.concatenate([twin.measure(fr(x, a, min(a + B, 10 * B + 5000))) for a in range(0, 10 * B + 5000, B)])
    assert got.size == 10 * (B // CHUNK) + 2 and same_rows(got, want)


# --------------------------------------------------------------------------------------------
# 5. the harness: pass 1 of --seamless-agc on the new call
# --------------------------------------------------------------------------------------------
HARNESS_ARGS = ["--raw-file-input-rate", "96e3", "--raw-file-input-sample-format", "cs16", "--output-rate", "29767.5",
                "--output-sample-format", "cs16", "--freq-shift", "8000", "--agc-profile", "digital"]
HARNESS_KW = dict(in_format="cs16", out_format="cs16", input_rate_hz=96e3, target_rate_hz=29767.5, shift_hz=8000.0, agc=True)


def test_harness_seamless_agc_writes_the_single_streams_file(gpu, tmp_path):
    n, chunk, seed, agc_chunk = 1048576, 16384, 9, 16384
    one, many = tmp_path / "one.cs16", tmp_path / "many.cs16"
    common = ["--synthetic", str(n), "--synthetic-hash", str(seed), *HARNESS_ARGS, "--chunk-frames", str(chunk)]
    run(*common, "-o", str(one), "--shards", "1")
    info = run(*common, "-o", str(many), "--shards", "4", "--seamless-agc", "--devices", "1")
    a, b = np.fromfile(one, np.int16), np.fromfile(many, np.int16)
    assert info["seamless_agc"] is True and a.size == b.size == 2 * info["frames_out"] and a.size > 0
    diff = int((a != b).sum())
    print("--shards 4 --seamless-agc against --shards 1: %d differing components of %d" % (diff, a.size))
    assert diff == 0
    # pass 1 against the synchronous call over the same ranges in the same calls: the row counts, and the AGC state the walk over
    # those rows puts in front of every shard, field by field as the report prints them (%.9g / %.17g: the floats round-trip)
    ch = gpu.Chain(**HARNESS_KW)
    st = ch.agc_initial_state()
    assert len(info["per_shard"]) == 4
    for s, ps in enumerate(info["per_shard"]):
        e = ps["entry"]
        print("shard %d: measure_seconds %.6f, %d rows, entry %s" % (s, ps["measure_seconds"], ps["agc_rows"], e))
        assert ps["measure_seconds"] >= 0.0 and ps["frames_out"] == ps["planned_out"]
        assert (e["locked"], e["samples_seen"]) == (st.locked, st.samples_seen)
        assert np.float32(e["peak_memory"]) == np.float32(st.peak_memory) and np.float32(e["current_gain"]) == np.float32(st.current_gain)
        assert e["last_strong_peak_time"] == st.last_strong_peak_time
        if s == 3:
            assert ps["agc_rows"] == 0
            break
        first, frames, pre = ps["first_frame"], ps["frames_in"], ps["preroll_frames"]
        ch.seek_agc(first, synth.hash_stream(pre, seed, "cs16", first - pre))
        rows = np.concatenate([ch.measure(synth.hash_stream(min(chunk, frames - at), seed, "cs16", first + at)) for at in range(0, frames, chunk)])
        assert ps["agc_rows"] == rows.size == -(-frames // agc_chunk)
        st = ch.agc_advance(st, rows)
    assert info["per_shard"][0]["entry"]["locked"] == 0 and info["per_shard"][3]["entry"]["locked"] == 1
