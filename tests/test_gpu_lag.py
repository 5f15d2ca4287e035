"""The lag-product accumulator on the device (include/iqgpu.h "lag products"; k_lag_rows / k_lag_fold) against the
float64 model of tests/lag_model.py.  Every product is exact in double and the order is fixed: EVERYTHING here is compared for
equality, rows and open row.

Shapes, the smallest at which each part of the kernel can go wrong: B = 64 (rows inside 16 lanes), 256 (a whole wave), 512 (two waves
through LDS), 1024 (one term per column), 4096 (four steps of a page: the LDS window moves on), 65536 (one full cell), 131072 (two cells
through the fold); lags on both sides of every border -- the thread's own four frames, the step of 1024, the row, the largest lag; one
stream of more than 2048 pages, so that a workgroup walks more than one page with its window."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import env_model
import lag_model
from env_model import BPF, FORMATS
from iq_tool_amd import lag, synth

pytestmark = pytest.mark.gpu
RATE = 2.4e6

_streams, _models = {}, {}


def stream_of(fmt, n, seed=21):
    if (fmt, n, seed) not in _streams:
        raw = env_model.stream(fmt, n, seed)
        raw.setflags(write=False)
        _streams[fmt, n, seed] = raw
    return _streams[fmt, n, seed]


def as_bytes(row_lag, row_sum, open_row, info):
    return row_lag.tobytes(), row_sum.tobytes(), (np.asarray(open_row[0], np.complex128).tobytes(), float(open_row[1])), info


def model_of(oracle, raw, fmt, b, lags, key=None):
    """the model's (row_lag bytes, row_sum bytes, (open lag bytes, open sum), info): computed once per shared stream, never changed"""
    if key is None or key not in _models:
        n = raw.size // BPF[fmt] if raw.dtype == np.uint8 else np.ascontiguousarray(raw).view(np.uint8).size // BPF[fmt]
        row_lag, row_sum, open_row, nonfinite = lag_model.model(raw, fmt, b, lags, oracle)
        got = as_bytes(row_lag, row_sum, open_row, dict(frames=n, rows=n // b, nonfinite_frames=nonfinite, open_frames=n % b, block_frames=b,
                                                         n_lags=len(lags), lags=list(lags)))
        if key is None:
            return got
        _models[key] = got
    return _models[key]


def push_split(gpu, raw, fmt, b, lags, cuts=(), device=(), offset=0, acc=None):
    """the stream pushed in pieces cut at `cuts` (frames); pieces whose index is in `device` go through push_device at a pointer
    `offset` bytes into its buffer.  What the pushes returned, concatenated, and the open row"""
    raw = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
    bpf, n, nl = BPF[fmt], raw.size // BPF[fmt], len(lags)
    acc = acc or gpu.Lag(fmt, b, lags)
    parts, keep = [], []
    edges = [0] + list(cuts) + [n]
    for i, (lo, hi) in enumerate(zip(edges[:-1], edges[1:])):
        if hi <= lo:
            continue
        piece = raw[lo * bpf:hi * bpf]
        cap = acc.max_rows(hi - lo)
        if i in device:
            d_in, d_rows = gpu.DeviceBuffer(piece.size + offset + 64), gpu.DeviceBuffer((8 * nl + 4) * cap + 64)
            buf = np.full(piece.size + offset, 0xA5, np.uint8)
            buf[offset:] = piece
            d_in.upload(buf)
            assert acc.push_device(d_in.ptr + offset, hi - lo, d_rows.ptr, d_rows.ptr + 8 * nl * cap, cap) == cap
            acc.read_open()                                    # (synchronises)
            out = d_rows.download((8 * nl + 4) * cap, np.uint8) if cap else np.zeros(0, np.uint8)
            parts.append((out[:8 * nl * cap], out[8 * nl * cap:]))
            keep += [d_in, d_rows]
        else:
            parts.append(acc.push(piece))
    row_lag = b"".join(p[0].tobytes() for p in parts)
    row_sum = b"".join(p[1].tobytes() for p in parts)
    return as_bytes(np.frombuffer(row_lag, np.complex64), np.frombuffer(row_sum, np.float32), acc.read_open()[:2], acc.read_open()[2])


def show(got, want):
    """what a failed comparison prints: where the rows differ"""
    a, b = np.frombuffer(got[0], np.uint32), np.frombuffer(want[0], np.uint32)
    if a.size != b.size:
        return "row_lag sizes %d / %d" % (a.size, b.size)
    bad = np.flatnonzero(a != b)
    return "row_lag differs at %s of %d; sums equal: %s; open equal: %s; info %s / %s" % (bad[:8], a.size, got[1] == want[1], got[2] == want[2], got[3], want[3])


# ---- 1. rows and open row equal the model: the shapes ----
SHAPES = [(64, 5 * 1024 + 3), (256, 5 * 1024 + 3), (512, 5 * 1024 + 3), (1024, 5 * 1024 + 3), (4096, 3 * 4096 + 17), (65536, 2 * 65536 + 17),
          (131072, 2 * 131072 + 777)]


@pytest.mark.parametrize("b,n", SHAPES)
def test_rows_and_open_row_equal_the_model(gpu, oracle, b, n):
    lags = (1, 3, 4, 1025)
    raw = stream_of("cs16", n)
    want = model_of(oracle, raw, "cs16", b, lags, ("cs16", n, b, lags))
    got = push_split(gpu, raw, "cs16", b, lags)
    assert got == want, show(got, want)
    one = push_split(gpu, raw, "cs16", b, (3,))                 # the instantiation for one lag
    want1 = model_of(oracle, raw, "cs16", b, (3,))
    assert one == want1, show(one, want1)


def test_a_workgroup_that_walks_more_than_one_page(gpu, oracle):
    n, b, lags = 2049 * 1024 + 5, 1024, (2, 1025)               # 2050 pages for 2048 workgroups: two pages each
    raw = stream_of("cu8", n)
    want = model_of(oracle, raw, "cu8", b, lags)
    got = push_split(gpu, raw, "cu8", b, lags)
    assert got == want, show(got, want)


# ---- 2. the lag edges ----
@pytest.mark.parametrize("lags,n", [((1, 2, 3, 4), 3 * 4096 + 17), ((1023, 1024, 1025, 1026), 3 * 4096 + 17), ((4095, 4096, 4097), 3 * 4096 + 17),
                                    ((65535, 65536), 3 * 65536 + 5)])
def test_lag_edges(gpu, oracle, lags, n):
    raw = stream_of("cs16", n)
    want = model_of(oracle, raw, "cs16", 4096, lags)
    got = push_split(gpu, raw, "cs16", 4096, lags)
    assert got == want, show(got, want)
    # ... and with the launch cut inside a step, inside the largest lag and on a row: the partners come from the history
    got = push_split(gpu, raw, "cs16", 4096, lags, cuts=sorted({lags[0], 4096, 4096 + 777}), device=(1, 3))
    assert got == want, show(got, want)


# ---- 3. all nine formats ----
@pytest.mark.parametrize("fmt", FORMATS)
def test_every_format(gpu, oracle, fmt):
    b, lags, n = 256, (1, 5), 5 * 1024 + 3
    raw = stream_of(fmt, n)
    want = model_of(oracle, raw, fmt, b, lags)
    got = push_split(gpu, raw, fmt, b, lags)
    assert got == want, show(got, want)
    if fmt == "cs24":                                           # a device pointer at 2-byte alignment
        got = push_split(gpu, raw, fmt, b, lags, cuts=(1000,), device=(0, 1), offset=2)
        assert got == want, show(got, want)
    if fmt in ("cs16", "cu8", "cf32"):                          # one frame off: the single loads; aligned: the vector loads
        for offset in (BPF[fmt], 0):
            got = push_split(gpu, raw, fmt, b, lags, cuts=(1000,), device=(0, 1), offset=offset)
            assert got == want, (offset, show(got, want))


# ---- 4. split invariance ----
def test_any_split_gives_the_same_rows(gpu, oracle):
    n, b, lags = 3 * 65536 + 911, 1024, (1, 1025, 40000)
    raw = stream_of("cs16", n)
    want = model_of(oracle, raw, "cs16", b, lags)
    whole = push_split(gpu, raw, "cs16", b, lags)
    assert whole == want, show(whole, want)
    pieces, at = [], 0
    for step in (1, 63, 1024, 1025, 39999, 65536):
        at += step
        pieces.append(at)
    splits = {"frame by frame for the first 70": list(range(1, 71)), "pieces": pieces}
    for name, cuts in splits.items():
        got = push_split(gpu, raw, "cs16", b, lags, cuts)
        assert got == want, (name, show(got, want))
        got = push_split(gpu, raw, "cs16", b, lags, cuts, device=range(0, 99, 2))
        assert got == want, (name, "host and device alternating", show(got, want))


# ---- 5. reset ----
def test_reset_drops_the_history(gpu, oracle):
    b, lags, n = 1024, (1, 1025, 3000), 4 * 1024 + 9
    raw = stream_of("cs16", n)
    want = model_of(oracle, raw, "cs16", b, lags)
    acc = gpu.Lag("cs16", b, lags)
    acc.push(stream_of("cs16", 5000, seed=22))
    acc.reset()
    got = push_split(gpu, raw, "cs16", b, lags, acc=acc)
    assert got == want, show(got, want)


# ---- 6. row_sum is iqgpu_env's ----
@pytest.mark.parametrize("fmt", ("cs16", "cf32"))
@pytest.mark.parametrize("b", (64, 4096, 131072))
def test_row_sum_is_envs(gpu, fmt, b):
    n = 2 * b + 777
    raw = stream_of(fmt, n)
    got = push_split(gpu, raw, fmt, b, (1, 2048))
    e = gpu.Env(fmt, b)
    s, _, _ = e.push(raw)
    assert got[1] == s.tobytes() and len(got[1]) == 4 * (n // b) and got[2][1] == e.read_open()[0]


# ---- 7. cf32 with NaN / Inf frames ----
@pytest.mark.parametrize("b", (64, 4096, 131072))
def test_cf32_nonfinite_frames(gpu, oracle, b):
    n, lags = 2 * b + 2777, (1, 5, 1500)
    v = stream_of("cf32", n).copy().view(np.float32).reshape(-1, 2)
    # at a row start, at a column's first frame, exactly d behind / in front of finite frames, side by side, at the end
    bad = {0: (np.nan, 0.0), b: (0.0, np.inf), 1024 + 7: (-np.inf, np.nan), b + 5: (np.nan, np.nan), b + 6: (np.inf, 0.5), b + 1500: (1.0, np.nan),
           n - 1: (0.25, -np.inf)}
    for i, pair in bad.items():
        v[i] = pair
    want = model_of(oracle, v, "cf32", b, lags)
    got = push_split(gpu, v, "cf32", b, lags)
    assert got == want, show(got, want)
    assert got[3]["nonfinite_frames"] == len(bad) and np.isfinite(np.frombuffer(got[0], np.float32)).all()
    got = push_split(gpu, v, "cf32", b, lags, cuts=(b + 6, b + 7), device=(1,))
    assert got == want, show(got, want)


# ---- 8. capacity, planes, frames == 0 ----
def test_capacity_max_rows_and_null_planes(gpu, oracle):
    b, n, lags = 64, 3 * 64 + 17, (1, 70)
    raw = stream_of("cs16", n)
    want = model_of(oracle, raw, "cs16", b, lags)
    acc = gpu.Lag("cs16", b, lags)
    lib = acc._lib
    assert acc.max_rows(n) == 3 and acc.max_rows(63) == 0 and acc.max_rows(64) == 1
    r, got = np.zeros(16, np.float32), C.c_size_t(9)
    rc = lib.iqgpu_lag_push(acc._h, raw.ctypes.data_as(C.c_void_p), n, r.ctypes.data_as(C.c_void_p), None, 2, C.byref(got))
    assert rc == -8 and got.value == 0 and not r.any()
    assert acc.read_open()[2]["frames"] == 0                   # the handle as it was
    assert push_split(gpu, raw, "cs16", b, lags, acc=acc) == want
    assert acc.max_rows(64 - 17) == 1 and acc.max_rows(64 - 18) == 0      # exact from the handle's position
    # each plane alone, and none: the other is not produced, the stream goes on all the same
    for which in range(3):
        acc.reset()
        planes = [np.full(12, 7, np.uint32), np.full(3, 7, np.uint32)]
        ptrs = [planes[i].ctypes.data_as(C.c_void_p) if i == which else None for i in range(2)]
        assert lib.iqgpu_lag_push(acc._h, raw.ctypes.data_as(C.c_void_p), n, *ptrs, 3 if which < 2 else 0, C.byref(got)) == 0 and got.value == 3
        for i in range(2):
            assert planes[i].tobytes() == (want[i] if i == which else np.full(planes[i].size, 7, np.uint32).tobytes())
        o = acc.read_open()
        assert (o[0].tobytes(), o[1]) == want[2]
    assert lib.iqgpu_lag_push(acc._h, None, 0, None, None, 0, C.byref(got)) == 0 and got.value == 0      # frames == 0 changes nothing
    assert acc.read_open()[2] == want[3]
    # the asynchronous entry point: one row short is refused before anything is queued, then the full push gives the same rows
    acc.reset()
    d_in, d_rows = gpu.DeviceBuffer(raw.size), gpu.DeviceBuffer(60)
    d_in.upload(raw)
    d_rows.upload(np.full(15, 7, np.uint32))
    got.value = 9
    rc = lib.iqgpu_lag_push_device(acc._h, C.c_void_p(d_in.ptr), n, C.c_void_p(d_rows.ptr), None, 2, C.byref(got), None)
    assert rc == -8 and got.value == 0 and acc.read_open()[2]["frames"] == 0
    assert d_rows.download(60, np.uint32).tolist() == [7] * 15
    assert acc.push_device(d_in.ptr, n, 0, d_rows.ptr + 48, 3) == 3 and acc.read_open()[2] == want[3]
    out = d_rows.download(60, np.uint32)
    assert out[:12].tolist() == [7] * 12 and out[12:].tobytes() == want[1]      # the NULL plane is not produced


# ---- 9. refusals of create ----
def test_create_refusals(gpu):
    lib, h = gpu.load(), C.c_void_p()
    good = lag.lag_opts(4096, (1, 2048))
    assert lib.iqgpu_lag_create(0, 11, C.byref(good), None) == -1
    assert lib.iqgpu_lag_create(0, 11, None, C.byref(h)) == -1 and not h.value
    assert lib.iqgpu_lag_create(0, 3, C.byref(good), C.byref(h)) == -5 and not h.value           # IQGPU_EFORMAT
    assert lib.iqgpu_lag_create(0, 17, C.byref(good), C.byref(h)) == -5 and not h.value
    for dev in (-1, lib.iqgpu_device_count()):
        assert lib.iqgpu_lag_create(dev, 11, C.byref(good), C.byref(h)) == lib.iqgpu_env_create(dev, 11, C.byref(gpu._lib.EnvOpts(64)), C.byref(h)) < 0
        assert not h.value
    for b, lags in ((100, (1,)), (32, (1,)), (1 << 25, (1,)), (4096, ()), (4096, (1, 2, 3, 4, 5)), (4096, (0,)), (4096, (65537,)), (4096, (2, 2)),
                    (4096, (3, 1))):
        assert lib.iqgpu_lag_create(0, 11, C.byref(lag.lag_opts(b, lags)), C.byref(h)) == -1 and not h.value, (b, lags)
    with gpu.Lag("cs16", 4096, (1, 2048)) as acc:
        assert acc.read_open()[2] == dict(frames=0, rows=0, nonfinite_frames=0, open_frames=0, block_frames=4096, n_lags=2, lags=[1, 2048])


# ---- 10. destroy with work in flight ----
def test_destroy_with_work_in_flight_gives_the_memory_back(gpu):
    from test_gpu_lifetime import BAR, free_bytes
    n, rounds = 1 << 20, 16
    raw = stream_of("cs16", n)
    d_in, d_rows = gpu.DeviceBuffer(raw.size), gpu.DeviceBuffer(36 * (n // 64))
    d_in.upload(raw)

    def once():
        acc = gpu.Lag("cs16", 64, (1, 2, 3, 65536))
        acc.push_device(d_in.ptr, n, d_rows.ptr, d_rows.ptr + 32 * (n // 64), n // 64)
        acc.close()                                             # the launch may still run: destroy waits for it
    once()
    before = free_bytes()
    for _ in range(rounds):
        once()
    drift = before - free_bytes()
    print("lifetime lag drift %d bytes over %d rounds (bar %d)" % (drift, rounds, BAR))
    assert drift < BAR


# ---- 11. the sign convention, end to end ----
def test_a_chain_shifted_by_minus_hz_centres_the_tone(gpu):
    """a tone at f0 is estimated at +f0; the chain whose shift_hz is -f0 brings it to 0 (include/iqgpu.h: THE SIGN)"""
    f0, n, b, out_rate = 0.0123 * RATE, 1 << 17, 4096, 744187.5
    z = 0.5 * np.exp(2j * np.pi * (f0 / RATE) * np.arange(n))
    raw = np.stack([z.real, z.imag], axis=1).astype(np.float32)
    with gpu.Lag("cf32", b) as acc:
        row_lag, row_sum = acc.push(raw)
    before = lag.estimate(row_lag, row_sum, b, (1,), 0, RATE)
    print("tone at %.3f Hz estimated at %.6f Hz" % (f0, before["hz"]))
    assert abs(before["hz"] - f0) <= 1e-6 * RATE
    ch = gpu.Chain(in_format="cf32", out_format="cf32", input_rate_hz=RATE, target_rate_hz=out_rate, shift_hz=-before["hz"], gain=1.0)
    out = ch.process(raw)
    with gpu.Lag("cf32", b) as acc:
        row_lag, row_sum = acc.push(out)
    rows = row_sum.size
    assert rows >= 8
    after = lag.estimate(row_lag, row_sum, b, (1,), 0, out_rate, first_row=2)        # (behind the filters' rise)
    print("behind the chain: %.6f Hz, coherence %.6f over %d rows" % (after["hz"], after["coherence"], rows - 2))
    assert abs(after["hz"]) <= 1e-6 * out_rate and after["coherence"] > 0.99


# ---- 12. behind a chain on its stream ----
def test_behind_a_chain_on_its_stream(gpu):
    kw = dict(in_format="cs16", out_format="cs8", input_rate_hz=RATE, target_rate_hz=744187.5, shift_hz=200e3, gain=40.0)
    n, b, lags = 1 << 17, 2048, (1, 2048)
    raw = synth.raw_stream(n, RATE, 31, "cs16")
    plain = gpu.Chain(**kw).process(raw)
    ch = gpu.Chain(**kw)
    cap = (ch.next_out_frames(n) + 1) * 2
    d_in, d_out = gpu.DeviceBuffer(raw.nbytes), gpu.DeviceBuffer(cap)
    d_in.upload(raw)
    got = ch.process_device(d_in.ptr, n, d_out.ptr, cap)
    acc = gpu.Lag("cs8", b, lags)
    rows = acc.max_rows(got)
    d_rows = gpu.DeviceBuffer(20 * rows)
    assert acc.push_device(d_out.ptr, got, d_rows.ptr, d_rows.ptr + 16 * rows, rows, ch.get_stream()) == rows
    open_row = acc.read_open()
    ch.synchronize()
    out = d_rows.download(20 * rows, np.uint8)
    want = push_split(gpu, plain, "cs8", b, lags)
    assert (out[:16 * rows].tobytes(), out[16 * rows:].tobytes()) == want[:2] and (open_row[0].tobytes(), open_row[1]) == want[2] and rows > 4


# ---- 13. the harness ----
EXE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "iq_tool_amd", "lib", "iqgpu_run")
ARGS = ["--raw-file-input-rate", "2.4e6", "--raw-file-input-sample-format", "cs16", "--output-rate", "744187.5",
        "--output-sample-format", "cs16", "--freq-shift", "200e3"]


def test_harness_lag_files_and_json(gpu, tmp_path):
    b, lags, n = 1024, (1, 8, 2048), 64 * 1024 + 77
    raw = np.ascontiguousarray(stream_of("cs16", n)).view(np.int16)
    fin, fout, prefix = tmp_path / "in.cs16", tmp_path / "out.cs16", tmp_path / "lag"
    raw.tofile(fin)
    r = subprocess.run([EXE, "-i", str(fin), "-o", str(fout), *ARGS, "--chunk-frames", "5000", "--lag", str(prefix), "--lag-list", "1,8,2048",
                        "--lag-block", str(b)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    out = np.fromfile(fout, np.int16)
    meta = json.loads(open(str(prefix) + ".json").read())
    assert meta["block_frames"] == b and meta["lags"] == list(lags)
    for side, data, rate in (("in", raw, 2.4e6), ("out", out, 744187.5)):
        row_lag, row_sum, open_row, info = push_split(gpu, data, "cs16", b, lags)
        assert open(str(prefix) + "." + side + ".lag.f32", "rb").read() == row_lag, side
        assert open(str(prefix) + "." + side + ".sum.f32", "rb").read() == row_sum, side
        assert len(row_lag) == info["rows"] * 8 * len(lags) and len(row_sum) == info["rows"] * 4
        m = meta[side]
        assert (m["frames"], m["rows"], m["open_frames"], m["nonfinite_frames"]) == (info["frames"], info["rows"], info["open_frames"], 0)
        assert m["sample_rate"] == rate
        for li, d in enumerate(lags):
            want = lag.estimate(np.frombuffer(row_lag, np.complex64), np.frombuffer(row_sum, np.float32), b, lags, li, rate)
            assert m["estimates"][li] == dict(lag=d, **want), (side, d)      # == on the parsed doubles
    assert meta["in"]["rows"] == 64 and meta["in"]["open_frames"] == 77 and meta["out"]["rows"] > 8


def test_harness_lag_refusals(gpu, tmp_path):
    base = ["--synthetic", "100000", "--synthetic-hash", "3", *ARGS, "--lag", str(tmp_path / "lag")]
    for extra in (["--shards", "2"], ["--shards", "2", "--seamless"], ["--shards", "2", "--seamless-agc"], ["--iq-calibrate"]):
        r = subprocess.run([EXE, *base, *extra], capture_output=True, text=True)
        assert r.returncode == 2 and "usage" in r.stderr and "--lag" in r.stderr, (extra, r.returncode, r.stderr)
    for block in ("100", "32", "33554432"):
        r = subprocess.run([EXE, *base, "--lag-block", block], capture_output=True, text=True)
        assert r.returncode == 2 and "--lag-block" in r.stderr, (block, r.stderr)
    for lst in ("0", "65537", "2,2", "3,1", "1,2,3,4,5", "1,x", ""):
        r = subprocess.run([EXE, *base, "--lag-list", lst], capture_output=True, text=True)
        assert r.returncode == 2 and "--lag-list" in r.stderr, (lst, r.stderr)
    for alone in (["--lag-block", "64"], ["--lag-list", "1,2"]):
        r = subprocess.run([EXE, "--synthetic", "100000", "--synthetic-hash", "3", *ARGS, *alone], capture_output=True, text=True)
        assert r.returncode == 2 and alone[0] in r.stderr
    assert not list(tmp_path.iterdir())
