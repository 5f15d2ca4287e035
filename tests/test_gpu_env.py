"""The envelope accumulator on the device (include/iqgpu.h "envelope"; k_env_rows / k_env_fold) against the float64
model of tests/env_model.py.  Every term is exact in double and the order is fixed: EVERYTHING here is compared for equality.

Shapes, the smallest at which each part of the kernel can go wrong: B = 64 (a row inside a wave), 1024 (one term per column), 2048
(two terms per column), 65536 (one full cell), 131072 (two cells through the fold); streams of 3 B + 17 frames and of 5 B exactly."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import env_model
from env_model import BPF, FORMATS
from iq_tool_amd import env, synth

pytestmark = pytest.mark.gpu
BLOCKS = (64, 1024, 2048, 65536, 131072)
RATE = 2.4e6


def cases():
    for fmt in FORMATS:
        for b in BLOCKS if fmt in ("cs16", "cu8", "cf32") else (64, 2048):
            yield fmt, b


_streams, _refs = {}, {}


def stream_of(fmt, n):
    if (fmt, n) not in _streams:
        raw = env_model.stream(fmt, n, 11)
        raw.setflags(write=False)
        _streams[fmt, n] = raw
    return _streams[fmt, n]


def one_push(gpu, raw, fmt, b):
    """(rows as bytes, open row, info) of ONE host push"""
    acc = gpu.Env(fmt, b)
    s, k, r = acc.push(raw)
    return (s.tobytes(), k.tobytes(), r.tobytes()), acc.read_open()


def reference(gpu, fmt, b, n):
    """the one-push result of the shared stream: computed once, never changed"""
    if (fmt, b, n) not in _refs:
        _refs[fmt, b, n] = one_push(gpu, stream_of(fmt, n), fmt, b)
    return _refs[fmt, b, n]


def collect(parts):
    return tuple(b"".join(p[i].tobytes() for p in parts) for i in range(3))


# ---- 1. rows and open row equal the model ----
@pytest.mark.parametrize("fmt,b", list(cases()))
@pytest.mark.parametrize("whole", (False, True))
def test_rows_and_open_row_equal_the_model(gpu, oracle, fmt, b, whole):
    n = 5 * b if whole else 3 * b + 17
    raw = stream_of(fmt, n)
    (s, k, r), (osum, opeak, orail, info) = reference(gpu, fmt, b, n)
    ws, wk, wr, wopen, wnonfinite = env_model.model(raw, fmt, b, oracle)
    assert info == dict(frames=n, rows=n // b, nonfinite_frames=wnonfinite, open_frames=n % b, block_frames=b)
    assert np.array_equal(np.frombuffer(s, np.uint32), ws.view(np.uint32)), (np.frombuffer(s, np.float32), ws)
    assert np.array_equal(np.frombuffer(k, np.uint32), wk.view(np.uint32))
    assert np.array_equal(np.frombuffer(r, np.uint32), wr) and int(wr.sum()) + wopen[2] >= 4       # (the planted rail codes)
    assert (osum, opeak, orail) == wopen


# ---- 2. cut-invariance ----
def push_split(gpu, raw, fmt, b, cuts, device=(), offset=0):
    """the stream pushed in pieces cut at `cuts` (frames); pieces whose index is in `device` go through push_device at a pointer
    `offset` bytes into its buffer"""
    bpf, n = BPF[fmt], raw.size // BPF[fmt]
    acc, parts, keep = gpu.Env(fmt, b), [], []
    edges = [0] + list(cuts) + [n]
    for i, (lo, hi) in enumerate(zip(edges[:-1], edges[1:])):
        if hi <= lo:
            continue
        piece = raw[lo * bpf:hi * bpf]
        cap = acc.max_rows(hi - lo)
        if i in device:
            d_in, d_rows = gpu.DeviceBuffer(piece.size + offset + 64), gpu.DeviceBuffer(12 * cap + 64)
            buf = np.full(piece.size + offset, 0xA5, np.uint8)
            buf[offset:] = piece
            d_in.upload(buf)
            got = acc.push_device(d_in.ptr + offset, hi - lo, d_rows.ptr, d_rows.ptr + 4 * cap, d_rows.ptr + 8 * cap, cap)
            assert got == cap
            acc.read_open()                                    # (synchronises)
            out = d_rows.download(12 * cap, np.uint8) if cap else np.zeros(0, np.uint8)
            parts.append((out[:4 * cap], out[4 * cap:8 * cap], out[8 * cap:12 * cap]))
            keep += [d_in, d_rows]
        else:
            parts.append(acc.push(piece))
    return collect(parts), acc.read_open()


@pytest.mark.parametrize("fmt,b", [(f, b) for f in ("cs16", "cf32", "cs24") for b in BLOCKS if f != "cs24" or b in (64, 2048)])
def test_any_split_gives_the_same_rows(gpu, fmt, b):
    n = 3 * b + 17
    raw, want = stream_of(fmt, n), reference(gpu, fmt, b, n)
    cell = min(b, 65536)
    splits = {
        "777": list(range(777, n, 777)),
        "around a row boundary": [b - 1, b + 1, 2 * b],
        "around a cell boundary": [cell - 1, cell, cell + 1, 2 * cell + 1],
    }
    for name, cuts in splits.items():
        assert push_split(gpu, raw, fmt, b, cuts) == want, name
        assert push_split(gpu, raw, fmt, b, cuts, device=range(0, 99, 2)) == want, (name, "host and device mixed")
    # a device pointer one frame off the buffer's alignment
    assert push_split(gpu, raw, fmt, b, [b + 5], device=(0, 1), offset=BPF[fmt]) == want


def test_pushes_of_one_frame(gpu):
    raw = env_model.stream("cs16", 300, 12)
    want = one_push(gpu, raw, "cs16", 64)
    assert push_split(gpu, raw, "cs16", 64, list(range(1, 300))) == want
    assert len(want[0][0]) == 4 * (300 // 64) and want[1][3]["open_frames"] == 300 % 64


# ---- 3. capacity ----
def test_capacity_max_rows_and_null_planes(gpu):
    b, n = 64, 3 * 64 + 17
    raw, want = stream_of("cs16", n), reference(gpu, "cs16", 64, n)
    acc = gpu.Env("cs16", b)
    lib = acc._lib
    assert acc.max_rows(n) == 3 and acc.max_rows(63) == 0 and acc.max_rows(64) == 1
    s, got = np.zeros(8, np.float32), C.c_size_t(9)
    rc = lib.iqgpu_env_push(acc._h, raw.ctypes.data_as(C.c_void_p), n, s.ctypes.data_as(C.c_void_p), None, None, 2, C.byref(got))
    assert rc == -8 and got.value == 0 and not s.any()
    assert acc.read_open()[3]["frames"] == 0                   # the handle as it was
    full = acc.push(raw)
    assert collect([full]) == want[0] and acc.read_open() == want[1]
    assert acc.max_rows(64 - 17) == 1 and acc.max_rows(64 - 18) == 0      # exact from the handle's position
    # each plane alone, and none: the others are not produced, the stream goes on all the same
    for which in range(4):
        acc.reset()
        planes = [np.full(3, 7, np.uint32) for _ in range(3)]
        ptrs = [planes[i].ctypes.data_as(C.c_void_p) if i == which else None for i in range(3)]
        assert lib.iqgpu_env_push(acc._h, raw.ctypes.data_as(C.c_void_p), n, *ptrs, 3 if which < 3 else 0, C.byref(got)) == 0 and got.value == 3
        for i in range(3):
            assert planes[i].tobytes() == (want[0][i] if i == which else np.full(3, 7, np.uint32).tobytes())
        assert acc.read_open() == want[1]
    assert lib.iqgpu_env_push(acc._h, None, 0, None, None, None, 0, C.byref(got)) == 0 and got.value == 0      # frames == 0 changes nothing
    assert acc.read_open() == want[1]
    # the asynchronous entry point: one row short is refused before anything is queued, then the full push gives the same rows
    acc.reset()
    d_in, d_rows = gpu.DeviceBuffer(raw.size), gpu.DeviceBuffer(36)
    d_in.upload(raw)
    d_rows.upload(np.full(9, 7, np.uint32))
    got.value = 9
    rc = lib.iqgpu_env_push_device(acc._h, C.c_void_p(d_in.ptr), n, C.c_void_p(d_rows.ptr), None, C.c_void_p(d_rows.ptr + 24), 2, C.byref(got), None)
    assert rc == -8 and got.value == 0 and acc.read_open()[3]["frames"] == 0
    assert d_rows.download(36, np.uint32).tolist() == [7] * 9
    assert acc.push_device(d_in.ptr, n, d_rows.ptr, 0, d_rows.ptr + 24, 3) == 3 and acc.read_open() == want[1]
    out = d_rows.download(36, np.uint32)
    assert out[:3].tobytes() == want[0][0] and out[3:6].tolist() == [7] * 3 and out[6:].tobytes() == want[0][2]      # the NULL plane is not produced


# ---- 4. cf32 edge cases, rails, silence ----
@pytest.mark.parametrize("b", (64, 2048, 131072))
def test_cf32_nonfinite_frames_are_skipped_and_counted(gpu, oracle, b):
    n = 3 * b + 17
    v = stream_of("cf32", n).copy().view(np.float32).reshape(-1, 2)
    bad = {0: (np.nan, 0.0), 1: (0.0, np.inf), b - 1: (-np.inf, np.nan), b: (np.nan, np.nan), 2 * b + 5: (np.inf, 0.5), n - 1: (0.25, -np.inf)}
    for i, pair in bad.items():
        v[i] = pair
    (s, k, r), (osum, opeak, orail, info) = one_push(gpu, v, "cf32", b)
    ws, wk, wr, wopen, wnonfinite = env_model.model(v, "cf32", b, oracle)
    assert info["nonfinite_frames"] == wnonfinite == len(bad)
    assert s == ws.tobytes() and k == wk.tobytes() and r == wr.tobytes() and (osum, opeak, orail) == wopen
    assert np.isfinite(np.frombuffer(s, np.float32)).all() and np.isfinite(np.frombuffer(k, np.float32)).all()
    # a row of nothing but non-finite frames: zeros
    (s, k, r), (_, _, _, info) = one_push(gpu, np.full((64, 2), np.nan, np.float32), "cf32", 64)
    assert s == k == r == bytes(4) and info["nonfinite_frames"] == 64


@pytest.mark.parametrize("fmt", FORMATS)
def test_rail_codes_and_silence(gpu, oracle, fmt):
    b, n = 64, 3 * 64
    if fmt == "cf32":
        hi = np.tile(np.array([1.0, -1.0], np.float32), n).view(np.uint8)
        zero = np.zeros(n * 8, np.uint8)
    else:
        hi = env_model.bytes_of(np.tile(np.array(env_model.RAILS[fmt], np.int64), n), fmt)
        mid = 0 if fmt[1] == "s" or fmt == "sc16q11" else (1 << (4 * BPF[fmt] - 1))      # the code nearest 0.0 (unsigned: x = -2^-(bits))
        zero = env_model.bytes_of(np.full((n, 2), mid, np.int64), fmt)
    (s, k, r), _ = one_push(gpu, hi, fmt, b)
    assert np.frombuffer(r, np.uint32).tolist() == [2 * b] * 3
    ws, wk, wr, _, _ = env_model.model(hi, fmt, b, oracle)
    assert s == ws.tobytes() and k == wk.tobytes()
    (s, k, r), _ = one_push(gpu, zero, fmt, b)
    ws, wk, wr, _, _ = env_model.model(zero, fmt, b, oracle)
    assert s == ws.tobytes() and k == wk.tobytes() and r == bytes(12)
    if fmt[1] == "s" or fmt in ("sc16q11", "cf32"):
        assert s == k == bytes(12)                             # digital silence: zeros


# ---- 5. the two cross-checks with iqgpu_stats ----
@pytest.mark.parametrize("fmt,b", [("cs16", 64), ("cu8", 2048), ("cf32", 65536), ("sc16q11", 2048), ("cs16", 131072)])
def test_cross_checks_with_stats(gpu, fmt, b):
    n = 5 * b
    raw = stream_of(fmt, n)
    (s, k, r), (_, _, _, info) = reference(gpu, fmt, b, n)
    st = gpu.Stats(fmt)
    st.push(raw)
    res = st.read()
    assert info["open_frames"] == 0
    assert np.float32(res.peak_power) == np.frombuffer(k, np.float32).max()
    assert sum(res.rail_lo) + sum(res.rail_hi) == int(np.frombuffer(r, np.uint32).sum()) > 0


# ---- 6. behind a chain ----
def test_behind_a_chain_on_its_stream(gpu):
    kw = dict(in_format="cs16", out_format="cs8", input_rate_hz=RATE, target_rate_hz=744187.5, shift_hz=200e3, gain=40.0)
    n, b = 1 << 17, 2048
    raw = synth.raw_stream(n, RATE, 31, "cs16")
    plain = gpu.Chain(**kw).process(raw)                      # no accumulator in play
    ch = gpu.Chain(**kw)
    cap = (ch.next_out_frames(n) + 1) * 2
    d_in, d_out = gpu.DeviceBuffer(raw.nbytes), gpu.DeviceBuffer(cap)
    d_in.upload(raw)
    got = ch.process_device(d_in.ptr, n, d_out.ptr, cap)
    acc = gpu.Env("cs8", b)
    rows = acc.max_rows(got)
    d_rows = gpu.DeviceBuffer(12 * rows)
    assert acc.push_device(d_out.ptr, got, d_rows.ptr, d_rows.ptr + 4 * rows, d_rows.ptr + 8 * rows, rows, ch.get_stream()) == rows
    open_row = acc.read_open()
    ch.synchronize()
    assert np.array_equal(d_out.download(got * 2, np.int8), plain)
    out = d_rows.download(12 * rows, np.uint8)
    want = one_push(gpu, plain, "cs8", b)
    assert (out[:4 * rows].tobytes(), out[4 * rows:8 * rows].tobytes(), out[8 * rows:].tobytes()) == want[0] and open_row == want[1]
    assert rows == got // b > 4 and np.frombuffer(want[0][2], np.uint32).sum() > 0


# ---- 7. the harness ----
EXE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "iq_tool_amd", "lib", "iqgpu_run")
ARGS = ["--raw-file-input-rate", "2.4e6", "--raw-file-input-sample-format", "cs16", "--output-rate", "744187.5",
        "--output-sample-format", "cs16", "--freq-shift", "200e3"]


def test_harness_envelope_files_json_and_bursts(gpu, tmp_path):
    b, rows, first, last = 1024, 64, 24 * 1024 + 300, 40 * 1024 - 200          # noise, a burst over frames [first, last), noise
    rng = np.random.default_rng(41)
    x = rng.standard_normal((rows * b + 77, 2)) * 0.01
    x[first:last] += rng.standard_normal((last - first, 2)) * 0.3
    raw = np.clip(np.rint(x * 32767.0), -32768, 32767).astype(np.int16)
    fin, fout, prefix = tmp_path / "in.cs16", tmp_path / "out.cs16", tmp_path / "env"
    raw.tofile(fin)
    r = subprocess.run([EXE, "-i", str(fin), "-o", str(fout), *ARGS, "--chunk-frames", "5000", "--envelope", str(prefix), "--envelope-block", str(b)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    out = np.fromfile(fout, np.int16)
    meta = json.loads(open(str(prefix) + ".json").read())
    assert meta["block_frames"] == b and (meta["min_rows"], meta["hang_rows"], meta["pad_rows"]) == (2, 2, 1)
    sums = {}
    for side, data in (("in", raw), ("out", out)):
        (s, _, _), (osum, opeak, orail, info) = one_push(gpu, data, "cs16", b)
        assert open(str(prefix) + "." + side + ".f32", "rb").read() == s, side
        m = meta[side]
        assert (m["frames"], m["rows"], m["open_frames"], m["nonfinite_frames"]) == (info["frames"], info["rows"], info["open_frames"], 0)
        assert m["open"] == dict(sum=osum, peak=opeak, rail=orail), side      # == on the parsed doubles
        sums[side] = np.frombuffer(s, np.float32)
    assert meta["in"]["rows"] == rows and meta["in"]["open_frames"] == 77 and meta["out"]["rows"] > 8
    # the bursts: the library's on the same rows, and they bracket the synthetic burst to within pad_rows + 1 rows
    floor = env.floor(sums["in"], b, 0.1)
    assert meta["floor"] == floor and meta["on"] == floor * 10.0 and meta["off"] == floor * 5.011872336272722
    assert meta["bursts"] == env.bursts(sums["in"], b, meta["on"], meta["off"], min_rows=2, hang_rows=2, pad_rows=1)
    assert len(meta["bursts"]) == 1
    got = meta["bursts"][0]
    r0, r1 = first // b, -(-last // b)                          # the rows the burst touches
    assert got["first_frame"] % b == 0 and got["frames"] % b == 0
    assert r0 - 2 <= got["first_frame"] // b <= r0 and r1 <= (got["first_frame"] + got["frames"]) // b <= r1 + 2
    assert r0 <= got["peak_row"] < r1 and got["peak_mean"] > 100 * floor


def test_harness_envelope_refusals(gpu, tmp_path):
    base = ["--synthetic", "100000", "--synthetic-hash", "3", *ARGS, "--envelope", str(tmp_path / "env")]
    for extra in (["--shards", "2"], ["--shards", "2", "--seamless"], ["--shards", "2", "--seamless-agc"], ["--iq-calibrate"]):
        r = subprocess.run([EXE, *base, *extra], capture_output=True, text=True)
        assert r.returncode == 2 and "usage" in r.stderr and "--envelope" in r.stderr, (extra, r.returncode, r.stderr)
    for block in ("100", "32", "33554432"):
        r = subprocess.run([EXE, *base, "--envelope-block", block], capture_output=True, text=True)
        assert r.returncode == 2 and "--envelope-block" in r.stderr, (block, r.stderr)
    r = subprocess.run([EXE, "--synthetic", "100000", "--synthetic-hash", "3", *ARGS, "--envelope-block", "64"], capture_output=True, text=True)
    assert r.returncode == 2 and "--envelope-block" in r.stderr
    assert not list(tmp_path.iterdir())
