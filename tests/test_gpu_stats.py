"""The capture-statistics accumulator on the device (include/iqgpu.h "capture statistics"; k_stats_pages / k_stats_fold).

1. Exact, all nine formats.  The model is numpy in this file: integer operations on the codes for hist and the rails, the oracle's
   conversion at gain 1 for the values.  Every integer field, min, max, peak_power and peak_frame must be EQUAL.  The five sums are
   held against math.fsum of the exact double terms: |got - exact| <= n 2^-53 sum|term|, the standard bound for n - 1 additions in
   any order (valid below 9e7 terms).
2. Degenerate data (every lane of every wave on one bin).   3. Bit for bit under any split, host or device, at every alignment; read
   observes; reset equals a fresh handle; two handles agree.   4. Guard frames: nothing outside is read.   5. cf32 with NaN / Inf
   frames.   6. Merge of four handles against one.   7. Behind a chain, on its stream.   8. The harness's --stats.
Shapes: with P = stats.geometry() frames a page (65536), streams of 1, P - 1, P, P + 1 and 2 P + 3 frames."""
import ctypes as C
import json
import math
import os
import subprocess

import numpy as np
import pytest

from iq_tool_amd import stats, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "iq_tool_amd", "lib", "iqgpu_run")
RATE = 2.4e6
FORMATS = ("cu8", "cs8", "cu16", "cs16", "sc16q11", "cs24", "cu32", "cs32", "cf32")
BPF = dict(cu8=2, cs8=2, cu16=4, cs16=4, sc16q11=4, cs24=6, cu32=8, cs32=8, cf32=8)
ALIGN = dict(cu8=2, cs8=2, cu16=4, cs16=4, sc16q11=4, cs24=2, cu32=8, cs32=8, cf32=8)
CODE = dict(cu8=np.uint8, cs8=np.int8, cu16=np.uint16, cs16=np.int16, sc16q11=np.int16, cu32=np.uint32, cs32=np.int32)
# lowest / highest code, histogram shift and offset
RAILS = dict(cu8=(0, 255, 0, 0), cs8=(-128, 127, 0, 128), cu16=(0, 65535, 8, 0), cs16=(-32768, 32767, 8, 128), sc16q11=(-2048, 2047, 4, 128),
             cs24=(-(1 << 23), (1 << 23) - 1, 16, 128), cu32=(0, (1 << 32) - 1, 24, 0), cs32=(-(1 << 31), (1 << 31) - 1, 24, 128))
EXACT = ("frames", "nonfinite_frames", "rail_lo", "rail_hi", "hist", "min", "max", "peak_power", "peak_frame")
SUMS = ("sum", "sum_sq", "sum_iq")


def sizes():
    P = stats.geometry()
    return {"1": 1, "P - 1": P - 1, "P": P, "P + 1": P + 1, "2 P + 3": 2 * P + 3}


def codes_of(raw, fmt):
    """[n][2] int64 codes of the raw bytes of an integer format"""
    raw = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
    if fmt == "cs24":
        b = raw.reshape(-1, 3).astype(np.int64)
        c = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        return np.where(c >= 1 << 23, c - (1 << 24), c).reshape(-1, 2)
    return raw.view(CODE[fmt]).astype(np.int64).reshape(-1, 2)


def bytes_of(codes, fmt):
    if fmt == "cs24":
        c = (codes.reshape(-1) & 0xffffff).astype(np.int64)
        return np.stack([c & 0xff, (c >> 8) & 0xff, (c >> 16) & 0xff], axis=1).astype(np.uint8).reshape(-1)
    return codes.reshape(-1).astype(CODE[fmt]).view(np.uint8)


def stream(fmt, n, seed):
    """n frames of the synthetic stream as bytes, rail codes (cf32: values at and beyond +-1.0) written in at known places"""
    raw = np.ascontiguousarray(synth.raw_stream(n, RATE, seed, fmt)).view(np.uint8).reshape(-1).copy()
    places = sorted({0, n // 3, n // 2, n - 1})
    if fmt == "cf32":
        v = raw.view(np.float32).reshape(-1, 2)
        for k, i in enumerate(places):
            v[i] = [(-1.0, 1.0), (1.0, -1.5), (0.99999994, 1.25), (-1.0, -1.0)][k % 4]
        return raw
    lo, hi = RAILS[fmt][:2]
    c = codes_of(raw, fmt)
    for k, i in enumerate(places):
        c[i] = [(lo, hi), (hi, hi), (lo, lo), (hi, lo)][k % 4]
    if fmt == "sc16q11" and n > 8:
        c[5], c[7] = (-32768, 32767), (-2049, 2048)           # beyond the Q11 rails: clamped bins, counted as on the rail
    if fmt == "cs32" and n > 8:
        c[5], c[7] = ((3 << 24) - 1, -(5 << 24) - 1), ((1 << 24) - 1, -1)    # codes that round to the next bin's edge in float
    return bytes_of(c, fmt)


def model(raw, fmt, oracle):
    """the exact fields as a dict like stats.as_dict's, and the exact double terms of the five sums"""
    raw = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
    x = oracle.to_cf32(raw, fmt, 1.0)
    n = x.size
    re, im = x.real.astype(np.float32), x.imag.astype(np.float32)
    ok = np.isfinite(re) & np.isfinite(im)
    m = dict(frames=n, nonfinite_frames=int(n - ok.sum()))
    if fmt == "cf32":
        v = np.stack([re, im], axis=1)[ok]
        bins = np.clip(np.floor(v.astype(np.float64) * 128.0), -128, 127).astype(np.int64) + 128
        lo, hi = v <= -1.0, v >= 1.0
    else:
        c = codes_of(raw, fmt)
        rl, rh, shift, off = RAILS[fmt]
        bins = np.clip((c >> shift) + off, 0, 255)
        lo, hi = (c <= rl, c >= rh) if fmt == "sc16q11" else (c == rl, c == rh)
    m["rail_lo"], m["rail_hi"] = [int(lo[:, c].sum()) for c in range(2)], [int(hi[:, c].sum()) for c in range(2)]
    m["hist"] = [np.bincount(bins[:, c], minlength=256).tolist() for c in range(2)]
    r64, i64 = re.astype(np.float64), im.astype(np.float64)
    p = np.where(ok, r64 * r64 + i64 * i64, -1.0)             # (numpy float64: two exact products, one rounded sum)
    if ok.any():
        m["min"], m["max"] = [float(re[ok].min()), float(im[ok].min())], [float(re[ok].max()), float(im[ok].max())]
        m["peak_power"], m["peak_frame"] = float(p.max()), int(p.argmax())
    else:
        m["min"], m["max"], m["peak_power"], m["peak_frame"] = [0.0, 0.0], [0.0, 0.0], 0.0, 0
    r64, i64 = r64[ok], i64[ok]
    terms = dict(sum=[r64, i64], sum_sq=[r64 * r64, i64 * i64], sum_iq=r64 * i64)
    return m, terms


def check_sums(got, terms, n):
    for name in SUMS:
        for g, t in zip(np.atleast_1d(got[name]), terms[name] if name != "sum_iq" else [terms[name]]):
            exact, bar = math.fsum(t), n * 2.0 ** -53 * math.fsum(np.abs(t))
            assert abs(g - exact) <= bar, (name, g, exact, bar)


def one_call(gpu, raw, fmt):
    acc = gpu.Stats(fmt)
    acc.push(raw)
    return acc


def result(acc):
    return bytes(acc.read())


_cache = {}


def reference(gpu, fmt, name, seed=11):
    """(bytes of the stream, bytes of the result of ONE host push): computed once, shared, never changed"""
    key = (fmt, name, seed)
    if key not in _cache:
        raw = stream(fmt, sizes()[name], seed)
        raw.setflags(write=False)
        _cache[key] = (raw, result(one_call(gpu, raw, fmt)))
    return _cache[key]


# ---- 1. exact, all nine formats ----
@pytest.mark.parametrize("name", ("1", "P - 1", "P", "P + 1", "2 P + 3"))
@pytest.mark.parametrize("fmt", FORMATS)
def test_exact_against_the_model(gpu, oracle, fmt, name):
    raw, _ = reference(gpu, fmt, name)
    n = sizes()[name]
    got = stats.as_dict(one_call(gpu, raw, fmt).read())
    want, terms = model(raw, fmt, oracle)
    for k in EXACT:
        assert got[k] == want[k], (k, got[k], want[k])
    assert sum(want["rail_lo"]) + sum(want["rail_hi"]) >= 2 and sum(got["hist"][0]) == n == sum(got["hist"][1])
    check_sums(got, terms, n)


# ---- 2. degenerate data: every lane on one bin ----
@pytest.mark.parametrize("case", ("zeros cs16", "zeros cu8", "zeros cf32", "high rail cs16", "high rail cs8", "alternating cu8"))
def test_degenerate_streams_are_exact(gpu, oracle, case):
    kind, fmt = case.rsplit(" ", 1)
    n = sizes()["2 P + 3"]
    if kind == "zeros":
        raw = np.zeros(n * BPF[fmt], np.uint8)
    elif kind == "high rail":
        raw = bytes_of(np.full((n, 2), RAILS[fmt][1], np.int64), fmt)
    else:
        raw = np.tile(np.array([0, 0, 255, 255], np.uint8), (n + 1) // 2)[:2 * n].copy()     # frames (0, 0), (255, 255), ...
    got = stats.as_dict(one_call(gpu, raw, fmt).read())
    want, terms = model(raw, fmt, oracle)
    for k in EXACT:
        assert got[k] == want[k], (k, got[k], want[k])
    check_sums(got, terms, n)
    if kind == "zeros":
        assert max(got["hist"][0]) == n and got["peak_frame"] == 0
        if fmt != "cu8":
            assert got["sum"] == [0.0, 0.0] and got["peak_power"] == 0.0
    if kind == "high rail":
        assert got["rail_hi"] == [n, n] and got["hist"][0][255] == n and got["peak_frame"] == 0
    if kind == "alternating":
        assert got["rail_lo"] == [(n + 1) // 2] * 2 and got["rail_hi"] == [n // 2] * 2 and got["hist"][1][0] + got["hist"][1][255] == n


# ---- 3. bit for bit under splits ----
def push_device_pieces(gpu, acc, raw, fmt, cuts, offsets=(0,)):
    bpf, keep = BPF[fmt], []
    edges = [0] + list(cuts) + [raw.size // bpf]
    for k, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
        if b > a:
            off = offsets[k % len(offsets)]
            d = gpu.DeviceBuffer((b - a) * bpf + off + 64)
            buf = np.full((b - a) * bpf + off, 0xA5, np.uint8)
            buf[off:] = raw[a * bpf:b * bpf]
            d.upload(buf)
            acc.push_device(d.ptr + off, b - a)
            keep.append(d)
    return keep


@pytest.mark.parametrize("fmt", ("cs16", "cu8", "cf32", "cs24"))
def test_any_split_gives_the_same_bytes(gpu, fmt):
    raw, base = reference(gpu, fmt, "2 P + 3")
    n, P, bpf = sizes()["2 P + 3"], stats.geometry(), BPF[fmt]
    rng = np.random.default_rng(5)
    for trial in range(2):
        cuts = np.sort(rng.choice(np.arange(1, n), 9, replace=False)).tolist()
        acc = gpu.Stats(fmt)
        for a, b in zip([0] + cuts, cuts + [n]):
            acc.push(raw[a * bpf:b * bpf])
        assert result(acc) == base, ("host", cuts)
        acc = gpu.Stats(fmt)
        keep = push_device_pieces(gpu, acc, raw, fmt, cuts)
        assert result(acc) == base, ("device", cuts)
        del keep
    # across a page boundary frame by frame, host and device pushes taking turns
    acc = gpu.Stats(fmt)
    acc.push(raw[:(P - 3) * bpf])
    keep = []
    for i in range(P - 3, P + 5):
        if i % 2:
            acc.push(raw[i * bpf:(i + 1) * bpf])
        else:
            keep += push_device_pieces(gpu, acc, raw[i * bpf:(i + 1) * bpf], fmt, [])
    acc.push(raw[(P + 5) * bpf:])
    assert result(acc) == base


@pytest.mark.parametrize("fmt", FORMATS)
def test_every_frame_alignment_of_a_device_pointer(gpu, fmt):
    raw, base = reference(gpu, fmt, "P + 1")
    n, a = sizes()["P + 1"], ALIGN[fmt]
    offsets = list(range(0, 32, a))
    cuts = [1000 + 997 * k for k in range(1, len(offsets))]
    acc = gpu.Stats(fmt)
    keep = push_device_pieces(gpu, acc, raw, fmt, [c for c in cuts if c < n], offsets)
    assert result(acc) == base
    del keep


def test_read_observes_reset_equals_fresh_and_two_handles_agree(gpu):
    raw, base = reference(gpu, "cs16", "2 P + 3")
    n, P = sizes()["2 P + 3"], stats.geometry()
    a, b = gpu.Stats("cs16"), gpu.Stats("cs16")
    fresh = result(a)
    assert fresh == bytes(C.sizeof(a.read()))                 # nothing pushed: all zero
    for cut in (1, 700, P, P + 1, n - 1):
        a.reset()
        a.push(raw[:cut * 4])
        mid = result(a)
        assert mid == result(a) == result(one_call(gpu, raw[:cut * 4], "cs16")), cut     # read twice: the same; a function of the frames
        a.push(raw[cut * 4:])
        assert result(a) == base, cut
    b.push(raw)
    assert result(b) == base
    b.push(np.zeros(0, np.uint8))                             # frames == 0 changes nothing
    assert result(b) == base
    a.reset()
    assert result(a) == fresh
    a.push(raw)
    assert result(a) == base


# ---- 4. nothing outside is read ----
@pytest.mark.parametrize("fmt", ("cf32", "cs16"))
def test_nothing_outside_the_pushed_frames_is_read(gpu, fmt):
    raw, base = reference(gpu, fmt, "P + 1")
    n, bpf, guard = sizes()["P + 1"], BPF[fmt], 4096
    if fmt == "cf32":
        g = np.full(2 * guard, np.nan, np.float32).view(np.uint8)
    else:
        g = np.tile(np.array([32767, -32768], np.int16), guard).view(np.uint8)
    clean = raw.copy()
    if fmt == "cs16":                                          # no rail code inside: any count is a guard frame's
        c = clean.view(np.int16)
        c[(c == 32767) | (c == -32768)] = 5
        base = result(one_call(gpu, clean, fmt))
    buf = np.concatenate([g, clean, g])
    d = gpu.DeviceBuffer(buf.size)
    d.upload(buf)
    half = n // 2 + 1
    acc = gpu.Stats(fmt)
    acc.push_device(d.ptr + guard * bpf, half)
    acc.push_device(d.ptr + (guard + half) * bpf, n - half)
    r = acc.read()
    assert bytes(r) == base
    assert r.nonfinite_frames == 0 and r.frames == n
    if fmt == "cs16":
        assert list(r.rail_lo) + list(r.rail_hi) == [0] * 4


# ---- 5. non-finite frames ----
def test_cf32_nonfinite_frames_are_counted_and_skipped(gpu, oracle):
    raw, _ = reference(gpu, "cf32", "2 P + 3")
    n, P = sizes()["2 P + 3"], stats.geometry()
    v = raw.copy().view(np.float32).reshape(-1, 2)
    bad = {0: (np.nan, 0.0), 1: (0.0, np.inf), 77: (-np.inf, np.nan), P - 1: (np.nan, np.nan), P: (np.inf, 0.5), n - 1: (0.25, -np.inf)}
    for i, pair in bad.items():
        v[i] = pair
    peak_at = P + 5
    v[peak_at] = (1.75, -1.75)                                 # the peak lies behind planted frames: its index still counts them
    got = stats.as_dict(one_call(gpu, v, "cf32").read())
    want, terms = model(v, "cf32", oracle)
    assert want["nonfinite_frames"] == len(bad) and want["peak_frame"] == peak_at
    for k in EXACT:
        assert got[k] == want[k], (k, got[k], want[k])
    check_sums(got, terms, n)
    # every other field: the stream with those frames removed
    removed = np.delete(v, sorted(bad), axis=0)
    rest = stats.as_dict(one_call(gpu, removed, "cf32").read())
    for k in ("rail_lo", "rail_hi", "hist", "min", "max", "peak_power"):
        assert got[k] == rest[k], k
    assert rest["frames"] == n - len(bad) and rest["nonfinite_frames"] == 0
    only = stats.as_dict(one_call(gpu, np.full((5, 2), np.nan, np.float32), "cf32").read())
    assert only["frames"] == 5 == only["nonfinite_frames"] and only["peak_power"] == 0.0 and only["min"] == [0.0, 0.0] and sum(only["hist"][0]) == 0


# ---- 6. merge ----
@pytest.mark.parametrize("fmt", ("cs16", "cf32", "cu8"))
def test_merge_of_four_handles_equals_one(gpu, oracle, fmt):
    raw, base = reference(gpu, fmt, "2 P + 3")
    n, P, bpf = sizes()["2 P + 3"], stats.geometry(), BPF[fmt]
    cuts = [0, 12345, P + 777, 2 * P - 1, n]
    parts = [one_call(gpu, raw[a * bpf:b * bpf], fmt).read() for a, b in zip(cuts[:-1], cuts[1:])]
    merged = stats.copy(parts[0])
    for p in parts[1:]:
        stats.merge(merged, p)
    one = stats.StatsResult.from_buffer_copy(base)
    got, want = stats.as_dict(merged), stats.as_dict(one)
    for k in EXACT:
        assert got[k] == want[k], k
    _, terms = model(raw, fmt, oracle)
    check_sums(got, terms, n)


# ---- 7. behind a chain ----
def test_behind_a_chain_on_its_stream(gpu):
    kw = dict(in_format="cs16", out_format="cs8", input_rate_hz=RATE, target_rate_hz=744187.5, shift_hz=200e3, gain=40.0)
    n = 1 << 18
    raw = synth.raw_stream(n, RATE, 31, "cs16")
    plain = gpu.Chain(**kw).process(raw)                      # no accumulator in play
    ch = gpu.Chain(**kw)
    cap = (ch.next_out_frames(n) + 1) * 2
    d_in, d_out = gpu.DeviceBuffer(raw.nbytes), gpu.DeviceBuffer(cap)
    d_in.upload(raw)
    acc_in, acc_out = gpu.Stats("cs16"), gpu.Stats("cs8")
    acc_in.push_device(d_in.ptr, n, ch.get_stream())
    got = ch.process_device(d_in.ptr, n, d_out.ptr, cap)
    acc_out.push_device(d_out.ptr, got, ch.get_stream())
    r_out, r_in = acc_out.read(), acc_in.read()
    ch.synchronize()
    out = d_out.download(got * 2, np.int8)
    assert np.array_equal(out, plain)
    assert bytes(r_out) == result(one_call(gpu, plain, "cs8")) and r_out.frames == got
    assert bytes(r_in) == result(one_call(gpu, raw, "cs16")) and r_in.frames == n
    assert r_out.rail_hi[0] > 0 and r_out.rail_hi[0] == int((plain.reshape(-1, 2)[:, 0] == 127).sum())


# ---- 8. the harness ----
ARGS = ["--raw-file-input-rate", "2.4e6", "--raw-file-input-sample-format", "cs16", "--output-rate", "744187.5",
        "--output-sample-format", "cs16", "--freq-shift", "200e3"]


def json_record(r):
    d = stats.as_dict(r)
    d["derived"] = stats.as_dict(stats.derive(r))
    return d


def test_harness_stats_plain_run(gpu, tmp_path):
    n = 1 << 18
    raw = synth.raw_stream(n, RATE, 37, "cs16")
    fin, fout, prefix = tmp_path / "in.cs16", tmp_path / "out.cs16", tmp_path / "st"
    raw.tofile(fin)
    r = subprocess.run([EXE, "-i", str(fin), "-o", str(fout), *ARGS, "--chunk-frames", "50000", "--stats", str(prefix)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    out = np.fromfile(fout, np.int16)
    meta = json.loads(open(str(prefix) + ".json").read())
    assert meta["shards"] == 1
    for side, data in (("in", raw), ("out", out)):
        want = json_record(one_call(gpu, data, "cs16").read())
        assert set(meta[side]) == set(want)
        for k, w in want.items():
            assert meta[side][k] == w, (side, k)                # == on the parsed doubles too


def test_harness_stats_shards_merge_in_shard_order(gpu, tmp_path):
    n = (1 << 18) + 10
    raw = synth.raw_stream(n, RATE, 38, "cs16")
    fin, fout, prefix = tmp_path / "in.cs16", tmp_path / "out.cs16", tmp_path / "st"
    raw.tofile(fin)
    r = subprocess.run([EXE, "-i", str(fin), "-o", str(fout), *ARGS, "--chunk-frames", "50000", "--shards", "2", "--stats", str(prefix)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    out = np.fromfile(fout, np.int16)
    meta = json.loads(open(str(prefix) + ".json").read())
    assert meta["shards"] == 2
    per = n // 2                                                # the harness's plan: equal ranges, the last takes the rest
    out_cut = gpu.design_out_frames(per, **dict(in_format="cs16", out_format="cs16", input_rate_hz=RATE, target_rate_hz=744187.5, shift_hz=200e3))
    for side, data, cut in (("in", raw, per), ("out", out, out_cut)):
        data = np.ascontiguousarray(data).view(np.uint8)
        a, b = one_call(gpu, data[:cut * 4], "cs16").read(), one_call(gpu, data[cut * 4:], "cs16").read()
        want = json_record(stats.merge(a, b))                   # Python's result for the same bytes, merged the same way: every field equal
        for k, w in want.items():
            assert meta[side][k] == w, (side, k)
        whole = stats.as_dict(one_call(gpu, data, "cs16").read())
        for k in EXACT:
            assert meta[side][k] == whole[k], (side, k)         # ... and the exact fields are the single stream's


def test_harness_stats_excludes_the_seamless_modes(gpu, tmp_path):
    base = ["--synthetic", "100000", "--synthetic-hash", "3", *ARGS, "--stats", str(tmp_path / "st")]
    for extra in (["--shards", "2", "--seamless"], ["--shards", "2", "--seamless-agc"], ["--iq-calibrate"]):
        r = subprocess.run([EXE, *base, *extra], capture_output=True, text=True)
        assert r.returncode == 2 and "usage" in r.stderr and "--stats" in r.stderr, (extra, r.returncode, r.stderr)
    assert not list(tmp_path.iterdir())
