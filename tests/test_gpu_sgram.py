"""The row accumulator on the device (include/iqgpu.h "spectrogram"; k_sgram_cells / k_sgram_fold).

1. Rows equal the power spectrum's, bit for bit: every finished row is float32(sum_power) / peak_power of a `Psd` pushed exactly the
   row's frames, the open row is the `Psd` of the remaining segments' frames (doubles as bytes).  R = 1, 3, 32, 33, 70: a row of one
   segment, of one short cell, of exactly one cell, of a cell and a one-segment cell, of two cells and a short one.  Those run Hann
   at gain 1; Blackman-Harris at gain 0.5 and the rectangular window at gain 2 at R = 3 pin how the two options reach the stream core.
2. Against float64, independent of the PSD code.  `want` is the numpy float64 periodogram of the frames unpacked by the oracle's
   conversion and windowed with the library's float32 table, summed (row_sum) or maximised (row_peak) per row.  Bar, per row and bin:
   |got - want| <= A want + B max_row(want).  A and B are 8 x the error of a FLOAT32 transform (scipy.fft.fft on complex64, powers
   re^2 + im^2 in float32, summed in double, rounded to float32) against the float64 one on these very inputs, measured on the CPU by
   `measure_f32_error` below (`PYTHONPATH=. python tests/test_gpu_sgram.py` prints it): a = the worst |err| / want over the bins with
   want >= 0.01 max_row(want), b = the worst |err| / max_row(want) over all bins, each the worst over all rows of all cases of test 2
   and over both outputs.
       measured  a = 3.14e-07 (row_peak, cs16, 2048 / 2048, R = 3)   b = 1.52e-07 (row_peak, cu8, 1024 / 256, R = 3)
       bars      A = 2.51e-06                                        B = 1.22e-06
   Measured on an MI355X, worst over the cases: row_sum a = 3.71e-07, b = 3.30e-07; row_peak a = 4.23e-07, b = 3.30e-07.
   The margin of 8 is the one tests/test_gpu_psd.py argues for: a radix-16 transform with another operation order and twiddles that
   are products of rounded table values may differ from scipy's by a small factor.
3. Any split of the stream into pushes gives the same row bytes in order and the same open row.   4. max_rows, capacity, guards.
5. Reset equals a fresh handle.   6. Behind a chain, on its stream.   7. The harness's --sgram.
Streams are synth.raw_stream, under 100 k frames."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from iq_tool_amd import psd, sgram, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "iq_tool_amd", "lib", "iqgpu_run")
RATE = 2.4e6
ECAPACITY = -8
A_BAR, B_BAR = 8 * 3.14e-07, 8 * 1.52e-07
BPF = dict(cu8=2, cs8=2, cu16=4, cs16=4, sc16q11=4, cs24=6, cu32=8, cs32=8, cf32=8)
ROW_SEGMENTS = (1, 3, 32, 33, 70)
# test 1: (format, nfft, hop, R)
EQUAL_CASES = ([(f, 1024, 256, R) for f in ("cs16", "cu8", "cf32", "cs24") for R in ROW_SEGMENTS]
               + [("cs16", 4096, 1024, 3), ("cs16", 2048, 2048, 3)])
# test 2
F64_CASES = [(f, 1024, 256, R) for f in ("cs16", "cu8", "cf32") for R in (1, 3, 33)] + [("cs16", 4096, 1024, 3), ("cs16", 2048, 2048, 3)]


def frames_for(segs, nfft, hop):
    return nfft + (segs - 1) * hop if segs > 0 else 0


def stream(n, fmt, seed=5):
    """n frames of three tones plus noise in the raw format, as bytes"""
    return np.ascontiguousarray(synth.raw_stream(n, RATE, seed, fmt)).view(np.uint8).reshape(-1)


_inputs = {}


def case_input(fmt, nfft, hop, R):
    """2 R + 1 segments and a ragged tail: two rows finish and one segment stays open (R = 1: three rows, nothing open)"""
    key = (fmt, nfft, hop, R)
    if key not in _inputs:
        n = frames_for(2 * R + 1, nfft, hop) + 37
        assert n < 100_000
        _inputs[key] = stream(n, fmt, seed=nfft + hop + R)
        _inputs[key].setflags(write=False)
    return _inputs[key]


def run(acc, feed):
    """feed(acc) -> [(row_sum, row_peak)] of its pushes; (row_sum bytes, row_peak bytes, open sum bytes, open peak bytes, info)"""
    parts = feed(acc)
    s, k, info = acc.read_open()
    rs = np.concatenate([p[0] for p in parts]) if parts else np.empty((0, acc.nfft), np.float32)
    rp = np.concatenate([p[1] for p in parts]) if parts else np.empty((0, acc.nfft), np.float32)
    assert rs.shape == rp.shape == (info["rows"], acc.nfft) and rs.dtype == rp.dtype == np.float32
    return rs.tobytes(), rp.tobytes(), s.tobytes(), k.tobytes(), info


def one_call(gpu, raw, fmt, nfft=1024, hop=256, R=32, **kw):
    acc = gpu.Sgram(fmt, nfft=nfft, hop=hop, row_segments=R, **kw)
    return run(acc, lambda a: [a.push(raw)])


# ---- 1. rows equal the power spectrum's ----
@pytest.mark.parametrize("fmt,nfft,hop,R", EQUAL_CASES)
def test_rows_equal_the_psd_of_their_frames(gpu, fmt, nfft, hop, R):
    raw, bpf = case_input(fmt, nfft, hop, R), BPF[fmt]
    n = raw.size // bpf
    acc = gpu.Sgram(fmt, nfft=nfft, hop=hop, row_segments=R)
    row_sum, row_peak = acc.push(raw)
    open_sum, open_peak, info = acc.read_open()
    segs = psd.segments(n, nfft, hop)
    rows, open_segs = segs // R, segs % R
    assert segs == 2 * R + 1 and row_sum.shape == row_peak.shape == (rows, nfft) and rows >= 2
    assert info == dict(frames=n, segments=segs, rows=rows, open_segments=open_segs, nfft=nfft, hop=hop, row_segments=R,
                        window_sum=info["window_sum"], window_sum_sq=info["window_sum_sq"])
    ref = gpu.Psd(fmt, nfft=nfft, hop=hop)
    for r in range(rows):
        first = r * R * hop
        ref.reset()
        ref.push(raw[first * bpf:(first + frames_for(R, nfft, hop)) * bpf])
        s, k, ref_info = ref.read()
        assert ref_info["segments"] == R
        assert row_sum[r].tobytes() == s.astype(np.float32).tobytes(), "row_sum of row %d" % r
        assert row_peak[r].tobytes() == k.tobytes(), "row_peak of row %d" % r
    ref.reset()
    first = rows * R * hop
    ref.push(raw[first * bpf:(first + frames_for(open_segs, nfft, hop)) * bpf])
    s, k, ref_info = ref.read()
    assert ref_info["segments"] == info["open_segments"]
    assert (ref_info["window_sum"], ref_info["window_sum_sq"]) == (info["window_sum"], info["window_sum_sq"])
    assert open_sum.tobytes() == s.tobytes() and open_peak.tobytes() == k.tobytes()


@pytest.mark.parametrize("window,gain", [("blackman_harris", 0.5), ("rect", 2.0)])
def test_window_and_gain_reach_the_rows_as_they_reach_the_psd(gpu, window, gain):
    """the other tests run Hann at gain 1: here the two options travel from iqgpu_sgram_opts into the stream core that the Psd holds too"""
    fmt, nfft, hop, R, bpf = "cs16", 1024, 256, 3, 4
    raw = case_input(fmt, nfft, hop, R)
    assert raw.size // bpf == 2597
    acc = gpu.Sgram(fmt, nfft=nfft, hop=hop, window=window, gain=gain, row_segments=R)
    row_sum, row_peak = acc.push(raw)
    open_sum, open_peak, info = acc.read_open()
    assert row_sum.shape == row_peak.shape == (2, nfft) and info["open_segments"] == 1
    for r in range(3):                     # the two finished rows, then the open one
        first, segs = r * R * hop, R if r < 2 else 1
        ref = gpu.Psd(fmt, nfft=nfft, hop=hop, window=window, gain=gain)
        ref.push(raw[first * bpf:(first + frames_for(segs, nfft, hop)) * bpf])
        s, k, ref_info = ref.read()
        assert ref_info["segments"] == segs and s.any()
        assert (ref_info["window_sum"], ref_info["window_sum_sq"]) == (info["window_sum"], info["window_sum_sq"])
        if r < 2:
            assert row_sum[r].tobytes() == s.astype(np.float32).tobytes(), "row_sum of row %d" % r
            assert row_peak[r].tobytes() == k.tobytes(), "row_peak of row %d" % r
        else:
            assert open_sum.tobytes() == s.tobytes() and open_peak.tobytes() == k.tobytes()


@pytest.mark.parametrize("R,open_segs", [(70, 31), (70, 32), (70, 33), (70, 69), (33, 32), (3, 2), (40, 0)])
def test_open_row_equals_the_psd_of_its_frames(gpu, R, open_segs):
    """the open row at every kind of position: inside the first cell, on a cell boundary, behind one, in the short last cell, empty"""
    nfft, hop = 1024, 256
    raw = stream(frames_for(R + open_segs, nfft, hop) + 200, "cs16", seed=41)
    acc = gpu.Sgram("cs16", nfft=nfft, hop=hop, row_segments=R)
    acc.push(raw)
    s, k, info = acc.read_open()
    assert info["rows"] == 1 and info["open_segments"] == open_segs
    ref = gpu.Psd("cs16", nfft=nfft, hop=hop)
    ref.push(raw[R * hop * 4:(R * hop + frames_for(open_segs, nfft, hop)) * 4])
    ws, wk, ref_info = ref.read()
    assert ref_info["segments"] == open_segs
    assert s.tobytes() == ws.tobytes() and k.tobytes() == wk.tobytes()
    again = acc.read_open()                # observes, does not disturb
    assert (s.tobytes(), k.tobytes(), info) == (again[0].tobytes(), again[1].tobytes(), again[2])


# ---- 2. against float64 ----
def windowed_segments(oracle, raw, fmt, nfft, hop):
    x = oracle.to_cf32(raw, fmt, 1.0).astype(np.complex128)
    w = psd.window(nfft, "hann")[0].astype(np.float64)
    n = psd.segments(x.size, nfft, hop)
    idx = np.arange(n)[:, None] * hop + np.arange(nfft)[None, :]
    return x[idx] * w


def per_row(p, R, how):
    rows = p.shape[0] // R
    return how(p[:rows * R].reshape(rows, R, -1), axis=1)


def reference(oracle, raw, fmt, nfft, hop, R):
    """(row_sum, row_peak) in float64, [rows, nfft]"""
    X = np.fft.fft(windowed_segments(oracle, raw, fmt, nfft, hop), axis=1)
    p = X.real ** 2 + X.imag ** 2
    return per_row(p, R, np.sum), per_row(p, R, np.max)


def error_figures(got, want):
    """(a, b) over [rows, nfft]: the worst |err| / want over each row's strong bins, the worst |err| / max_row(want) over all"""
    err, top = np.abs(got.astype(np.float64) - want), want.max(axis=1, keepdims=True)
    strong = want >= 0.01 * top
    return float((err[strong] / want[strong]).max()), float((err / top).max())


def measure_f32_error(oracle):
    """the float32 transform against the float64 one on the inputs of test 2, on the CPU: [(a, b, what)]"""
    import scipy.fft
    out = []
    for fmt, nfft, hop, R in F64_CASES:
        raw = case_input(fmt, nfft, hop, R)
        X = scipy.fft.fft(windowed_segments(oracle, raw, fmt, nfft, hop).astype(np.complex64), axis=1)
        assert X.dtype == np.complex64
        p = X.real * X.real + X.imag * X.imag
        assert p.dtype == np.float32
        want_sum, want_peak = reference(oracle, raw, fmt, nfft, hop, R)
        got_sum = per_row(p.astype(np.float64), R, np.sum).astype(np.float32)
        for name, got, want in (("row_sum", got_sum, want_sum), ("row_peak", per_row(p, R, np.max), want_peak)):
            a, b = error_figures(got, want)
            out.append((a, b, "%s, %s, %d / %d, R = %d" % (name, fmt, nfft, hop, R)))
    return out


@pytest.mark.parametrize("fmt,nfft,hop,R", F64_CASES)
def test_against_float64(gpu, oracle, fmt, nfft, hop, R):
    raw = case_input(fmt, nfft, hop, R)
    got_sum, got_peak = gpu.Sgram(fmt, nfft=nfft, hop=hop, row_segments=R).push(raw)
    want_sum, want_peak = reference(oracle, raw, fmt, nfft, hop, R)
    assert got_sum.shape == want_sum.shape == ((2 * R + 1) // R, nfft)
    for name, got, want in (("row_sum", got_sum, want_sum), ("row_peak", got_peak, want_peak)):
        a, b = error_figures(got, want)
        excess = np.abs(got.astype(np.float64) - want) - (A_BAR * want + B_BAR * want.max(axis=1, keepdims=True))
        print("%s %s %d/%d R=%d: a = %.3g (bar %.3g), b = %.3g (bar %.3g), worst excess over the bar %.3g" % (name, fmt, nfft, hop, R, a, A_BAR, b, B_BAR, excess.max()))
        assert np.isfinite(got).all() and excess.max() <= 0.0, (name, int(excess.argmax()), float(excess.max()))


# ---- 3. split invariance, bit for bit ----
class DevicePushes:
    """device pushes whose buffers live until the rows are fetched; rows() synchronises through read_open"""

    def __init__(self, gpu, acc):
        self.gpu, self.acc, self.kept = gpu, acc, []

    def push(self, piece, frames, stream=None):
        cap = self.acc.max_rows(frames)
        d = self.gpu.DeviceBuffer(max(piece.size, 1))
        d.upload(piece)
        planes = [self.gpu.DeviceBuffer(max(cap, 1) * self.acc.nfft * 4) for _ in range(2)]
        got = self.acc.push_device(d.ptr, frames, planes[0].ptr, planes[1].ptr, cap, stream)
        assert got == cap
        self.kept.append((d, planes, got))
        return len(self.kept) - 1

    def rows(self, i):
        self.acc.read_open()
        _, planes, got = self.kept[i]
        n = got * self.acc.nfft
        return tuple(p.download(n * 4, np.float32).reshape(got, self.acc.nfft) for p in planes)


def split_variants(gpu, raw, fmt, nfft, hop, R, single_frames):
    bpf = BPF[fmt]
    n = raw.size // bpf

    def pieces(cuts):
        cuts = sorted({c for c in cuts if 0 < c < n} | {0, n})
        return [(raw[a * bpf:b * bpf], b - a) for a, b in zip(cuts[:-1], cuts[1:])]

    def host(cuts):
        return lambda acc: [acc.push(p) for p, _ in pieces(cuts)]

    def mixed(acc):
        dev, out = DevicePushes(gpu, acc), []
        for turn, (p, m) in enumerate(pieces(range(0, n, 1777))):
            out.append(dev.push(p, m) if turn % 2 else acc.push(p))
        return [dev.rows(x) if isinstance(x, int) else x for x in out]

    def two_streams(acc):
        lib, streams = gpu.load(), [C.c_void_p(), C.c_void_p()]
        for s in streams:
            assert lib.iqgpu_stream_create(0, C.byref(s)) == 0
        dev = DevicePushes(gpu, acc)
        ids = [dev.push(p, m, streams[turn % 2].value) for turn, (p, m) in enumerate(pieces(range(0, n, 2 * R * hop // 3 + 11)))]
        out = [dev.rows(i) for i in ids]
        for s in streams:
            assert lib.iqgpu_stream_destroy(s) == 0
        return out

    row_ends = [frames_for((r + 1) * R, nfft, hop) for r in range((2 * R + 1) // R)]
    v = {"one push": host([]), "1000 frames": host(range(0, n, 1000)),
         "on the row boundaries": host(row_ends), "one frame before": host([e - 1 for e in row_ends]), "one frame after": host([e + 1 for e in row_ends]),
         "before, on and after": host([e + d for e in row_ends for d in (-1, 0, 1)]),
         "host and device": mixed, "two streams": two_streams}
    if single_frames:
        v["single frames"] = host(range(n))
    return v


@pytest.mark.parametrize("fmt,nfft,hop,R", [("cs16", 1024, 256, 1), ("cs16", 1024, 256, 3), ("cs24", 1024, 256, 33), ("cs16", 1024, 512, 70),
                                             ("cf32", 1024, 256, 32), ("cu8", 2048, 2048, 3)])
def test_any_split_gives_the_same_rows(gpu, fmt, nfft, hop, R):
    raw = case_input(fmt, nfft, hop, R)
    want = None
    for name, feed in split_variants(gpu, raw, fmt, nfft, hop, R, single_frames=R == 1).items():
        got = run(gpu.Sgram(fmt, nfft=nfft, hop=hop, row_segments=R), feed)
        assert got[4]["rows"] == (2 * R + 1) // R and got[4]["open_segments"] == (2 * R + 1) % R, name
        if want is None:
            want = got
        for what, g, w in zip(("row_sum", "row_peak", "open sum", "open peak", "info"), got, want):
            assert g == w, "%s differs: %s" % (what, name)


# ---- 4. max_rows, capacity, guards ----
def test_max_rows_is_what_the_next_push_returns(gpu):
    nfft, hop, R = 1024, 256, 3
    raw = stream(40_000, "cs16", seed=43)
    acc = gpu.Sgram("cs16", nfft=nfft, hop=hop, row_segments=R)
    at, total = 0, 0
    for m in (0, 1, 1023, 1, 255, 256, 3 * 256, 3 * 256 - 1, 1, 5000, 1, 12345):
        want = sgram.rows(at + m, nfft, hop, R) - sgram.rows(at, nfft, hop, R)
        assert acc.max_rows(m) == want
        assert acc.max_rows(0) == 0
        got = acc.push(raw[at * 4:(at + m) * 4])[0].shape[0]
        assert got == want, (at, m)
        at, total = at + m, total + got
    assert total == sgram.rows(at, nfft, hop, R) == acc.read_open()[2]["rows"]


def test_capacity_is_checked_before_anything_is_queued(gpu):
    nfft, hop, R, lib = 1024, 256, 3, gpu.load()
    raw = stream(20_000, "cs16", seed=47)
    head, rest = raw[:5003 * 4], raw[5003 * 4:]
    a, b = gpu.Sgram("cs16", nfft=nfft, hop=hop, row_segments=R), gpu.Sgram("cs16", nfft=nfft, hop=hop, row_segments=R)
    first = [x.push(head) for x in (a, b)]
    n = rest.size // 4
    need = a.max_rows(n)
    assert need >= 2
    planes = [np.full((need, nfft), -7.0, np.float32) for _ in range(2)]
    got = C.c_size_t(99)
    args = (rest.ctypes.data_as(C.c_void_p), n, planes[0].ctypes.data_as(C.c_void_p), planes[1].ctypes.data_as(C.c_void_p))
    assert lib.iqgpu_sgram_push(a._h, *args, need - 1, C.byref(got)) == ECAPACITY and got.value == 0
    assert (planes[0] == -7.0).all() and (planes[1] == -7.0).all()
    d = gpu.DeviceBuffer(rest.size)
    d.upload(rest)
    d_rows = gpu.DeviceBuffer(need * nfft * 4)
    with pytest.raises(gpu.IqgpuError) as e:
        a.push_device(d.ptr, n, d_rows.ptr, 0, need - 1)
    assert e.value.code == ECAPACITY
    assert a.max_rows(n) == need and a.read_open()[2]["frames"] == 5003
    assert run(a, lambda x: [first[0], x.push(rest)]) == run(b, lambda x: [first[1], x.push(rest)])


def test_output_planes_are_written_up_to_rows_and_a_null_plane_is_left_out(gpu):
    nfft, hop, R = 1024, 256, 3
    raw = stream(frames_for(4 * R + 2, nfft, hop) + 100, "cs16", seed=53)
    n = raw.size // 4
    want = one_call(gpu, raw, "cs16", nfft, hop, R)
    d = gpu.DeviceBuffer(raw.size)
    d.upload(raw)
    guard, rows = 2, 4
    sentinel = np.full((guard + rows + guard, nfft), -3.0, np.float32)
    for which in ("both", "sum only", "peak only", "neither"):
        acc = gpu.Sgram("cs16", nfft=nfft, hop=hop, row_segments=R)
        planes = [gpu.DeviceBuffer(sentinel.nbytes) for _ in range(2)]
        for p in planes:
            p.upload(sentinel)
        ptr = [p.ptr + guard * nfft * 4 for p in planes]
        ps = ptr[0] if which in ("both", "sum only") else 0
        pp = ptr[1] if which in ("both", "peak only") else 0
        # room for more rows than the push finishes: what lies behind `rows` stays as it was
        assert acc.push_device(d.ptr, n, ps, pp, rows + guard) == rows
        s, k, info = acc.read_open()
        assert (s.tobytes(), k.tobytes(), info) == want[2:]
        for plane, given, ref in ((planes[0], ps, want[0]), (planes[1], pp, want[1])):
            host = plane.download(sentinel.nbytes, np.float32).reshape(sentinel.shape)
            assert (host[:guard] == -3.0).all() and (host[guard + rows:] == -3.0).all(), which
            if given:
                assert host[guard:guard + rows].tobytes() == ref, which
            else:
                assert (host == -3.0).all(), which


@pytest.mark.parametrize("R", [1, 40])
def test_nothing_outside_the_pushed_frames_is_read(gpu, R):
    nfft, hop, guard = 1024, 256, 4096
    n = frames_for(2 * R + 5, nfft, hop) + hop // 2
    x = synth.complex_signal(n, RATE, 29)
    buf = np.full(n + 2 * guard, np.nan + 1j * np.nan, np.complex64)
    buf[guard:guard + n] = x
    d = gpu.DeviceBuffer(buf.nbytes)
    d.upload(buf)
    acc = gpu.Sgram("cf32", nfft=nfft, hop=hop, row_segments=R)
    half = n // 2 + 3
    cap = acc.max_rows(n)
    planes = [gpu.DeviceBuffer(cap * nfft * 4) for _ in range(2)]
    r0 = acc.push_device(d.ptr + guard * 8, half, planes[0].ptr, planes[1].ptr, cap)
    r1 = acc.push_device(d.ptr + (guard + half) * 8, n - half, planes[0].ptr + r0 * nfft * 4, planes[1].ptr + r0 * nfft * 4, cap - r0)
    s, k, info = acc.read_open()
    got = [p.download((r0 + r1) * nfft * 4, np.float32) for p in planes]
    assert all(np.isfinite(v).all() for v in (s, k, *got)) and r0 + r1 == info["rows"] == (2 * R + 5) // R
    assert (got[0].tobytes(), got[1].tobytes(), s.tobytes(), k.tobytes(), info) == one_call(gpu, x, "cf32", nfft, hop, R)


# ---- 5. reset ----
@pytest.mark.parametrize("R,cut_segs", [(70, 45), (3, 4)])
def test_reset_equals_a_fresh_handle(gpu, R, cut_segs):
    nfft, hop = 1024, 256
    raw = case_input("cs16", nfft, hop, R)
    other = stream(frames_for(cut_segs, nfft, hop) + 77, "cs16", seed=59)      # ends in mid-row and mid-cell, with a carry
    acc = gpu.Sgram("cs16", nfft=nfft, hop=hop, row_segments=R)
    acc.push(other)
    before = acc.read_open()
    assert before[2]["open_segments"] == cut_segs % R and before[0].any()
    empty = acc.push(raw[:0])
    assert empty[0].shape == empty[1].shape == (0, nfft)
    after = acc.read_open()
    assert before[2] == after[2] and before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
    acc.reset()
    s, k, info = acc.read_open()
    fresh = gpu.Sgram("cs16", nfft=nfft, hop=hop, row_segments=R).read_open()
    assert not s.any() and not k.any() and info == fresh[2] and info["frames"] == info["segments"] == info["rows"] == info["open_segments"] == 0
    assert run(acc, lambda a: [a.push(raw[:3001 * 4]), a.push(raw[3001 * 4:])]) == one_call(gpu, raw, "cs16", nfft, hop, R)


# ---- 6. behind a chain ----
def test_on_a_chains_stream(gpu):
    kw = dict(in_format="cs16", out_format="cs16", input_rate_hz=RATE, target_rate_hz=744187.5, shift_hz=200e3)
    nfft, hop, R = 1024, 256, 8
    calls = (70_001, 33_333, 90_000)
    n = sum(calls)
    raw = synth.raw_stream(n, RATE, 31, "cs16")
    plain = gpu.Chain(**kw).process(raw)                     # no accumulator in play
    ch = gpu.Chain(**kw)
    acc = gpu.Sgram("cs16", nfft=nfft, hop=hop, row_segments=R)
    d_in = gpu.DeviceBuffer(raw.nbytes)
    d_in.upload(raw)
    kept, at = [], 0
    for m in calls:
        cap = (ch.next_out_frames(m) + 1) * 4
        d_out = gpu.DeviceBuffer(cap)
        got = ch.process_device(d_in.ptr + at * 4, m, d_out.ptr, cap)
        rows = acc.max_rows(got)
        planes = [gpu.DeviceBuffer(max(rows, 1) * nfft * 4) for _ in range(2)]
        assert acc.push_device(d_out.ptr, got, planes[0].ptr, planes[1].ptr, rows, ch.get_stream()) == rows
        kept.append((d_out, got, planes, rows))
        at += m
    s, k, info = acc.read_open()
    ch.synchronize()
    out = np.concatenate([d.download(got * 4, np.int16) for d, got, _, _ in kept])
    assert np.array_equal(out, plain) and info["frames"] == out.size // 2
    rs = np.concatenate([p[0].download(r * nfft * 4, np.float32) for _, _, p, r in kept])
    rp = np.concatenate([p[1].download(r * nfft * 4, np.float32) for _, _, p, r in kept])
    assert info["rows"] >= 10
    assert (rs.tobytes(), rp.tobytes(), s.tobytes(), k.tobytes(), info) == one_call(gpu, plain, "cs16", nfft, hop, R)


# ---- 7. the harness ----
ARGS = ["--raw-file-input-rate", "2.4e6", "--raw-file-input-sample-format", "cs16", "--output-rate", "744187.5",
        "--output-sample-format", "cs16", "--freq-shift", "200e3"]


def test_harness_sgram(gpu, tmp_path):
    n = 65536
    raw = synth.raw_stream(n, RATE, 37, "cs16")
    fin, fout, prefix = tmp_path / "in.cs16", tmp_path / "out.cs16", tmp_path / "gram"
    raw.tofile(fin)
    r = subprocess.run([EXE, "-i", str(fin), "-o", str(fout), *ARGS, "--chunk-frames", "20000", "--sgram", str(prefix), "--sgram-row-segments", "8"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    out = np.fromfile(fout, np.int16)
    meta = json.loads(open(str(prefix) + ".json").read())
    for side, data, rate in (("in", np.fromfile(fin, np.int16), 2.4e6), ("out", out, 744187.5)):
        acc = gpu.Sgram("cs16", row_segments=8)
        want_sum, _ = acc.push(data)
        info = acc.read_open()[2]
        got = np.fromfile(str(prefix) + "." + side + ".f32", "<f4")
        assert info["rows"] >= 3 and got.size == info["rows"] * 1024 and got.tobytes() == want_sum.tobytes(), side
        m = meta[side]
        assert m["rate_hz"] == rate and {k: m[k] for k in info} == info
        assert m["row_segments"] == 8 and m["window"] == "hann" and m["file"] == str(prefix) + "." + side + ".f32"


def test_harness_sgram_excludes_shards(gpu, tmp_path):
    base = ["--synthetic", "100000", "--synthetic-hash", "3", *ARGS, "--sgram", str(tmp_path / "gram")]
    for extra in (["--shards", "2"], ["--shards", "2", "--seamless"], ["--iq-calibrate"]):
        r = subprocess.run([EXE, *base, *extra], capture_output=True, text=True)
        assert r.returncode == 2 and "usage" in r.stderr and "--sgram" in r.stderr, (extra, r.returncode, r.stderr)
    assert not list(tmp_path.iterdir())


if __name__ == "__main__":
    from oracle import pyoracle
    pyoracle.build()
    figures = measure_f32_error(pyoracle)
    for a, b, what in figures:
        print("a = %.3g  b = %.3g  %s" % (a, b, what))
    wa, wb = max(figures, key=lambda r: r[0]), max(figures, key=lambda r: r[1])
    print("worst a = %.3g (%s)\nworst b = %.3g (%s)\nbars: A = %.3g, B = %.3g" % (wa[0], wa[2], wb[1], wb[2], 8 * wa[0], 8 * wb[1]))
