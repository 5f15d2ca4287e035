"""The power-spectrum accumulator on the device (include/iqgpu.h "power spectrum"; k_psd_pages / k_psd_fold / k_psd_carry).

1. Against float64.  `want` is the numpy float64 periodogram of the frames unpacked by the oracle's conversion and windowed with the
   library's float32 table.  Bar, per bin: |got - want| <= A want + B max(want), for sum_power and -- against the float64 maximum --
   for peak_power.  A and B are 8 x the error of a FLOAT32 transform (scipy.fft.fft on complex64, powers re^2 + im^2 in float32,
   summed in double) against the float64 one on these very inputs, measured on the CPU by `measure_f32_error` below
   (`PYTHONPATH=. python tests/test_gpu_psd.py` prints it): a = the worst |err| / want over the bins with want >= 0.01 max(want), b = the worst
   |err| / max(want) over all bins, each the worst over all cases of test 1 and over both outputs.
       measured  a = 2.72e-07 (peak_power, cu8, 1024 / 512, blackman_harris)   b = 1.66e-07 (peak_power, cu8, 1024 / 512, rect)
       bars      A = 2.18e-06                                                  B = 1.33e-06
   (sum_power alone: a <= 1.12e-07, b <= 5.04e-08 -- the sum averages the rounding of its segments, the maximum does not.)
   Measured on an MI355X, worst over the cases: sum_power a = 2.34e-07, b = 2.34e-07; peak_power a = 3.56e-07, b = 3.56e-07.
   The margin of 8 is there because a radix-16 transform with another operation order and twiddles that are products of rounded
   table values may differ from scipy's by a small factor.
2. - 4.  Bit for bit: any split of the stream into pushes, host or device, gives the same bytes; read observes and does not disturb;
   two accumulators agree; reset equals a fresh handle; the carry across calls.
5. Guard frames of NaN around the device buffer: nothing outside the pushed frames is read.
6. With a chain, on its stream.   7. The harness's --psd.
Shapes: with G = psd.geometry() segments per page, streams of nfft - 1, nfft, nfft + 1 frames and the frame counts that give G - 1, G,
G + 1 and 2 G + 3 segments (under 70 k frames at nfft 1024)."""
import json
import os
import subprocess

import numpy as np
import pytest

from iq_tool_amd import psd, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "iq_tool_amd", "lib", "iqgpu_run")
RATE = 2.4e6
A_BAR, B_BAR = 8 * 2.72e-07, 8 * 1.66e-07
BPF = dict(cu8=2, cs8=2, cu16=4, cs16=4, sc16q11=4, cs24=6, cu32=8, cs32=8, cf32=8)
# test 1: (format, nfft, hop, window)
CASES = ([(f, 1024, 512, w) for w in ("rect", "hann", "hamming", "blackman_harris") for f in ("cs16", "cu8", "cf32")]
         + [(f, 2048, 2048, "hann") for f in ("cs16", "cu8", "cf32")] + [(f, 4096, 1024, "hann") for f in ("cs16", "cu8", "cf32")]
         + [(f, 1024, 512, "hann") for f in ("cs8", "cu16", "sc16q11", "cs24", "cu32", "cs32")])
# test 2; the 6-byte format (frame alignment 2) once, at the smallest hop
SPLIT_SHAPES = [("cs16", 1024, 1024), ("cs16", 1024, 512), ("cs16", 1024, 256), ("cs16", 4096, 1024), ("cs24", 1024, 256)]


def page_segments(name):
    G = psd.geometry()
    return {"G - 1": G - 1, "G": G, "G + 1": G + 1, "2 G + 3": 2 * G + 3}[name]


def frames_for(segs, nfft, hop):
    return nfft + (segs - 1) * hop


def stream(n, fmt, seed=5):
    """n frames of three tones plus noise in the raw format, as bytes"""
    return np.ascontiguousarray(synth.raw_stream(n, RATE, seed, fmt)).view(np.uint8).reshape(-1)


def case_input(fmt, nfft, hop):
    """test 1's stream of a case: G + 1 segments and a ragged tail, so that a page closes and one stays open"""
    n = frames_for(psd.geometry() + 1, nfft, hop) + 37
    return stream(n, fmt, seed=nfft + hop)


def windowed_segments(oracle, raw, fmt, nfft, hop, window, gain=1.0):
    x = oracle.to_cf32(raw, fmt, gain).astype(np.complex128)
    w = psd.window(nfft, window)[0].astype(np.float64)
    n = psd.segments(x.size, nfft, hop)
    idx = np.arange(n)[:, None] * hop + np.arange(nfft)[None, :]
    return x[idx] * w


def reference(oracle, raw, fmt, nfft, hop, window, gain=1.0):
    """(sum_power, peak_power) in float64"""
    X = np.fft.fft(windowed_segments(oracle, raw, fmt, nfft, hop, window, gain), axis=1)
    p = X.real ** 2 + X.imag ** 2
    return p.sum(axis=0), p.max(axis=0)


def error_figures(got, want):
    """(a, b): the worst |err| / want over the strong bins, the worst |err| / max(want) over all"""
    err, top = np.abs(got.astype(np.float64) - want), want.max()
    strong = want >= 0.01 * top
    return float((err[strong] / want[strong]).max()), float(err.max() / top)


def measure_f32_error(oracle):
    """the float32 transform against the float64 one on the inputs of test 1, on the CPU: [(a, b, what)]"""
    import scipy.fft
    rows = []
    for fmt, nfft, hop, window in CASES:
        raw = case_input(fmt, nfft, hop)
        seg = windowed_segments(oracle, raw, fmt, nfft, hop, window)
        X = scipy.fft.fft(seg.astype(np.complex64), axis=1)
        assert X.dtype == np.complex64
        p = X.real * X.real + X.imag * X.imag
        assert p.dtype == np.float32
        want_sum, want_peak = reference(oracle, raw, fmt, nfft, hop, window)
        for name, got, want in (("sum_power", p.astype(np.float64).sum(axis=0), want_sum), ("peak_power", p.max(axis=0), want_peak)):
            a, b = error_figures(got, want)
            rows.append((a, b, "%s, %s, %d / %d, %s" % (name, fmt, nfft, hop, window)))
    return rows


def result(acc):
    s, k, info = acc.read()
    return s.tobytes(), k.tobytes(), info


def one_call(gpu, raw, fmt, nfft, hop, window="hann", gain=1.0):
    acc = gpu.Psd(fmt, nfft=nfft, hop=hop, window=window, gain=gain)
    acc.push(raw)
    return acc


# ---- 1. against float64 ----
@pytest.mark.parametrize("fmt,nfft,hop,window", CASES)
def test_against_float64(gpu, oracle, fmt, nfft, hop, window):
    raw = case_input(fmt, nfft, hop)
    got_sum, got_peak, info = one_call(gpu, raw, fmt, nfft, hop, window).read()
    want_sum, want_peak = reference(oracle, raw, fmt, nfft, hop, window)
    n = raw.size // BPF[fmt]
    w = psd.window(nfft, window)[0].astype(np.float64)
    assert info == dict(frames=n, segments=psd.segments(n, nfft, hop), nfft=nfft, hop=hop, window_sum=info["window_sum"], window_sum_sq=info["window_sum_sq"])
    assert info["segments"] == psd.geometry() + 1
    assert abs(info["window_sum"] - w.sum()) <= 1e-12 * w.sum() and abs(info["window_sum_sq"] - (w * w).sum()) <= 1e-12 * (w * w).sum()
    for name, got, want in (("sum_power", got_sum, want_sum), ("peak_power", got_peak, want_peak)):
        a, b = error_figures(got, want)
        excess = np.abs(got.astype(np.float64) - want) - (A_BAR * want + B_BAR * want.max())
        print("%s %s %d/%d %s: a = %.3g (bar %.3g), b = %.3g (bar %.3g), worst excess over the bar %.3g" % (name, fmt, nfft, hop, window, a, A_BAR, b, B_BAR, excess.max()))
        assert np.isfinite(got).all() and excess.max() <= 0.0, (name, int(excess.argmax()), float(excess.max()))


def test_gain_is_applied_at_unpack(gpu, oracle):
    raw = case_input("cs16", 1024, 512)
    got_sum, got_peak, _ = one_call(gpu, raw, "cs16", 1024, 512, gain=0.37).read()
    want_sum, want_peak = reference(oracle, raw, "cs16", 1024, 512, "hann", gain=0.37)
    for got, want in ((got_sum, want_sum), (got_peak, want_peak)):
        assert (np.abs(got - want) <= A_BAR * want + B_BAR * want.max()).all()


def test_a_full_scale_tone_reads_zero_dbfs(gpu):
    n = 8192
    x = np.exp(2j * np.pi * 100 / 1024 * np.arange(n)).astype(np.complex64)
    acc = gpu.Psd("cf32")
    acc.push(x)
    freqs, mean, peak = acc.spectrum(RATE)
    k = int(np.argmax(mean))
    assert abs(freqs[k] - 100 / 1024 * RATE) < 1e-3 and abs(mean[k]) < 1e-3 and abs(peak[k]) < 1e-3
    assert freqs[0] == -RATE / 2 and freqs.size == 1024


# ---- 2. split invariance, bit for bit ----
def push_variants(gpu, raw, fmt, nfft, hop):
    """name -> function feeding a fresh accumulator the whole stream in its own way"""
    bpf, G = BPF[fmt], psd.geometry()
    n = raw.size // bpf

    def cut(acc, lengths, device_turns=()):
        """pushes of the given lengths, cycling, to the end of the stream; the turns listed go through device memory"""
        at, turn, keep = 0, 0, []
        while at < n:
            m = min(lengths[turn % len(lengths)], n - at)
            piece = raw[at * bpf:(at + m) * bpf]
            if turn % 2 in device_turns:
                d = gpu.DeviceBuffer(piece.size)
                d.upload(piece)
                acc.push_device(d.ptr, m)
                keep.append(d)
            else:
                acc.push(piece)
            at, turn = at + m, turn + 1
        acc.read()
        return keep

    def one(acc):
        acc.push(raw)

    def single_frames_then_rest(acc):
        head = nfft + 3
        for i in range(head):
            acc.push(raw[i * bpf:(i + 1) * bpf])
        acc.push(raw[head * bpf:])

    def at_page_ends(acc):
        # the first call ends with the last frame of page 0's last segment, every later one a page further
        first = frames_for(G, nfft, hop)
        acc.push(raw[:first * bpf])
        cut_rest = raw[first * bpf:]
        for at in range(0, cut_rest.size // bpf, G * hop):
            acc.push(cut_rest[at * bpf:(at + G * hop) * bpf])

    def offset_device_pointer(acc):
        d = gpu.DeviceBuffer(raw.size + bpf)
        d.upload(np.concatenate([np.full(bpf, 0xA5, np.uint8), raw]))
        acc.push_device(d.ptr + bpf, n)
        acc.read()

    return {"one call": one, "single frames, then the rest": single_frames_then_rest,
            "1023, 1025, hop, hop + 1 cycling": lambda acc: cut(acc, (1023, 1025, hop, hop + 1)),
            "cut at page ends": at_page_ends,
            "host and device alternating": lambda acc: cut(acc, (1023, 1025, hop, hop + 1, 7), device_turns=(1,)),
            "device pointer offset by one frame": offset_device_pointer}


@pytest.mark.parametrize("fmt,nfft,hop", SPLIT_SHAPES)
def test_any_split_gives_the_same_bytes(gpu, fmt, nfft, hop):
    G = psd.geometry()
    n = frames_for(2 * G + 3, nfft, hop) + hop - 1
    raw = stream(n, fmt, seed=11)
    want = None
    for name, feed in push_variants(gpu, raw, fmt, nfft, hop).items():
        acc = gpu.Psd(fmt, nfft=nfft, hop=hop)
        feed(acc)
        got = result(acc)
        assert got[2]["frames"] == n and got[2]["segments"] == 2 * G + 3, name
        if want is None:
            want = got
        assert got[0] == want[0], "sum_power differs: " + name
        assert got[1] == want[1], "peak_power differs: " + name
        assert got[2] == want[2], "info differs: " + name


# ---- 3. read is a pure observer ----
@pytest.mark.parametrize("segs_before", ["G - 1", "G", "G + 1"])
def test_read_observes_and_does_not_disturb(gpu, segs_before):
    nfft, hop, G = 1024, 256, psd.geometry()
    n = frames_for(2 * G + 3, nfft, hop)
    raw = stream(n, "cs16", seed=13)
    cut = frames_for(page_segments(segs_before), nfft, hop) + 100        # mid-segment, in mid-page (or just behind a page's end)
    whole = result(one_call(gpu, raw, "cs16", nfft, hop))
    prefix = result(one_call(gpu, raw[:cut * 4], "cs16", nfft, hop))
    acc = gpu.Psd("cs16", nfft=nfft, hop=hop)
    acc.push(raw[:cut * 4])
    mid = result(acc)
    assert mid == result(acc)              # twice: the same again
    acc.push(raw[cut * 4:])
    assert mid == prefix
    assert result(acc) == whole


# ---- 4. determinism, reset, carry ----
def test_two_accumulators_agree_and_reset_equals_fresh(gpu):
    nfft, hop, G = 2048, 1024, psd.geometry()
    raw = stream(frames_for(G + 1, nfft, hop) + 5, "cu8", seed=17)
    other = stream(frames_for(G - 1, nfft, hop) + 999, "cu8", seed=18)
    a, b = gpu.Psd("cu8", nfft=nfft, hop=hop), gpu.Psd("cu8", nfft=nfft, hop=hop)
    for acc in (a, b):
        acc.push(raw[:3001 * 2])
        acc.push(raw[3001 * 2:])
    assert result(a) == result(b)
    b.reset()
    s, k, info = b.read()
    assert not s.any() and not k.any() and info["frames"] == 0 and info["segments"] == 0
    b.push(other)
    assert result(b) == result(one_call(gpu, other, "cu8", nfft, hop))
    assert result(b) != result(a)


@pytest.mark.parametrize("nfft,hop", [(1024, 512), (2048, 512), (4096, 4096)])
def test_short_streams_and_the_carry(gpu, nfft, hop):
    raw = stream(nfft + 1, "cs16", seed=19)
    acc = gpu.Psd("cs16", nfft=nfft, hop=hop)
    acc.push(raw[:0])                       # no frames: nothing changes
    acc.push(raw[:(nfft - 1) * 4])
    s, k, info = acc.read()
    assert info["frames"] == nfft - 1 and info["segments"] == 0 and not s.any() and not k.any()
    acc.push(raw[(nfft - 1) * 4:nfft * 4])  # the one frame the first segment was waiting for
    got = result(acc)
    want = result(one_call(gpu, raw[:nfft * 4], "cs16", nfft, hop))
    assert got == want and got[2]["segments"] == 1
    s, k, _ = acc.read()
    assert s.any() and np.array_equal(s.astype(np.float32), k)     # one segment: the sum is the peak
    acc.push(raw[nfft * 4:])                # nfft + 1 frames: still one segment (hop > 1)
    after = result(acc)
    assert after[:2] == got[:2] and after[2]["frames"] == nfft + 1 and after[2]["segments"] == 1


@pytest.mark.parametrize("segs", ["G - 1", "G", "G + 1", "2 G + 3"])
def test_page_boundaries_against_float64(gpu, oracle, segs):
    nfft, hop = 1024, 256
    n = frames_for(page_segments(segs), nfft, hop)
    raw = stream(n, "cs16", seed=23)
    got_sum, got_peak, info = one_call(gpu, raw, "cs16", nfft, hop).read()
    want_sum, want_peak = reference(oracle, raw, "cs16", nfft, hop, "hann")
    assert info["segments"] == page_segments(segs)
    assert (np.abs(got_sum - want_sum) <= A_BAR * want_sum + B_BAR * want_sum.max()).all()
    assert (np.abs(got_peak - want_peak) <= A_BAR * want_peak + B_BAR * want_peak.max()).all()


# ---- 5. stray reads ----
@pytest.mark.parametrize("nfft,hop", [(1024, 256), (4096, 2048)])
def test_nothing_outside_the_pushed_frames_is_read(gpu, nfft, hop):
    G, guard = psd.geometry(), 4096
    n = frames_for(G + 2, nfft, hop) + hop // 2
    x = synth.complex_signal(n, RATE, 29)
    buf = np.full(n + 2 * guard, np.nan + 1j * np.nan, np.complex64)
    buf[guard:guard + n] = x
    d = gpu.DeviceBuffer(buf.nbytes)
    d.upload(buf)
    acc = gpu.Psd("cf32", nfft=nfft, hop=hop)
    half = n // 2 + 3
    acc.push_device(d.ptr + guard * 8, half)
    acc.push_device(d.ptr + (guard + half) * 8, n - half)
    s, k, info = acc.read()
    assert np.isfinite(s).all() and np.isfinite(k).all() and info["segments"] == G + 2
    assert (s.tobytes(), k.tobytes(), info) == result(one_call(gpu, x, "cf32", nfft, hop))


# ---- 6. with a chain ----
def test_on_a_chains_stream(gpu):
    kw = dict(in_format="cs16", out_format="cs16", input_rate_hz=RATE, target_rate_hz=744187.5, shift_hz=200e3)
    n = 1 << 18
    raw = synth.raw_stream(n, RATE, 31, "cs16")
    plain = gpu.Chain(**kw).process(raw)                     # no accumulator in play
    ch = gpu.Chain(**kw)
    cap = (ch.next_out_frames(n) + 1) * 4
    d_in, d_out = gpu.DeviceBuffer(raw.nbytes), gpu.DeviceBuffer(cap)
    d_in.upload(raw)
    acc_in, acc_out = gpu.Psd("cs16"), gpu.Psd("cs16")
    acc_in.push_device(d_in.ptr, n, ch.get_stream())
    got = ch.process_device(d_in.ptr, n, d_out.ptr, cap)
    acc_out.push_device(d_out.ptr, got, ch.get_stream())
    out_result, in_result = result(acc_out), result(acc_in)
    ch.synchronize()
    out = d_out.download(got * 4, np.int16)
    assert np.array_equal(out, plain)
    assert out_result == result(one_call(gpu, plain, "cs16", 1024, 512)) and out_result[2]["frames"] == got
    assert in_result == result(one_call(gpu, raw, "cs16", 1024, 512)) and in_result[2]["frames"] == n


# ---- 7. the harness ----
ARGS = ["--raw-file-input-rate", "2.4e6", "--raw-file-input-sample-format", "cs16", "--output-rate", "744187.5",
        "--output-sample-format", "cs16", "--freq-shift", "200e3"]


def test_harness_psd(gpu, tmp_path):
    n = 1 << 18
    raw = synth.raw_stream(n, RATE, 37, "cs16")
    fin, fout, prefix = tmp_path / "in.cs16", tmp_path / "out.cs16", tmp_path / "spec"
    raw.tofile(fin)
    r = subprocess.run([EXE, "-i", str(fin), "-o", str(fout), *ARGS, "--chunk-frames", "50000", "--psd", str(prefix)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    out = np.fromfile(fout, np.int16)
    meta = json.loads(open(str(prefix) + ".json").read())
    for side, data, rate in (("in", raw, 2.4e6), ("out", out, 744187.5)):
        want_sum, _, info = one_call(gpu, data, "cs16", 1024, 512).read()
        got = np.fromfile(str(prefix) + "." + side + ".f64", "<f8")
        assert got.size == 1024 and got.tobytes() == want_sum.tobytes(), side
        m = meta[side]
        assert m["rate_hz"] == rate and {k: m[k] for k in info} == info
        assert m["window"] == "hann" and m["file"] == str(prefix) + "." + side + ".f64"


def test_harness_psd_excludes_shards(gpu, tmp_path):
    base = ["--synthetic", "100000", "--synthetic-hash", "3", *ARGS, "--psd", str(tmp_path / "spec")]
    for extra in (["--shards", "2"], ["--shards", "2", "--seamless"], ["--iq-calibrate"]):
        r = subprocess.run([EXE, *base, *extra], capture_output=True, text=True)
        assert r.returncode == 2 and "usage" in r.stderr and "--psd" in r.stderr, (extra, r.returncode, r.stderr)
    assert not list(tmp_path.iterdir())


if __name__ == "__main__":
    from oracle import pyoracle
    pyoracle.build()
    rows = measure_f32_error(pyoracle)
    for a, b, what in rows:
        print("a = %.3g  b = %.3g  %s" % (a, b, what))
    wa, wb = max(rows, key=lambda r: r[0]), max(rows, key=lambda r: r[1])
    print("worst a = %.3g (%s)\nworst b = %.3g (%s)\nbars: A = %.3g, B = %.3g" % (wa[0], wa[2], wb[1], wb[2], 8 * wa[0], 8 * wb[1]))
