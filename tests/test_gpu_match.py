"""The template-correlation accumulator on the device (include/iqgpu.h "template correlation"; k_match_segs / k_match_fold)
against the float64 model of tests/match_model.py.

1. Against float64.  `want` is the model: frames unpacked by the oracle's conversion, correlation and powers in float64, the row rules.
   Bars, per (row, template): |row_peak - want| <= PEAK_BAR want and |row_sum - want| <= SUM_BAR want, each 8 x the worst relative error
   of the SAME overlap-save in float32 on the CPU (match_model.f32_overlap_save: scipy.fft on complex64, G rounded to float32, powers
   in float32, sums in double) against the model over the cases of this test, measured by `measure_f32_error` below
   (`PYTHONPATH=.:tests python tests/test_gpu_match.py` prints it):
       measured  row_peak 4.50e-07 (cs16, 2048, L 1025, 1 template, B 2 V)   row_sum 1.48e-07 (cs8, 1024, L 16, 1 template, B 2 V)
       bars      PEAK_BAR 3.60e-06                                          SUM_BAR 1.18e-06
   Measured on an MI355X, worst over the cases: row_peak 6.90e-07 (cs16, 4096, L 16), row_sum 3.03e-07 (cu8, 1024, L 513; it includes
   the one rounding of the row to float, which the figure measured on the CPU does not).
   The margin of 8 is there because a radix-16 transform with another operation order and twiddles that are products of rounded table
   values may differ from scipy's by a small factor.
   row_at must EQUAL the model's wherever the model's best value of the row exceeds its runner-up by more than 1e-4 relative; the rows
   left out for a thinner margin may be at most 2 % of a case's rows, and a row with a planted copy is never left out.
   Copies are planted at n = 0, V - 1 and V, r B - 1 and r B, the last reported start position, and one behind the last whole segment --
   which no row and no open row may report.
2. Bit for bit: any split of the stream into pushes, host or device, gives the same bytes; reset equals a fresh handle; read_open
   observes; max_rows is what a push returns; a capacity one short is refused with the handle unchanged; a device push of more
   segments than one launch takes (2^15) equals the host push, which goes slice by slice.
3. The tie rule on an all-zero stream.   4. Guard frames of NaN.   5. The shift bank, end to end.   6. On a chain's stream.
7. The harness's --match: the row files equal the Python rows, the JSON detections name the planted frames; its refusals.
Shapes: V = nfft / 2; rows of 1 segment (B = V), 2, 32 and 64 segments; streams of 2 rows and a few segments (under 70 k frames at nfft
1024); nfft 2048 and 4096 once each."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import match_model
from env_model import BPF
from iq_tool_amd import match, synth

pytestmark = pytest.mark.gpu
RATE = 2.4e6
PEAK_BAR, SUM_BAR = 8 * 4.50e-07, 8 * 1.48e-07
MARGIN = 1e-4
# test 1: (format, nfft, L, templates, B / V)
CASES = ([("cs16", 1024, 16, 2, 2), ("cu8", 1024, 513, 1, 1), ("cf32", 1024, 512, 2, 32), ("cs16", 1024, 2, 8, 64)]
         + [(f, 1024, 16, 1, 2) for f in ("cs8", "cu16", "sc16q11", "cs24", "cu32", "cs32")]
         + [("cs16", 2048, 1025, 1, 2), ("cs16", 4096, 16, 2, 1)])

_cases = {}


def case_of(fmt, nfft, L, nt, mult):
    """(raw bytes, templates, B, segments, {planted position: (template, amplitude)}) of a case: two rows and a few segments, a ragged tail"""
    key = (fmt, nfft, L, nt, mult)
    if key not in _cases:
        V = nfft // 2
        B, segs = mult * V, (41 if mult <= 2 else 2 * mult + 5)
        n = nfft + (segs - 1) * V + 37
        tmpl = match_model.templates(nt, L, nfft + L)
        last = segs * V - 1
        at = [0, V - 1, V, B - 1, B, 2 * B - 1, 2 * B, last, last + 1]
        places = {a: (i % nt, (0.25, 0.2)[i % 2]) for i, a in enumerate(at)}
        raw = match_model.planted(n, fmt, tmpl, [(a, t, amp) for a, (t, amp) in sorted(places.items())], seed=nfft + mult)
        raw.setflags(write=False)
        _cases[key] = (raw, tmpl, B, segs, places)
    return _cases[key]


_models = {}


def model_of(oracle, key):
    if key not in _models:
        raw, tmpl, B, _, _ = case_of(*key)
        _models[key] = match_model.model(raw, key[0], tmpl, B, oracle, key[1])
    return _models[key]


def result(parts, acc):
    """what the pushes returned, concatenated, and the open row, as bytes"""
    o = acc.read_open()
    return (b"".join(p[0].tobytes() for p in parts), b"".join(p[1].tobytes() for p in parts), b"".join(p[2].tobytes() for p in parts),
            (o[0].tobytes(), o[1].tobytes(), o[2].tobytes()), o[3])


def push_split(gpu, raw, fmt, tmpl, B, nfft=0, cuts=(), device=(), offset=0, acc=None):
    """the stream pushed in pieces cut at `cuts` (frames); pieces whose index is in `device` go through push_device at a pointer
    `offset` bytes into its buffer"""
    raw = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
    bpf, n = BPF[fmt], raw.size // BPF[fmt]
    acc = acc or gpu.Match(fmt, tmpl, B, nfft)
    nt, parts, keep = acc.n_templates, [], []
    edges = [0] + list(cuts) + [n]
    for i, (lo, hi) in enumerate(zip(edges[:-1], edges[1:])):
        if hi <= lo:
            continue
        piece = raw[lo * bpf:hi * bpf]
        cap = acc.max_rows(hi - lo)
        if i in device:
            plane = 4 * nt * cap
            d_in, d_rows = gpu.DeviceBuffer(piece.size + offset + 64), gpu.DeviceBuffer(3 * plane + 64)
            buf = np.full(piece.size + offset, 0xA5, np.uint8)
            buf[offset:] = piece
            d_in.upload(buf)
            assert acc.push_device(d_in.ptr + offset, hi - lo, d_rows.ptr, d_rows.ptr + plane, d_rows.ptr + 2 * plane, cap) == cap
            acc.read_open()                                    # (synchronises)
            out = d_rows.download(3 * plane, np.uint8) if cap else np.zeros(0, np.uint8)
            parts.append((out[:plane], out[plane:2 * plane], out[2 * plane:]))
            keep += [d_in, d_rows]
        else:
            parts.append(acc.push(piece))
    return result(parts, acc)


def arrays(got, nt):
    return (np.frombuffer(got[0], np.float32).reshape(-1, nt), np.frombuffer(got[1], np.uint32).reshape(-1, nt),
            np.frombuffer(got[2], np.float32).reshape(-1, nt))


def rel_err(got, want):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(want > 0, np.abs(got.astype(np.float64) - want) / want, np.abs(got.astype(np.float64)))


def measure_f32_error(oracle):
    """the float32 overlap-save against the float64 model on the inputs of test 1, on the CPU: [(peak error, sum error, what)]"""
    rows = []
    for key in CASES:
        raw, tmpl, B, _, _ = case_of(*key)
        (peak, _, total, _), _, _ = model_of(oracle, key)
        p32, _, s32 = match_model.f32_overlap_save(raw, key[0], tmpl, B, oracle, key[1])
        rows.append((float(rel_err(p32, peak).max()), float(rel_err(s32, total).max()), "%s, %d, L %d, %d templates, B %d V" % key))
    return rows


# ---- 1. against float64 ----
@pytest.mark.parametrize("key", CASES, ids=lambda k: "-".join(str(v) for v in k))
def test_rows_against_the_float64_model(gpu, oracle, key):
    fmt, nfft, L, nt, mult = key
    raw, tmpl, B, segs, places = case_of(*key)
    V = nfft // 2
    (peak, at, total, margin), (o_sum, o_peak, o_at), info = model_of(oracle, key)
    got = push_split(gpu, raw, fmt, tmpl, B, nfft)
    g_peak, g_at, g_sum = arrays(got, nt)
    want_info = dict(info)
    energy, got_energy = want_info.pop("template_energy"), got[4].pop("template_energy")
    assert got[4] == want_info and np.allclose(got_energy, energy, rtol=1e-12, atol=0)
    assert g_peak.shape == peak.shape and info["rows"] == segs // mult >= 2 and (mult == 1 or info["open_segments"] > 0)
    e_peak, e_sum = rel_err(g_peak, peak), rel_err(g_sum, total)
    print("%s: row_peak error %.3g (bar %.3g), row_sum error %.3g (bar %.3g)" % (key, e_peak.max(), PEAK_BAR, e_sum.max(), SUM_BAR))
    assert e_peak.max() <= PEAK_BAR and e_sum.max() <= SUM_BAR
    # the positions: every row with a clear winner, the rows of the planted copies among them
    clear = margin > MARGIN
    assert (g_at[clear] == at[clear]).all(), np.argwhere(clear & (g_at != at))[:8]
    assert (~clear).sum() <= 0.02 * clear.size
    reported = [a for a in places if a < info["rows"] * B]
    for a in reported:
        assert clear[a // B, places[a][0]], ("a row with a planted copy has no clear winner in the model", a)
    # the last reported start position holds a copy and wins its row or the open row; the copy one behind it is nowhere
    last = segs * V - 1
    assert last in places and last + 1 in places and info["rows"] * B + info["open_segments"] * V == last + 1
    t_last = places[last][0]
    g_open = (np.frombuffer(got[3][0], np.float64), np.frombuffer(got[3][1], np.float32), np.frombuffer(got[3][2], np.uint32))
    if info["open_segments"]:
        assert g_open[2][t_last] == o_at[t_last] == last - info["rows"] * B
        assert rel_err(g_open[1], o_peak).max() <= PEAK_BAR and rel_err(g_open[0], o_sum).max() <= SUM_BAR
    else:
        assert g_at[-1][t_last] == at[-1][t_last] == last - (info["rows"] - 1) * B and not np.frombuffer(got[3][0], np.uint8).any()
    assert g_at.max(initial=0) < B and (g_open[2] < max(1, info["open_segments"]) * V).all()


# ---- 2. bit for bit ----
SPLIT = ("cs16", 1024, 16, 2, 2)


def test_any_split_gives_the_same_bytes(gpu):
    raw, tmpl, B, segs, _ = case_of(*SPLIT)
    n = raw.size // 4
    whole = push_split(gpu, raw, "cs16", tmpl, B, 1024)
    assert whole[4]["rows"] == segs // 2 and len(whole[0]) == 4 * 2 * (segs // 2)
    pieces, at = [], 0
    for step in (1, 63, 511, 513, 1023, 1025, 1537, 3000, 7001):
        at += step
        pieces.append(at)
    for name, cuts in {"pieces": pieces, "on the grid": [512, 1024, 1536, 4096]}.items():
        assert push_split(gpu, raw, "cs16", tmpl, B, 1024, cuts) == whole, name
        # host and device alternating, the device pointer one frame off any wider alignment
        assert push_split(gpu, raw, "cs16", tmpl, B, 1024, cuts, device=range(0, 99, 2), offset=4) == whole, name
        assert push_split(gpu, raw, "cs16", tmpl, B, 1024, cuts, device=range(1, 99, 2), offset=0) == whole, name


def test_single_frame_pushes(gpu):
    raw, tmpl, B, _, _ = case_of(*SPLIT)
    n = 1024 + 3 * 512 + 5                                      # two rows of two segments and a tail
    short = raw[:4 * n]
    whole = push_split(gpu, short, "cs16", tmpl, B, 1024)
    assert whole[4]["rows"] == 2 and whole[4]["open_segments"] == 0
    assert push_split(gpu, short, "cs16", tmpl, B, 1024, cuts=range(1, n)) == whole
    one_more = push_split(gpu, raw[:4 * (n + 512)], "cs16", tmpl, B, 1024, cuts=range(1, n + 512, 7))
    assert one_more[4]["open_segments"] == 1 and one_more[:3] == whole[:3] and np.frombuffer(one_more[3][0], np.float64).all()


@pytest.mark.parametrize("key", [("cf32", 1024, 512, 2, 32), ("cs16", 1024, 2, 8, 64), ("cs24", 1024, 16, 1, 2), ("cu8", 1024, 513, 1, 1), ("cs16", 4096, 16, 2, 1)],
                         ids=lambda k: "-".join(str(v) for v in k))
def test_a_row_that_opens_in_one_push_and_closes_in_another(gpu, key):
    fmt, nfft, L, nt, mult = key
    raw, tmpl, B, segs, _ = case_of(*key)
    n = raw.size // BPF[fmt]
    whole = push_split(gpu, raw, fmt, tmpl, B, nfft)
    cuts = sorted({nfft // 2 + 3, B // 2 + 7, B + 1, B + nfft + 11, 2 * B - 1})
    assert cuts[-1] < n
    assert push_split(gpu, raw, fmt, tmpl, B, nfft, cuts) == whole
    assert push_split(gpu, raw, fmt, tmpl, B, nfft, cuts, device=(1, 2, 4), offset=2 if fmt == "cs24" else BPF[fmt]) == whole      # (cu8: 2 bytes off)


def test_a_device_push_cut_into_two_launches(gpu):
    """one push_device of more segments than the slab holds (2^15: match.hpp) is cut into two launches; behind a first push of two
    segments the second launch starts inside a row.  A host push of the same bytes goes slice by slice, every launch below the bound.
    The same bytes both ways."""
    nfft, B, slab, pre = 1024, 2048, 1 << 15, 1024 + 512
    n = nfft + (slab + 4) * 512 + 9                             # slab + 5 segments: launches over segments [2, slab + 2) and [slab + 2, slab + 5)
    raw = synth.hash_stream(n, 7, "cu8")
    tmpl = match_model.templates(2, 2, 13)
    d_in = gpu.DeviceBuffer(raw.nbytes)
    d_in.upload(raw)
    acc = gpu.Match("cu8", tmpl, B, nfft)
    assert acc.push(raw[:2 * pre])[0].shape == (0, 2) and acc.read_open()[3]["open_segments"] == 2
    rows = acc.max_rows(n - pre)
    assert rows == (slab + 5) // 4
    d_rows = gpu.DeviceBuffer(24 * rows)
    assert acc.push_device(d_in.ptr + 2 * pre, n - pre, d_rows.ptr, d_rows.ptr + 8 * rows, d_rows.ptr + 16 * rows, rows) == rows
    o = acc.read_open()
    out = d_rows.download(24 * rows, np.uint8)
    want = push_split(gpu, raw, "cu8", tmpl, B, nfft)
    assert (out[:8 * rows].tobytes(), out[8 * rows:16 * rows].tobytes(), out[16 * rows:].tobytes()) == want[:3]
    assert (o[0].tobytes(), o[1].tobytes(), o[2].tobytes()) == want[3] and o[3] == want[4] and o[3]["open_segments"] == 1


def test_reset_read_open_max_rows_and_capacity(gpu):
    raw, tmpl, B, segs, _ = case_of(*SPLIT)
    n, rows = raw.size // 4, segs // 2
    whole = push_split(gpu, raw, "cs16", tmpl, B, 1024)
    acc = gpu.Match("cs16", tmpl, B, 1024)
    lib = acc._lib
    acc.push(synth.raw_stream(5000, RATE, 3, "cs16"))
    acc.reset()
    assert acc.read_open()[3]["frames"] == 0 and not acc.read_open()[0].any()
    assert push_split(gpu, raw, "cs16", tmpl, B, 1024, acc=acc) == whole          # reset equals a fresh handle
    a, b = acc.read_open(), acc.read_open()                                        # observes, does not disturb
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3] == whole[4]
    acc.reset()
    assert acc.max_rows(n) == rows and acc.max_rows(1024 + 511) == 0 and acc.max_rows(1024 + 512) == 1
    # a capacity one short: refused before anything is queued, the handle as it was
    pk, got = np.full(2 * rows, 7, np.uint32), C.c_size_t(9)
    rc = lib.iqgpu_match_push(acc._h, raw.ctypes.data_as(C.c_void_p), n, pk.ctypes.data_as(C.c_void_p), None, None, rows - 1, C.byref(got))
    assert rc == -8 and got.value == 0 and (pk == 7).all() and acc.read_open()[3]["frames"] == 0
    d_in, d_rows = gpu.DeviceBuffer(raw.size), gpu.DeviceBuffer(8 * rows)
    d_in.upload(raw)
    got.value = 9
    rc = lib.iqgpu_match_push_device(acc._h, C.c_void_p(d_in.ptr), n, None, C.c_void_p(d_rows.ptr), None, rows - 1, C.byref(got), None)
    assert rc == -8 and got.value == 0 and acc.read_open()[3]["frames"] == 0
    # one plane alone: the others are not produced, the stream goes on all the same; no plane: no capacity asked
    assert acc.push_device(d_in.ptr, n, 0, d_rows.ptr, 0, rows) == rows
    assert acc.read_open()[3] == whole[4] and d_rows.download(8 * rows, np.uint8).tobytes() == whole[1]
    acc.reset()
    assert lib.iqgpu_match_push(acc._h, raw.ctypes.data_as(C.c_void_p), n, None, None, None, 0, C.byref(got)) == 0 and got.value == rows
    o = acc.read_open()
    assert (o[0].tobytes(), o[1].tobytes(), o[2].tobytes()) == whole[3]
    assert lib.iqgpu_match_push(acc._h, None, 0, None, None, None, 0, C.byref(got)) == 0 and got.value == 0      # frames == 0 changes nothing
    assert acc.read_open()[3] == whole[4]


# ---- 3. the tie rule ----
@pytest.mark.parametrize("nfft,mult", [(1024, 1), (1024, 2), (4096, 2)])
def test_an_all_zero_stream_reports_position_zero(gpu, nfft, mult):
    V = nfft // 2
    tmpl = match_model.templates(2, 16, 9)
    raw = np.zeros(2 * (nfft + (4 * mult) * V + 5), np.int16)
    with gpu.Match("cs16", tmpl, mult * V, nfft) as acc:
        pk, at, sm = acc.push(raw)
        o = acc.read_open()
    assert pk.shape == (4 + (mult == 1), 2) and o[3]["open_segments"] == (1 if mult > 1 else 0)      # 4 mult + 1 segments
    assert not pk.any() and not at.any() and not sm.any() and not o[0].any() and not o[1].any() and not o[2].any()


# ---- 4. stray reads ----
@pytest.mark.parametrize("nfft", (1024, 4096))
def test_nothing_outside_the_pushed_frames_is_read(gpu, nfft):
    V, guard = nfft // 2, 4096
    n = nfft + 6 * V + V // 2
    tmpl = match_model.templates(2, 16, 11)
    x = synth.complex_signal(n, RATE, 29)
    buf = np.full(n + 2 * guard, np.nan + 1j * np.nan, np.complex64)
    buf[guard:guard + n] = x
    d = gpu.DeviceBuffer(buf.nbytes)
    d.upload(buf)
    acc = gpu.Match("cf32", tmpl, 2 * V, nfft)
    rows = acc.max_rows(n)
    d_rows = gpu.DeviceBuffer(3 * 8 * rows)
    half = n // 2 + 3
    r0 = acc.push_device(d.ptr + guard * 8, half, d_rows.ptr, d_rows.ptr + 8 * rows, d_rows.ptr + 16 * rows, rows)
    r1 = acc.push_device(d.ptr + (guard + half) * 8, n - half, d_rows.ptr + 8 * r0, d_rows.ptr + 8 * (rows + r0), d_rows.ptr + 8 * (2 * rows + r0), rows - r0)
    o = acc.read_open()
    out = d_rows.download(24 * rows, np.uint8)
    assert r0 + r1 == rows == 3 and o[3]["open_segments"] == 1
    assert np.isfinite(out.view(np.float32)[:2 * rows]).all() and np.isfinite(out.view(np.float32)[4 * rows:]).all() and np.isfinite(o[0]).all()
    want = push_split(gpu, x, "cf32", tmpl, 2 * V, nfft)
    assert (out[:8 * rows].tobytes(), out[8 * rows:16 * rows].tobytes(), out[16 * rows:].tobytes()) == want[:3]
    assert (o[0].tobytes(), o[1].tobytes(), o[2].tobytes()) == want[3]


# ---- 5. the bank, end to end ----
def test_the_shift_bank_finds_the_offset_and_the_frame(gpu):
    L, B, n, frame = 512, 4096, 5 * 4096 + 1024, 2 * 4096 + 1234
    hz = [-15e3, -5e3, 5e3, 15e3, 25e3]
    tmpl = match_model.templates(1, L, 17)[0]
    bank = match.shift_bank(tmpl, hz, RATE)
    rng = np.random.default_rng(41)
    z = 0.02 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    z[frame:frame + L] += 0.25 * tmpl.astype(np.complex128) * np.exp(2j * np.pi * hz[2] * np.arange(L) / RATE)     # received hz[2] off centre
    raw = synth.quantise(z.astype(np.complex64), "cs16")
    with gpu.Match("cs16", bank, B) as acc:
        assert acc.nfft == 1024
        pk, at, sm = acc.push(raw)
    found = match.peaks(pk, at, sm, B, L, 100.0)
    best = max(found, key=lambda d: d["ratio"])
    assert best["template"] == 2 and best["first_frame"] == frame, found
    every = [d for d in match.peaks(pk, at, sm, B, L, 0.0) if d["first_frame"] // B == frame // B]
    assert len(every) == 5 and all(d["ratio"] < best["ratio"] for d in every if d["template"] != 2)
    assert all(d["first_frame"] // B == frame // B for d in found), found           # nothing in the noise rows


# ---- 6. behind a chain on its stream ----
def test_behind_a_chain_on_its_stream(gpu):
    kw = dict(in_format="cs16", out_format="cs8", input_rate_hz=RATE, target_rate_hz=744187.5, shift_hz=200e3, gain=40.0)
    n, B = 1 << 17, 2048
    tmpl = match_model.templates(2, 64, 23)
    raw = synth.raw_stream(n, RATE, 31, "cs16")
    plain = gpu.Chain(**kw).process(raw)
    ch = gpu.Chain(**kw)
    cap = (ch.next_out_frames(n) + 1) * 2
    d_in, d_out = gpu.DeviceBuffer(raw.nbytes), gpu.DeviceBuffer(cap)
    d_in.upload(raw)
    got = ch.process_device(d_in.ptr, n, d_out.ptr, cap)
    acc = gpu.Match("cs8", tmpl, B)
    rows = acc.max_rows(got)
    d_rows = gpu.DeviceBuffer(24 * rows)
    assert acc.push_device(d_out.ptr, got, d_rows.ptr, d_rows.ptr + 8 * rows, d_rows.ptr + 16 * rows, rows, ch.get_stream()) == rows
    o = acc.read_open()
    ch.synchronize()
    out = d_rows.download(24 * rows, np.uint8)
    want = push_split(gpu, plain, "cs8", tmpl, B)
    assert (out[:8 * rows].tobytes(), out[8 * rows:16 * rows].tobytes(), out[16 * rows:].tobytes()) == want[:3] and rows > 4
    assert (o[0].tobytes(), o[1].tobytes(), o[2].tobytes()) == want[3] and o[3] == want[4]


# ---- 7. the harness ----
EXE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "iq_tool_amd", "lib", "iqgpu_run")
ARGS = ["--raw-file-input-rate", "2.4e6", "--raw-file-input-sample-format", "cs16", "--output-rate", "744187.5",
        "--output-sample-format", "cs16"]


def harness_input(tmp_path, hz=0.0):
    """a cs16 file of noise with the template planted at two frames (received hz off centre), the template file, the frames"""
    L, n, frames = 64, 40 * 1024 + 77, (3 * 1024 + 5, 20 * 1024 + 1023)
    tmpl = match_model.templates(1, L, 31)[0]
    rng = np.random.default_rng(43)
    z = 0.02 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for at in frames:
        z[at:at + L] += 0.25 * tmpl.astype(np.complex128) * np.exp(2j * np.pi * hz * np.arange(L) / RATE)
    raw = synth.quantise(z.astype(np.complex64), "cs16")
    raw.tofile(tmp_path / "in.cs16")
    tmpl.tofile(tmp_path / "tmpl.cf32")
    return raw, tmpl, frames


@pytest.mark.parametrize("shifts", (None, (-40e3, 0.0, 40e3)))
def test_harness_match_files_and_json(gpu, tmp_path, shifts):
    B = 1024
    raw, tmpl, frames = harness_input(tmp_path, hz=shifts[2] if shifts else 0.0)
    fout, prefix = tmp_path / "out.cs16", tmp_path / "m"
    extra = ["--match-shifts", ",".join("%r" % h for h in shifts)] if shifts else []
    r = subprocess.run([EXE, "-i", str(tmp_path / "in.cs16"), "-o", str(fout), *ARGS, "--chunk-frames", "5000", "--match", str(prefix),
                        "--match-template", str(tmp_path / "tmpl.cf32"), "--match-block", str(B), *extra], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    out = np.fromfile(fout, np.int16)
    meta = json.loads(open(str(prefix) + ".json").read())
    nt = len(shifts) if shifts else 1
    assert (meta["nfft"], meta["block_frames"], meta["n_templates"], meta["template_frames"], meta["ratio"]) == (1024, B, nt, 64, 100.0)
    assert meta["shifts_hz"] == (list(shifts) if shifts else [])
    for side, data, rate in (("in", raw, 2.4e6), ("out", out, 744187.5)):
        bank = match.shift_bank(tmpl, shifts, rate) if shifts else tmpl
        got = push_split(gpu, data, "cs16", bank, B)
        for i, plane in enumerate(("peak.f32", "at.u32", "sum.f32")):
            assert open("%s.%s.%s" % (prefix, side, plane), "rb").read() == got[i], (side, plane)
        m, info = meta[side], got[4]
        assert (m["sample_rate"], m["frames"], m["segments"], m["rows"], m["open_segments"]) == (rate, info["frames"], info["segments"], info["rows"],
                                                                                                 info["open_segments"])
        assert m["template_energy"] == info["template_energy"] and m["files"] == ["%s.%s.%s" % (prefix, side, p) for p in ("peak.f32", "at.u32", "sum.f32")]
        want = match.peaks(*arrays(got, nt), B, 64, 100.0)
        assert [(d["first_frame"], d["template"]) for d in m["detections"]] == [(d["first_frame"], d["template"]) for d in want]
        assert [d["ratio"] for d in m["detections"]] == [d["ratio"] for d in want]          # == on the parsed doubles
    assert meta["in"]["rows"] == 39 and meta["out"]["rows"] > 8
    # the detections of the input name the planted frames, with the member the burst was shifted by
    best = {}
    for d in meta["in"]["detections"]:
        if d["first_frame"] // B not in best or d["ratio"] > best[d["first_frame"] // B]["ratio"]:
            best[d["first_frame"] // B] = d
    assert sorted((d["first_frame"], d["template"]) for d in best.values()) == [(f, 2 if shifts else 0) for f in frames]


def test_harness_match_refusals(gpu, tmp_path):
    files = tmp_path / "files"
    files.mkdir()
    harness_input(files)
    np.zeros(3, np.float32).tofile(files / "ragged.cf32")
    np.zeros(2 * 2050, np.float32).tofile(files / "long.cf32")
    np.ones(2 * 600, np.float32).tofile(files / "l600.cf32")
    where = tmp_path / "w"
    where.mkdir()
    tm = ["--match-template", str(files / "tmpl.cf32")]
    base = ["--synthetic", "100000", "--synthetic-hash", "3", *ARGS, "--match", str(where / "m")]
    for extra in (["--shards", "2"], ["--shards", "2", "--seamless"], ["--iq-calibrate"]):
        r = subprocess.run([EXE, *base, *tm, *extra], capture_output=True, text=True)
        assert r.returncode == 2 and "usage" in r.stderr and "--match" in r.stderr, (extra, r.returncode, r.stderr)
    r = subprocess.run([EXE, *base], capture_output=True, text=True)                       # no template
    assert r.returncode == 2 and "--match-template" in r.stderr
    for name in ("ragged.cf32", "long.cf32", "absent.cf32"):
        r = subprocess.run([EXE, *base, "--match-template", str(files / name)], capture_output=True, text=True)
        assert r.returncode == 2 and "--match-template" in r.stderr, (name, r.stderr)
    for block in ("100", "256", "1000", "33554432"):
        r = subprocess.run([EXE, *base, *tm, "--match-block", block], capture_output=True, text=True)
        assert r.returncode == 2 and "--match-block" in r.stderr, (block, r.stderr)
    r = subprocess.run([EXE, *base, "--match-template", str(files / "l600.cf32"), "--match-block", "512"], capture_output=True, text=True)
    assert r.returncode == 2 and "--match-block" in r.stderr, r.stderr                     # L = 600 runs at nfft 2048: B >= 1024
    for lst in ("", "1,x", "nan", "1,2,3,4,5,6,7,8,9", "5,"):
        r = subprocess.run([EXE, *base, *tm, "--match-shifts", lst], capture_output=True, text=True)
        assert r.returncode == 2 and "--match-shifts" in r.stderr, (lst, r.stderr)
    for alone in (["--match-block", "1024"], ["--match-shifts", "1,2"], tm):
        r = subprocess.run([EXE, "--synthetic", "100000", "--synthetic-hash", "3", *ARGS, *alone], capture_output=True, text=True)
        assert r.returncode == 2 and alone[0] in r.stderr, (alone, r.stderr)
    assert not list(where.iterdir())


if __name__ == "__main__":
    from oracle import pyoracle
    pyoracle.build()
    figures = measure_f32_error(pyoracle)
    for a, b, what in figures:
        print("row_peak %.3g  row_sum %.3g  %s" % (a, b, what))
    wa, wb = max(figures, key=lambda r: r[0]), max(figures, key=lambda r: r[1])
    print("worst row_peak %.3g (%s)\nworst row_sum %.3g (%s)\nbars: PEAK_BAR %.3g, SUM_BAR %.3g" % (wa[0], wa[2], wb[1], wb[2], 8 * wa[0], 8 * wb[1]))
    for key in CASES:
        margin = model_of(pyoracle, key)[0][3]
        print("%s: %d of %d (row, template) without a clear winner" % (key, (margin <= MARGIN).sum(), margin.size))
