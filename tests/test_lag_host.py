"""The parts of the lag-product accumulator that need no device (include/iqgpu.h "lag products"): the row arithmetic and every refusal
of the options, the struct layouts, the float64 model of lag_model.py against a naive float64 sum and against env_model's row_sum, the
two host helpers against the model's restatement, and the physical sense of the whole on noise-free tones."""
import ctypes as C
import math

import numpy as np
import pytest

import env_model
import lag_model
from iq_tool_amd import _lib, lag

FS = 2.4e6


def rc_of(fn, *args):
    return getattr(_lib.load(), fn)(*args)


def opts(b, lags):
    o = _lib.LagOpts(b, len(lags))
    for i, d in enumerate(lags[:4]):
        o.lags[i] = d
    return o


class _FakeOracle:
    """cf32 only: the unpack at gain 1 is the identity"""
    @staticmethod
    def to_cf32(raw, fmt, gain):
        assert fmt == "cf32" and gain == 1.0
        return np.ascontiguousarray(raw).view(np.complex64).copy()


def test_defaults_and_rows_arithmetic():
    o = lag.lag_opts()
    assert (o.block_frames, o.n_lags, list(o.lags)) == (4096, 1, [1, 0, 0, 0])
    for b in (64, 1024, 4096, 1 << 24):
        for frames in (0, 1, b - 1, b, b + 1, 5 * b + 17, (1 << 40) + 3):
            assert lag.rows(frames, b, (1, 65536)) == frames // b
    assert rc_of("iqgpu_lag_max_rows", None, 1000) == 0


BAD_OPTS = [(b, (1,)) for b in (0, 32, 96, 100, 4095, 1 << 25, (1 << 24) + 1)] + \
           [(4096, ()), (4096, (1, 2, 3, 4, 5)), (4096, (0,)), (4096, (65537,)), (4096, (1, 0)), (4096, (3, 3)), (4096, (5, 4)),
            (4096, (1, 2, 2, 9)), (4096, (1, 2, 3, 65537))]


@pytest.mark.parametrize("b,lags", BAD_OPTS)
def test_every_refusal_of_the_options(b, lags):
    o, n, h = opts(b, lags), C.c_uint64(7), C.c_void_p()
    if len(lags) == 5:
        o.n_lags = 5
    assert rc_of("iqgpu_lag_rows", C.byref(o), 1000, C.byref(n)) == -1
    assert rc_of("iqgpu_lag_create", 0, 11, C.byref(o), C.byref(h)) == -1 and not h.value      # refused before any device is looked for
    est, v = _lib.LagEstimate(), np.zeros(16, np.float32)
    assert rc_of("iqgpu_lag_estimate_rows", v.ctypes.data_as(C.c_void_p), None, 1, C.byref(o), 0, 0, 1, 1.0, C.byref(est)) == -1


def test_null_arguments_are_refused():
    o, n, h = opts(64, (1,)), C.c_uint64(0), C.c_void_p()
    assert rc_of("iqgpu_lag_rows", None, 1000, C.byref(n)) == -1
    assert rc_of("iqgpu_lag_rows", C.byref(o), 1000, None) == -1
    assert rc_of("iqgpu_lag_create", 0, 11, None, C.byref(h)) == -1
    assert rc_of("iqgpu_lag_create", 0, 11, C.byref(o), None) == -1
    assert rc_of("iqgpu_lag_reset", None) == -1
    assert rc_of("iqgpu_lag_push", None, None, 0, None, None, 0, None) == -1
    assert rc_of("iqgpu_lag_push_device", None, None, 0, None, None, 0, None, None) == -1
    assert rc_of("iqgpu_lag_read_open", None, None, None, None) == -1
    assert rc_of("iqgpu_lag_freq", 1.0, 0.0, 1, 1.0, None) == -1
    est, v = _lib.LagEstimate(), np.zeros(2, np.float32)
    assert rc_of("iqgpu_lag_estimate_rows", None, None, 1, C.byref(o), 0, 0, 1, 1.0, C.byref(est)) == -1
    assert rc_of("iqgpu_lag_estimate_rows", v.ctypes.data_as(C.c_void_p), None, 1, None, 0, 0, 1, 1.0, C.byref(est)) == -1
    assert rc_of("iqgpu_lag_estimate_rows", v.ctypes.data_as(C.c_void_p), None, 1, C.byref(o), 0, 0, 1, 1.0, None) == -1
    rc_of("iqgpu_lag_destroy", None)                              # a NULL handle is nothing to destroy
    rc_of("iqgpu_lag_opts_init", None)


def test_struct_layouts():
    u32, u64, f64 = C.sizeof(C.c_uint32), C.sizeof(C.c_uint64), C.sizeof(C.c_double)
    assert C.sizeof(_lib.LagOpts) == 6 * u32 and _lib.LagOpts.lags.offset == 8
    assert C.sizeof(_lib.LagInfo) == 3 * u64 + 8 * u32 and _lib.LagInfo.open_frames.offset == 24 and _lib.LagInfo.lags.offset == 36
    assert C.sizeof(_lib.LagEstimate) == 6 * f64 and _lib.LagEstimate.hz.offset == 24
    # the library writes the fields where the mirrors read them
    got = lag.estimate(np.array([[0, 3 + 4j]], np.complex64), np.array([10], np.float32), 64, (1, 4), 1, 8.0)
    assert got == dict(re=3.0, im=4.0, power=10.0, hz=math.atan2(4.0, 3.0) / (2.0 * math.pi * 4) * 8.0, coherence=0.5, span_hz=2.0)


# ---- the model ----
@pytest.mark.parametrize("b", (64, 1024, 4096, 65536, 131072))
def test_the_model_against_a_naive_sum(b):
    """the model and np.sum add the SAME terms (two exact products, one rounding each), so they differ by the order of at most B
    additions alone: |model - naive| <= B * 2^-52 * the sum of the term magnitudes"""
    rng = np.random.default_rng(b)
    n, lags = 2 * b + 17, (1, 5, 1025)
    x = (rng.standard_normal((n, 2)) * 0.3).astype(np.float32)
    comps, ok = lag_model.components(x, "cf32", lags, _FakeOracle)
    z = x.astype(np.float64)[:, 0] + 1j * x.astype(np.float64)[:, 1]
    for l, d in enumerate(lags):
        terms = np.zeros(n, np.complex128)
        terms[d:] = z[d:] * np.conj(z[:-d])
        for r in range(3):
            sl = slice(r * b, min((r + 1) * b, n))
            naive = np.sum(terms[sl])
            got = complex(lag_model.row_value(comps[2 * l][0][sl], comps[2 * l][1][sl], b), lag_model.row_value(comps[2 * l + 1][0][sl], comps[2 * l + 1][1][sl], b))
            bound = b * 2.0 ** -52
            assert abs(got.real - naive.real) <= bound * np.sum(np.abs(terms[sl].real)), (d, r)
            assert abs(got.imag - naive.imag) <= bound * np.sum(np.abs(terms[sl].imag)), (d, r)
    # the first d frames of the stream have no term
    assert not comps[4][1][:1025].any() and comps[4][1][1025:].all() and not comps[0][1][0] and comps[0][1][1:].all()


@pytest.mark.parametrize("b", (64, 1024, 4096, 131072))
def test_the_models_row_sum_is_env_models(b):
    n = 2 * b + 333
    v = lag_model.stream("cf32", n, 5).copy().view(np.float32).reshape(-1, 2)
    v[7], v[b], v[n - 2] = (np.nan, 0.0), (0.5, np.inf), (-np.inf, np.nan)
    _, s, (_, osum), nonfinite = lag_model.model(v, "cf32", b, (1, 3), _FakeOracle)
    ws, _, _, wopen, wnonfinite = env_model.model(v, "cf32", b, _FakeOracle)
    assert s.tobytes() == ws.tobytes() and osum == wopen[0] and nonfinite == wnonfinite == 3


def test_nonfinite_partners_and_absent_terms_in_the_model():
    b, d = 64, 3
    x = np.ones((2 * b, 2), np.float32)
    x[10] = (np.nan, 1.0)
    row_lag, s, _, nonfinite = lag_model.model(x, "cf32", b, (d,), _FakeOracle)
    # every present term is (1 + j) conj(1 + j) = 2: row 0 lacks frames 0 .. 2 (no partner), 10 (non-finite) and 13 (its partner)
    assert row_lag[:, 0].tolist() == [2.0 * (b - 5), 2.0 * b] and s.tolist() == [2.0 * (b - 1), 2.0 * b] and nonfinite == 1


# ---- the host helpers ----
def test_freq_against_the_model_and_its_refusals():
    rng = np.random.default_rng(3)
    for _ in range(200):
        re, im = rng.standard_normal(2) * 10.0 ** rng.integers(-20, 20)
        d, fs = int(rng.integers(1, 65537)), float(rng.uniform(1.0, 1e9))
        assert lag.freq(re, im, d, fs) == lag_model.freq(re, im, d, fs)
    assert lag.freq(0.0, 0.0, 7, FS) == 0.0 and lag.freq(-0.0, 0.0, 7, FS) == 0.0
    assert lag.freq(-1.0, 0.0, 1, FS) == FS / 2 and lag.freq(0.0, -1.0, 2, FS) == -FS / 8
    hz = C.c_double(5.0)
    for re, im, d, fs in ((math.nan, 0.0, 1, FS), (0.0, math.inf, 1, FS), (1.0, 0.0, 0, FS), (1.0, 0.0, 1, 0.0), (1.0, 0.0, 1, -FS),
                          (1.0, 0.0, 1, math.nan), (1.0, 0.0, 1, math.inf)):
        assert rc_of("iqgpu_lag_freq", re, im, d, fs, C.byref(hz)) == -1, (re, im, d, fs)


def test_estimate_rows_against_the_model():
    rng = np.random.default_rng(4)
    lags, rows = (1, 8, 2048), 40
    v = (rng.standard_normal((rows, 3)) + 1j * rng.standard_normal((rows, 3))).astype(np.complex64)
    s = (rng.uniform(1.0, 9.0, rows)).astype(np.float32)
    v[3, 1], v[9, 0], s[17] = np.nan + 1j, 1 + 1j * np.nan, np.nan        # rows 3 (lag 1), 9 (lag 0) and 17 (every lag) are skipped
    for li in range(3):
        for first, n in ((0, rows), (0, 0), (2, 5), (9, 1), (rows, 0), (16, 3)):
            assert lag.estimate(v, s, 4096, lags, li, FS, first, n) == lag_model.estimate(v, s, lags, li, first, n, FS), (li, first, n)
            assert lag.estimate(v, None, 4096, lags, li, FS, first, n) == lag_model.estimate(v, None, lags, li, first, n, FS)
    got = lag.estimate(v, None, 4096, lags, 2, FS)
    assert got["power"] == 0.0 and got["coherence"] == 0.0 and got["span_hz"] == FS / 2048
    # the zero vector
    z = lag.estimate(np.zeros((4, 3), np.complex64), np.zeros(4, np.float32), 4096, lags, 1, FS)
    assert z == dict(re=0.0, im=0.0, power=0.0, hz=0.0, coherence=0.0, span_hz=FS / 8)
    # ranges out of bounds, a lag_index beyond the lags, a bad rate
    o, est = opts(4096, lags), _lib.LagEstimate()
    p = np.ascontiguousarray(v).ctypes.data_as(C.c_void_p)
    for li, first, n, fs in ((0, 0, rows + 1, FS), (0, rows + 1, 0, FS), (0, rows, 1, FS), (0, 5, 2 ** 64 - 3, FS), (3, 0, 1, FS), (0, 0, 1, 0.0),
                             (0, 0, 1, math.nan)):
        assert rc_of("iqgpu_lag_estimate_rows", p, None, rows, C.byref(o), li, first, n, fs, C.byref(est)) == -1, (li, first, n, fs)


# ---- physical sanity on a noise-free tone 0.5 exp(2 pi i f0 n) ----
def tone(fmt, f0, n):
    z = 0.5 * np.exp(2j * np.pi * f0 * np.arange(n))
    iq = np.stack([z.real, z.imag], axis=1)
    if fmt == "cf32":
        return iq.astype(np.float32).view(np.uint8).reshape(-1)
    if fmt == "cs16":
        return np.rint(iq * 32767.0).astype(np.int16).view(np.uint8).reshape(-1)
    return (np.rint(iq * 127.0) + 128).astype(np.uint8).reshape(-1)          # cu8


def tone_estimate(fmt, f0, d, b, oracle, rows=4):
    row_lag, s, _, _ = lag_model.model(tone(fmt, f0, rows * b), fmt, b, (d,), oracle)
    got = lag.estimate(row_lag, s, b, (d,), 0, FS)
    assert got == lag_model.estimate(row_lag, s, (d,), 0, 0, rows, FS)
    return got


@pytest.mark.parametrize("fmt", ("cf32", "cs16"))
@pytest.mark.parametrize("f0,d", ((0.0123, 1), (-0.2371, 1), (0.0123, 8)))
def test_a_tone_comes_back_at_its_frequency(oracle, fmt, f0, d):
    """rounding re and im of the sum to float moves the angle by at most sqrt(2) 2^-24 rad, under 1.4e-8 fs / d; the bound of 1e-6 fs
    leaves room for the quantisation of cs16 (about 3e-10 fs at this shape)"""
    got = tone_estimate(fmt, f0, d, 4096, oracle)
    assert abs(got["hz"] - f0 * FS) <= 1e-6 * FS, got
    assert 0.999 < got["coherence"] <= 1.0 + 1e-6 and got["span_hz"] == FS / d


def test_a_cu8_tone_is_held_to_the_model_alone(oracle):
    tone_estimate("cu8", 0.0123, 1, 64, oracle)                      # (its own assertion: the library's estimate == the model's)


@pytest.mark.parametrize("fmt", ("cf32", "cs16"))
def test_a_tone_outside_the_span_comes_back_aliased(oracle, fmt):
    f0, d = -0.2371, 8
    got = tone_estimate(fmt, f0, d, 4096, oracle)
    k = (got["hz"] - f0 * FS) / got["span_hz"]
    assert round(k) != 0 and abs(k - round(k)) * got["span_hz"] <= 1e-6 * FS, (got, k)
    assert -got["span_hz"] / 2 < got["hz"] <= got["span_hz"] / 2
