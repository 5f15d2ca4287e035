"""The user filter's apply paths on the device against a float64 convolution (k_fir in kernels.hip, k_fftconv16<10..14> in fftconv.hip /
fft16.hpp, the selection in abi.cpp, the history and the block-quantised counts in process.cpp / plan.cpp).

Reference.  `want` is scipy.signal.fftconvolve in float64 of the input (as complex128) with the taps the chain itself reports
(Chain.filter_taps(), float32), zero history in front, cut to the frames the chain emitted.  The taps must equal
oracle.Filter(...).taps() bit for bit, which ties the device's design to the one the host tests pin; an FFT-kind chain must emit
floor((pending + in) / block) * block frames call by call.

Error figure.  e = max |y - want| / (sum |h| * max |x|).

Bar.  8 x the worst e of the ORACLE's Filter.apply in float32 on these very inputs, per path class of the device (the selection rule
of abi.cpp decides the class of a case; the oracle runs the same direct form for all of them).  "In float32" is the oracle built
with float accumulators (liboracle_fast.so: the same source, ORC_ACC=float), an independent float32 implementation of the operation
as the spectrum tests' complex64 transform is; the strict build accumulates in double and its error is only the rounding of the
result to float32 (e <= 4.72e-08 over all cases here), which no float32 kernel can be held to.  measure_oracle_error() below measures
it on the CPU over the cases of tests 1 and 4 (`PYTHONPATH=. python tests/test_gpu_user_filter.py` prints every figure):
    direct form    worst e = 1.37e-06 (test 1: 8194 taps, FFT kind, real low-pass)   bar = 1.10e-05
    overlap-save   worst e = 1.41e-06 (test 1: 8193 taps, FFT kind, real low-pass)   bar = 1.13e-05
(the sequential float32 sum of thousands of products: at 97 taps the same oracle is at 2.5e-07, at 2049 taps at 6.6e-07.)
The margin of 8 is the one the spectrum tests argue for: another summation or transform order may differ from the oracle's by a
small factor.
Condition.  The suite's existing filter tests hold |y - oracle| <= 1e-5 on the three-tone stream up to 6001 taps.  Where the bar
above, as an absolute error bar * sum |h| * max |x|, would exceed 1e-5 for a case with L <= 6001 on that stream, 1e-5 stands
instead (tolerance()): this module is not looser than the tests it stands beside.
Measured on an MI355X, worst e over the cases of tests 1, 4 and 5: direct form 1.37e-06 (8194 taps, FFT kind, real low-pass: the
float oracle's own figure, k_fir sums in the same order), bar 1.10e-05; overlap-save 2.97e-07 (2 taps, FFT kind, real low-pass), at
8193 taps 1.0e-07, bar 1.13e-05; the closest any case came to its bar in absolute terms is 0.12 of it.  The impulses of test 3 on
overlap-save: e <= 1.85e-08.
One tap.  The Kaiser design of length 1 is 0 / 0 in the reference's formula; the oracle does not refuse it and its tap is NaN.  No
tap count of test 1 is refused by the oracle, so none may be refused by the device; at L = 1 the device must design the same
bytes and emit NaN for every frame it owes, as the float64 convolution does (test_tap_count_axis).
Mutation check (not part of the suite): with k_fir's window base and fftconv16_tail's first output index each moved by one, all
ten impulse cases of test 3 fail, as do 64 of the 68 cases of test 1 (all but the NaN design), all of test 4 and all of test 5.

Tests.  1 the tap-count axis (every threshold of the selection rule and of the transform size, both kinds, real and complex taps,
three ways of cutting the stream); 2 the path of each case of 1 (IQGPU_FORCE_GENERIC gives the same bytes exactly where the table
says direct form; IQGPU_FFT_LOG2N set to the table's N gives the same bytes where it says overlap-save); 3 impulses; 4 kinds, even
lengths and chains; 5 the mixer in the filter's epilogue.
An even tap count reaches the library through a description edited by hand (device_filter): make_desc follows the reference's
command line and bumps an even count to the next odd one, the library designs what its description says."""
import numpy as np
import pytest

from iq_tool_amd import synth

pytestmark = pytest.mark.gpu
RATE = 2.4e6
TOL_SUITE = 1e-5                           # test_gpu_parity.TOL: the bar of the filter tests this module stands beside
MEASURED = {"direct": 1.37e-06, "os": 1.41e-06}     # measure_oracle_error(): the worst e of the float32 oracle per path class
BAR = {k: 8 * v for k, v in MEASURED.items()}
MIXER_TOL = 2e-6                           # what test_freq_shift_operator allows for the mixer

LOWPASS = (("lowpass", 300e3, 0.0),)
BANDPASS = (("passband", -250e3, 120e3),)  # negative centre: complex taps
KINDS = {"real": LOWPASS, "complex": BANDPASS}

# ---- test 1's parameter table: (L, path of the FIR kind, path of the FFT kind); 0 = the direct form k_fir, N = k_fftconv16 at N points.
# From the rule in abi.cpp, not from a run:
#   overlap-save  <=>  L >= 2 and 2 (L - 1) <= kMaxFftN = 16384 and (FFT kind or L >= kFftMinTaps = 96)
#   N = 1024; doubled while N < 4 (L - 1) and N < 4096; doubled while N < 2 (L - 1)
AXIS = [
    (1,    0,     0),          # L - 1 = 0: nothing to overlap, the direct form for either kind
    (2,    0,     1024),
    (21,   0,     1024),
    (95,   0,     1024),
    (96,   1024,  1024),       # kFftMinTaps
    (97,   1024,  1024),
    (257,  1024,  1024),       # 4 * 256 = 1024
    (258,  2048,  2048),
    (513,  2048,  2048),       # 4 * 512 = 2048
    (514,  4096,  4096),
    (2049, 4096,  4096),       # 2 * 2048 = 4096 (the rule of four stops at 4096)
    (2050, 8192,  8192),
    (4097, 8192,  8192),       # 2 * 4096 = 8192
    (4098, 16384, 16384),
    (8193, 16384, 16384),      # 2 * 8192 = 16384 = kMaxFftN: half of every window is new output
    (8194, 0,     0),          # does not fit the largest transform: back to the direct form, 33 tap chunks per output
    (9001, 0,     0),
]
AXIS_CASES = [(L, impl, kind, path) for L, p_fir, p_fft in AXIS for impl, path in (("fir", p_fir), ("fft", p_fft)) for kind in KINDS]
AXIS_IDS = ["%d-%s-%s" % c[:3] for c in AXIS_CASES]
FIR_TILE = 1024                            # kFirOutTile: k_fir's outputs per workgroup, the direct form's stand-in for V


def path_by_rule(L, fft_kind):
    """the selection rule restated, for the cases outside test 1's table (tests 4 and 5 and the measurement)"""
    if L < 2 or 2 * (L - 1) > 16384 or not (fft_kind or L >= 96):
        return 0
    N = 1024
    while N < 4 * (L - 1) and N < 4096:
        N *= 2
    while N < 2 * (L - 1):
        N *= 2
    return N


def test_the_table_restates_the_rule():
    assert [(L, path_by_rule(L, False), path_by_rule(L, True)) for L, _, _ in AXIS] == AXIS
    assert {p for _, a, b in AXIS for p in (a, b)} == {0, 1024, 2048, 4096, 8192, 16384}


# ---- the operation in float64 ----
def conv64(x, h):
    """the first len(x) frames of the linear convolution, complex128"""
    from scipy.signal import fftconvolve
    x, h = np.asarray(x).astype(np.complex128), np.asarray(h).astype(np.complex128)
    if h.size < 32 or x.size < 32:
        return np.convolve(x, h)[:x.size]
    return fftconvolve(x, h)[:x.size]


def error_figure(y, want, h, x):
    return float(np.abs(y.astype(np.complex128) - want).max() / (np.abs(h.astype(np.complex128)).sum() * np.abs(x).max()))


def tolerance(path, h, x, L, three_tone=True):
    """the bar of the case's path class as an absolute error, capped by the suite's 1e-5 where the condition above asks for it"""
    tol = BAR["os" if path else "direct"] * float(np.abs(h.astype(np.complex128)).sum()) * float(np.abs(x).max())
    return min(tol, TOL_SUITE) if three_tone and L <= 6001 else tol


def emitted(lengths, block):
    """frames an FFT-kind filter of this block emits call by call: floor((pending + in) / block) * block (src/filter.c:503-525)"""
    out, pending = [], 0
    for n in lengths:
        k = (pending + n) // block * block
        out.append(k)
        pending += n - k
    return out


def design_block(L):
    """the FFT kind's block with fft_size left to the design rule (src/filter.c:314-344)"""
    bs = 1
    while bs < L - 1:
        bs *= 2
    return bs * 2 if bs < 2 * L else bs


# ---- the oracle's and the device's filter of a case ----
def oracle_filter(oracle, reqs, L, impl="auto", rate=RATE, fast=False, **kw):
    cfg = oracle.make_filter_cfg(reqs, filter_taps=L, impl=impl, **kw)
    return oracle.Filter(cfg, rate, rate, no_resample=True, L=oracle.lib(fast=fast))


def device_filter(reqs, L, impl="auto", rate=RATE, **kw):
    """ops.Filter on a description that carries the tap count as given, even ones too"""
    from iq_tool_amd import ops
    from iq_tool_amd.chain import make_desc
    d = make_desc(in_format="cf32", out_format="cf32", input_rate_hz=rate, no_resample=True, filters=tuple(reqs), filter_taps=L,
                  filter_impl=impl, **kw)
    d.filter_taps = L
    return ops.Filter(reqs, rate, desc=d)


def feed(op, x, lengths):
    """the stream in calls of the given lengths; (output, frames emitted per call)"""
    outs, at = [], 0
    for n in lengths:
        outs.append(op.apply(x[at:at + n]))
        at += n
    assert at == x.size
    return np.concatenate(outs), [o.size for o in outs]


def cycling(n, lengths):
    out, i = [], 0
    while n > 0:
        out.append(min(lengths[i % len(lengths)], n))
        n -= out[-1]
        i += 1
    return out


def axis_geometry(L, impl, path):
    """(V, stream length, block) of a case of test 1: two windows' worth of new output plus L plus 37 frames, and at least two
    design blocks plus 37 for the FFT kind"""
    V = path - (L - 1) if path else FIR_TILE
    n = 2 * V + L + 37
    block = design_block(L) if impl == "fft" else 0
    return V, max(n, 2 * block + 37), block


def axis_variants(n, V):
    return {"one call": [n], "1, V - 1, 1, rest": [1, V - 1, 1, n - V - 1], "1023, 1025, 7 cycling": cycling(n, (1023, 1025, 7))}


def axis_input(L, impl, path):
    return synth.complex_signal(axis_geometry(L, impl, path)[1], RATE, 100 + L)


def check_against_float64(y, counts, x, lengths, h, block, path, L, what, extra=0.0, mix=None, want=None, three_tone=True):
    """the counts call by call, then the float64 bar; returns the error figure"""
    assert counts == (emitted(lengths, block) if block else list(lengths)), what
    want = (conv64(x, h) if want is None else want)[:y.size]
    if mix is not None:
        want = mix(want.astype(np.complex64)).astype(np.complex128)
    tol = tolerance(path, h, x, L, three_tone) + extra
    err = float(np.abs(y.astype(np.complex128) - want).max()) if y.size else 0.0
    e = err / (np.abs(h.astype(np.complex128)).sum() * np.abs(x).max())
    print("%s: e = %.3g, |err| = %.3g (bar %.3g)" % (what, e, err, tol))
    assert np.isfinite(y.view(np.float32)).all() and err <= tol, (what, err, tol)
    return e


_default_runs = {}


def default_run(L, impl, kind, path):
    """the default chain's one-call output of a case of test 1 and its taps, computed once (tests 1 and 2 share it)"""
    key = (L, impl, kind)
    if key not in _default_runs:
        op = device_filter(KINDS[kind], L, impl)
        _default_runs[key] = (op.apply(axis_input(L, impl, path)), op.chain.filter_taps())
    return _default_runs[key]


def oracle_filter_or_refusal(oracle, reqs, L, impl, **kw):
    """the oracle's filter, or None where the oracle refuses the description; the device must then refuse it as a filter error too"""
    from iq_tool_amd._lib import IqgpuError
    try:
        return oracle_filter(oracle, reqs, L, impl, **kw)
    except ValueError:
        with pytest.raises(IqgpuError) as info:
            device_filter(reqs, L, impl, **kw)
        assert info.value.code == -7            # IQGPU_EFILTER
        return None


# ---- 1. the tap-count axis ----
@pytest.mark.parametrize("L,impl,kind,path", AXIS_CASES, ids=AXIS_IDS)
def test_tap_count_axis(gpu, oracle, L, impl, kind, path):
    """k_fir accumulates an output's products in tap order k = 0 .. L - 1 with explicit fmaf, chunk after chunk into the same
    registers, from a zero start; where the call begins changes which workgroup and lane own the output and nothing in that
    sequence (kernels.hip, k_fir).  So on the direct form every way of cutting the stream gives the same bytes."""
    reqs = KINDS[kind]
    f = oracle_filter_or_refusal(oracle, reqs, L, impl)
    if f is None:
        return
    V, n, block = axis_geometry(L, impl, path)
    x = axis_input(L, impl, path)
    assert f.ntaps == L and f.block == block
    first = None
    for name, lengths in axis_variants(n, V).items():
        what = "%d %s %s, %s" % (L, impl, kind, name)
        if name == "one call":
            y, h = default_run(L, impl, kind, path)
            counts = [y.size]
        else:
            op = device_filter(reqs, L, impl)
            h = op.chain.filter_taps()
            y, counts = feed(op, x, lengths)
        assert h.tobytes() == f.taps().tobytes(), what
        if np.isfinite(h.view(np.float32)).all():
            check_against_float64(y, counts, x, lengths, h, block, path, L, what)
        else:
            # one tap: the Kaiser window of length 1 is 0 / 0 in the reference's formula, the oracle does not refuse it and its tap
            # is NaN.  The device designs the same bytes, emits the frames it owes, and every one of them is NaN in both parts, as
            # in the float64 convolution
            assert L == 1 and counts == (emitted(lengths, block) if block else list(lengths)), what
            assert np.isnan(conv64(x, h).real).all() and np.isnan(conv64(x, h).imag).all()
            assert np.isnan(y.real).all() and np.isnan(y.imag).all(), what
        if first is None:
            first = y
        if path == 0:
            assert y.tobytes() == first.tobytes(), "the direct form's bytes depend on the cut: " + what


# ---- 2. the path of each case ----
@pytest.mark.parametrize("L,impl,kind,path", AXIS_CASES, ids=AXIS_IDS)
def test_the_case_runs_the_path_of_its_table_entry(gpu, oracle, monkeypatch, L, impl, kind, path):
    reqs = KINDS[kind]
    if oracle_filter_or_refusal(oracle, reqs, L, impl) is None:
        return
    x = axis_input(L, impl, path)
    y, _ = default_run(L, impl, kind, path)
    monkeypatch.setenv("IQGPU_FORCE_GENERIC", "1")
    direct = device_filter(reqs, L, impl).apply(x)
    monkeypatch.delenv("IQGPU_FORCE_GENERIC")
    assert direct.size == y.size
    if path == 0:
        assert direct.tobytes() == y.tobytes(), "the table says direct form, the default run is something else"
        return
    assert direct.tobytes() != y.tobytes(), "the table says overlap-save, the default run is the direct form"
    # the transform size: forced to the table's N the chain is the default chain; forced to another, it is not
    for N, same in ((path, True), (path * 2 if path < 16384 else path // 2, False)):
        if N < 2 * (L - 1):
            continue                            # (the switch is ignored where the taps do not fit: nothing to tell apart)
        monkeypatch.setenv("IQGPU_FFT_LOG2N", str(N.bit_length() - 1))
        forced = device_filter(reqs, L, impl).apply(x)
        monkeypatch.delenv("IQGPU_FFT_LOG2N")
        assert (forced.tobytes() == y.tobytes()) == same, "N = %d forced: %s bytes as the default run" % (N, "other" if same else "the same")


# ---- 3. impulses ----
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("L", [21, 95, 8194])
def test_direct_form_returns_its_taps_for_a_unit_impulse(gpu, L, kind):
    """times one and plus zero are exact: the response to 1 + 0j at frame 0 is the taps, value for value"""
    assert path_by_rule(L, False) == 0
    x = np.zeros(L + FIR_TILE + 37, np.complex64)
    x[0] = 1.0
    op = device_filter(KINDS[kind], L, "fir")
    h = op.chain.filter_taps()
    y = op.apply(x)
    assert h.size == L and y.size == x.size and np.abs(h).max() > 0
    assert np.array_equal(y[:L], h)
    assert not y[L:].any()
    op = device_filter(KINDS[kind], L, "fir")
    y2, _ = feed(op, x, [1, L - 1, 1, x.size - L - 1])
    assert np.array_equal(y2, y)


AMPLITUDES = np.array([1.0, 0.5 - 0.25j, -0.75j, 0.3 + 0.6j, -1.0 + 0.5j], np.complex64)


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("L,N", [(97, 1024), (8193, 16384)])
def test_overlap_save_impulses_at_the_window_seams(gpu, L, N, kind):
    assert path_by_rule(L, False) == N
    V = N - (L - 1)
    n = 2 * V + L + 37
    at = np.array([0, V - 1, V, 2 * V - 1, n - 1])
    x = np.zeros(n, np.complex64)
    x[at] = AMPLITUDES
    # frames further than L - 1 behind the last impulse in front of them: the float64 result there is exactly zero
    since = np.arange(n) - at[np.searchsorted(at, np.arange(n), side="right") - 1]
    silent = since > L - 1
    assert silent.any()
    # the float64 convolution of a few impulses, term by term: exactly zero where no response reaches
    def response64(h):
        want = np.zeros(n + L, np.complex128)
        for k, a in zip(at, AMPLITUDES):
            want[k:k + L] += np.complex128(a) * h.astype(np.complex128)
        return want[:n]

    for name, lengths in (("one call", [n]), ("cut at V - 1 and V", [V - 1, 1, n - V])):
        op = device_filter(KINDS[kind], L, "fir")
        h = op.chain.filter_taps()
        y, counts = feed(op, x, lengths)
        what = "impulses, %d taps %s, %s" % (L, kind, name)
        want = response64(h)
        assert not want[silent].any() and np.abs(want - conv64(x, h)).max() <= 1e-12
        check_against_float64(y, counts, x, lengths, h, 0, N, L, what, want=want, three_tone=False)
        tol = tolerance(N, h, x, L, three_tone=False)
        assert np.abs(y[silent]).max() <= tol, (what, float(np.abs(y[silent]).max()), tol)


# ---- 4. kinds and chains ----
STOP = ("stopband", 100e3, 40e3)
FIVE = (("lowpass", 500e3, 0.0), ("highpass", 50e3, 0.0), ("passband", 250e3, 300e3), STOP, ("passband", 0.0, 700e3))
KIND_CASES = (
    [(name, reqs, L, {}) for L in (129, 0) for name, reqs in (
        ("low-pass", LOWPASS), ("high-pass", (("highpass", 300e3, 0.0),)), ("band-pass at 0", (("passband", 0.0, 240e3),)),
        ("band-pass at +250 kHz", (("passband", 250e3, 120e3),)), ("band-pass at -250 kHz", BANDPASS), ("band-stop", (STOP,)),
        ("low-pass, band-stop", (("lowpass", 400e3, 0.0), STOP)), ("five requests", FIVE))]
    + [("high-pass", (("highpass", 300e3, 0.0),), 128, {}), ("band-stop", (STOP,), 128, {})]
    + [("low-pass, 100 dB", LOWPASS, L, dict(attenuation_db=100.0, transition_width_hz=30e3)) for L in (129, 128, 0)]
    + [("low-pass at 250 kS/s", (("lowpass", 30e3, 0.0),), L, dict(rate=250e3)) for L in (129, 0)])


def kind_geometry(oracle, reqs, L, kw):
    """(oracle filter, path, stream, call lengths) of a case of test 4"""
    f = oracle_filter(oracle, reqs, L, **kw)
    path = path_by_rule(f.ntaps, f.block > 0)
    n = 30011 + 2 * f.block
    x = synth.complex_signal(n, kw.get("rate", RATE), 200 + L + len(reqs))
    return f, path, x, [5000, 1, 12345, n - 17346]


@pytest.mark.parametrize("name,reqs,L,kw", KIND_CASES, ids=["%s-%d" % (c[0], c[2]) for c in KIND_CASES])
def test_kinds_and_chains(gpu, oracle, name, reqs, L, kw):
    f, path, x, lengths = kind_geometry(oracle, reqs, L, kw)
    op = device_filter(reqs, L, **kw)
    h = op.chain.filter_taps()
    assert h.tobytes() == f.taps().tobytes()
    if L:
        assert h.size == len(reqs) * (L - 1) + 1       # (five requests of 129 taps: 641)
    else:
        assert h.size % 2 == 1 and h.size >= 21
    y, counts = feed(op, x, lengths)
    check_against_float64(y, counts, x, lengths, h, f.block, path, h.size, "%s, %d -> %d taps, path %d" % (name, L, h.size, path))


# ---- 5. the mixer in the filter's epilogue ----
@pytest.mark.parametrize("L,path,shift", [(33, 0, 200e3), (97, 1024, -333.3e3), (8193, 16384, 200e3)])
def test_post_mixer_in_the_filters_epilogue(gpu, oracle, L, path, shift):
    """filter, then the mixer (shift_after_resample) in the same kernel: the float64 convolution rounded to cf32 and mixed by the
    oracle's NCO, an exact table lookup (test_oracle.py)"""
    assert path_by_rule(L, False) == path
    V = path - (L - 1) if path else FIR_TILE
    n = 2 * V + L + 37
    x = synth.complex_signal(n, RATE, 300 + L)
    op = device_filter(LOWPASS, L, "fir", shift_hz=shift, shift_after_resample=True)
    h = op.chain.filter_taps()
    assert h.tobytes() == oracle_filter(oracle, LOWPASS, L, "fir").taps().tobytes()
    lengths = [1, V - 1, 1, 333, n - V - 334]
    y, counts = feed(op, x, lengths)
    nco = oracle.Nco(np.float32(2 * np.pi * abs(shift) / RATE))
    check_against_float64(y, counts, x, lengths, h, 0, path, L, "post mixer, %d taps" % L, extra=MIXER_TOL,
                          mix=lambda w: nco.mix(w, up=shift >= 0))


# ---- the bar: the oracle's float32 error on the inputs of tests 1 and 4, on the CPU ----
def measure_oracle_error(oracle):
    """[(e of the float-accumulator build, e of the strict build, path class, what)]"""
    rows = []

    def figures(reqs, L, impl, x, kw, what, path=None):
        es = []
        for fast in (True, False):
            try:
                f = oracle_filter(oracle, reqs, L, impl, fast=fast, **kw)
            except ValueError:
                print("refused by the oracle: " + what)
                return
            h = f.taps()
            y = f.apply(x)
            es.append(error_figure(y, conv64(x, h)[:y.size], h, x))
        p = path_by_rule(f.ntaps, f.block > 0)
        assert path is None or p == path
        rows.append((es[0], es[1], "os" if p else "direct", what + ("" if np.isfinite(h.view(np.float32)).all() else " (the taps are not finite)")))

    for L, impl, kind, path in AXIS_CASES:
        figures(KINDS[kind], L, impl, axis_input(L, impl, path), {}, "axis %d %s %s" % (L, impl, kind), path)
    for name, reqs, L, kw in KIND_CASES:
        x = kind_geometry(oracle, reqs, L, kw)[2]
        figures(reqs, L, "auto", x, kw, "kinds %s %d" % (name, L))
    return rows


if __name__ == "__main__":
    from oracle import pyoracle
    pyoracle.build()
    rows = measure_oracle_error(pyoracle)
    for e32, e64, cls, what in rows:
        print("e = %.3g  (strict build %.3g)  %-6s  %s" % (e32, e64, cls, what))
    rows = [r for r in rows if np.isfinite(r[0])]               # (one tap: see test_tap_count_axis)
    print("strict build, worst of all: %.3g" % max(r[1] for r in rows))
    for cls in ("direct", "os"):
        w = max((r for r in rows if r[2] == cls), key=lambda r: r[0])
        print("%-6s worst e = %.3g (%s)   bar = %.3g" % (cls, w[0], w[3], 8 * w[0]))
