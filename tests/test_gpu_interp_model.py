"""k_interp (iq_tool_amd/csrc/interp.hip: every chain with r > 1, and r = 1 behind a pre-resample filter) against the float64 model
of tests/interp_model.py -- not against the oracle, which tests/test_interp_model_host.py holds to the same model.

1. - 3.  ops.Resampler(r), cf32 in and out, against the model.  THE BAR is derived per case, on that very input:
       E_f = max |float-accumulator oracle - model|          (oracle.lib(fast=True): float32 sums in ONE chain, on the CPU)
       max |device - model| <= 8 E_f + (S + 2) 2^-24 max|model|,  and never more than the contract's 1e-5.
   8 is what tests/test_gpu_psd.py grants a float32 computation with another summation order (the kernel's half-band branches sum
   in two chains and use fused multiply-adds, the float build sums in one); the floor is one rounding per stage, for inputs where E_f
   happens to be 0.  Every case prints E_f, the bar and the device's error before it asserts (pytest -s).
   E_f measured on the CPU (`PYTHONPATH=. python tests/test_gpu_interp_model.py` prints them), dense cases of test a:
       r       1.0      1+2^-23  1.37     1.999    2.0      2+2^-22  3.3      5.3      47.9     480
       S       0        0        0        0        0        1        1        2        5        8
       E_f     1.52e-07 1.63e-07 1.50e-07 1.55e-07 1.38e-07 2.31e-07 1.96e-07 2.33e-07 2.51e-07 3.44e-07
       bar     1.31e-06 1.39e-06 1.29e-06 1.33e-06 1.20e-06 1.99e-06 1.70e-06 2.04e-06 2.32e-06 3.19e-06
   the 3 x 2^20-output case of test c: E_f 4.10e-07, bar 3.60e-06; one impulse (0.7 - 0.3j), worst E_f over the runs of test b:
   r = 1.37 2.78e-08 (bar 2.97e-07: an output is ONE product there), r = 2 1.65e-08 (2.21e-07), r = 5.3 1.10e-07 (1.05e-06),
   r = 480 2.44e-07 (2.39e-06).  The float build is compiled for the machine it runs on, so E_f may differ in its last digit from
   CPU to CPU; the tests compute it where they run.  The MI355X figures are in DESIGN.md section 1.
   a. dense, >= 5 tiles of 2048 final outputs in one call, every shape of the cascade: step 2^23 (r = 2), mixed one-bit distances
      between the two outputs of a pair (1.37, 1.999), 64 and 8 resampler outputs per tile (47.9, 480; at 480 the rebuilt prefix
      ext[0] is longer than the tile).  What the ratios of the issue turned out to be: msresamp interpolates for r > 1 and halves
      while rate_arb > 2, so r = 1.0 is NOT k_interp (S = 0, the decimating twin's kernel k_front_s1 at step 2^24; kept, held to the
      same model and bar, its kernel asserted) and r = 2.0 has S = 0 and rate_arb 2.  The two shapes meant -- every pair at distance
      1, and one half-band stage behind rate_arb ~ 1 -- are the next float32 above: r = 1 + 2^-23 (step 2^24 - 2, S = 0) and
      r = 2 + 2^-22 (step 2^24 - 2, S = 1), both k_interp.  A step of exactly 2^24 reaches k_interp only behind a pre-resample
      filter (tests/test_gpu_parity.py::test_chain_filter_then_unit_ratio_resampler).
   b. one impulse per run at the seams: stream start, tile boundaries 2048 j (j = 1, 3), call boundaries (the last 1, 14 and `hist`
      samples of call 1); outside the structural support of the response every output is exactly 0.0.
   c. second tile trips: more tiles than 4 x CUs workgroups (asserted), dense, and bytes equal to a two-call run cut at an odd input.
   d. splits: any call schedule gives the bytes of the one call.
4. every pack of k_interp, bit for bit: the integer chain's bytes EQUAL oracle.from_cf32(cf32 twin's frames, format) -- the twin is
   the same kernel instantiation with out_fmt = cf32, so the float pair is the same and only the store differs.  All eight integer
   formats, S = 0 and S = 2, with and without the post-resample shift, an odd number of outputs (the lone-frame pack_store
   fallback), a three-call schedule with odd per-call counts into ONE device buffer (pair stores at odd frame offsets), guard bytes
   behind the last frame, >= 5 % of the components clamped and >= 50 % not (asserted on the twin's output)."""
import numpy as np
import pytest

from interp_model import (ARB_TAPS, TILE, first_input_reaching, impulse_support, interp_geometry, numpy_msresamp_interp, stage_order)
from iq_tool_amd import synth

pytestmark = pytest.mark.gpu
TOL = 1e-5
SEED = 83
IMPULSE = 0.7 - 0.3j
R_ABOVE_1 = float(np.nextafter(np.float32(1.0), np.float32(2.0)))
R_ABOVE_2 = float(np.nextafter(np.float32(2.0), np.float32(3.0)))
# ratio -> (interp, S, front_kernel())
DENSE = {1.0: (False, 0, "k_front_s1"), R_ABOVE_1: (True, 0, "k_front+k_interp"), 1.37: (True, 0, "k_front+k_interp"),
         1.999: (True, 0, "k_front+k_interp"), 2.0: (True, 0, "k_front+k_interp"), R_ABOVE_2: (True, 1, "k_front+k_interp"),
         3.3: (True, 1, "k_front+k_interp"), 5.3: (True, 2, "k_front+k_interp"), 47.9: (True, 5, "k_front+k_interp"),
         480.0: (True, 8, "k_front+k_interp")}
SEAM_RATIOS = (1.37, 2.0, 5.3, 480.0)


def design(oracle, r):
    m = oracle.MsResamp(np.float32(r))
    assert (m.interp, m.S) == DENSE[r][:2], (r, m.interp, m.S)
    return m


def dense_frames(r):
    """at least 5.5 tiles of final outputs, at least 1000 inputs, ragged"""
    return max(int(np.ceil(5.5 * TILE / r)), 1000) + 37


def dense_input(r):
    x = synth.complex_signal(dense_frames(r), 2.4e6, SEED)
    x.setflags(write=False)
    return x


def impulse_input(n, pos):
    x = np.zeros(n, np.complex64)
    x[pos] = IMPULSE
    return x


def bar_of(oracle, m, r, x, want):
    """(E_f, bar) of one input: the float-accumulator oracle against the model on the CPU"""
    fast = oracle.MsResamp(np.float32(r), L=oracle.lib(fast=True)).execute(x)
    assert fast.size == want.size
    e_f = float(np.abs(fast - want).max()) if want.size else 0.0
    bar = min(TOL, 8.0 * e_f + (m.S + 2) * 2.0 ** -24 * float(np.abs(want).max()))
    return e_f, bar


def check_routing(rs, m, r):
    info = rs.chain.info()
    assert (bool(info.interp), int(info.num_halfband_stages), int(info.arb_step)) == (m.interp, m.S, m.step), r
    assert [int(info.stage_m[k]) for k in range(m.S)] == [m.stage_m(k) for k in range(m.S)], r
    assert rs.chain.front_kernel() == DENSE[r][2], (r, rs.chain.front_kernel())


def run_calls(rs, x, sizes):
    """x through the operator in calls of the given sizes and the rest"""
    outs, pos = [], 0
    for k in list(sizes) + [x.size - sum(sizes)]:
        assert 0 < k <= x.size - pos
        outs.append(rs.execute(x[pos:pos + k]))
        pos += k
    assert pos == x.size
    return np.concatenate(outs)


def same_bytes(a, b, what):
    assert a.size == b.size, (what, a.size, b.size)
    ne = a.view(np.uint8) != b.view(np.uint8)
    assert not ne.any(), (what, int(ne.sum()), int(np.flatnonzero(ne)[0]))


_dense = {}


def dense_case(oracle, r):
    """(design, input, model, E_f, bar) of test a's case, made once"""
    if r not in _dense:
        m = design(oracle, r)
        x = dense_input(r)
        want = numpy_msresamp_interp(m, x)
        want.setflags(write=False)
        _dense[r] = (m, x, want) + bar_of(oracle, m, r, x, want)
    return _dense[r]


# --------------------------------------------------------------------------------------------
# a. dense, per shape
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", sorted(DENSE))
def test_dense_against_the_model(gpu, oracle, r):
    from iq_tool_amd import ops
    m, x, want, e_f, bar = dense_case(oracle, r)
    ext, hist = interp_geometry(m)
    assert want.size >= 5 * TILE
    if r == 2.0:
        assert m.step == 1 << 23
    if r in (R_ABOVE_1, R_ABOVE_2):
        assert m.step == (1 << 24) - 2                       # every pair of this stream at distance 1: the first repeat is 2^23 outputs away
    if r == 47.9:
        assert TILE >> m.S == 64
    if r == 480.0:
        assert TILE >> m.S == 8 and ext[0] > TILE >> m.S
    rs = ops.Resampler(np.float32(r))
    got = rs.execute(x)
    check_routing(rs, m, r)
    assert got.size == want.size
    err = float(np.abs(got - want).max())
    print("r = %.9g (S = %d, step %d, ext %s, hist %d): %d in, %d out; E_f %.3g, bar %.3g, device %.3g, peak %.3f"
          % (r, m.S, m.step, ext, hist, x.size, got.size, e_f, bar, err, float(np.abs(want).max())))
    assert float(np.abs(want).max()) > 0.5
    assert err <= bar


# --------------------------------------------------------------------------------------------
# b. impulses at the seams
# --------------------------------------------------------------------------------------------
def seam_runs(m):
    """[(what, n, sizes of the calls before the last, impulse position)] for one design"""
    ext, hist = interp_geometry(m)
    m_last = m.stage_m(0) if m.S else ARB_TAPS // 2          # the stage at the output rate (S = 0: the arbitrary stage's own semi-length)
    runs, seen = [], set()
    for p in (0, 13):
        runs.append(("stream start", p + hist + 40, [], p))
    for j in (1, 3):
        for d in (1, 2, 2 * m_last):
            p = first_input_reaching(m, TILE * j - d)
            lo, hi = impulse_support(m, p)
            assert TILE * j - d - (2 << m.S) <= lo <= TILE * j - d and lo < TILE * j <= hi, (j, d, p, lo, hi)   # the response straddles the boundary
            if p not in seen:
                seen.add(p)
                runs.append(("tile boundary %d, first response sample %d before it" % (TILE * j, TILE * j - lo), p + hist + 40, [], p))
        # ... and the other end: the earliest input whose response still reaches the tile -- its last samples are made from the
        # deepest samples of the prefix the tile rebuilds (ext[])
        p = first_input_reaching(m, TILE * j)
        while p > 0 and impulse_support(m, p - 1)[1] >= TILE * j:
            p -= 1
        if p not in seen:
            seen.add(p)
            runs.append(("tile boundary %d, last response sample %d behind it" % (TILE * j, impulse_support(m, p)[1] - TILE * j), p + hist + 40, [], p))
    n1 = hist + 51
    first_of_call_2 = -(-(n1 << 24) // m.step) << m.S
    reaches = [back for back in range(1, n1 + 1) if impulse_support(m, n1 - back)[1] >= first_of_call_2]
    # call 2 reads the response of the last `deepest` samples of call 1 and of no sample in front of them: the history k_interp keeps
    # covers them (a 14-tap window ending at x[q] makes the 14th sample from the end the first one that S = 0 no longer needs)
    deepest = reaches[-1]
    assert reaches == list(range(1, deepest + 1)) and ARB_TAPS - 1 <= deepest <= hist, (deepest, hist)
    for back in sorted({1, ARB_TAPS, deepest, deepest + 1, hist}):
        runs.append(("call boundary, impulse %d before it (call 2 reads the last %d)" % (back, deepest), n1 + hist + 60, [n1], n1 - back))
    return runs


@pytest.mark.parametrize("r", SEAM_RATIOS)
def test_one_impulse_at_every_seam(gpu, oracle, r):
    from iq_tool_amd import ops
    m = design(oracle, r)
    ext, hist = interp_geometry(m)
    rs = ops.Resampler(np.float32(r))
    worst = 0.0
    for what, n, sizes, p in seam_runs(m):
        x = impulse_input(n, p)
        want = numpy_msresamp_interp(m, x)
        e_f, bar = bar_of(oracle, m, r, x, want)
        rs.reset()
        got = run_calls(rs, x, sizes)
        check_routing(rs, m, r)
        assert got.size == want.size
        lo, hi = impulse_support(m, p)
        assert hi < want.size, (what, hi, want.size)
        err = float(np.abs(got - want).max())
        worst = max(worst, e_f)
        print("r = %g, %s (input %d of %d, response [%d, %d]): E_f %.3g, bar %.3g, device %.3g" % (r, what, p, n, lo, hi, e_f, bar, err))
        outside = np.ones(want.size, bool)
        outside[lo:hi + 1] = False
        assert not want[outside].any()
        assert np.abs(want[lo:hi + 1]).max() > 0.3
        z = got[outside].view(np.float32)
        assert not z.any(), (what, int(np.count_nonzero(z)))             # exactly 0.0 (either sign) outside the response
        assert err <= bar, (what, err, bar)
    print("r = %g: worst E_f over the seams %.3g; ext %s, hist %d" % (r, worst, ext, hist))


# --------------------------------------------------------------------------------------------
# c. second tile trips
# --------------------------------------------------------------------------------------------
def long_input(oracle):
    m = design(oracle, 47.9)
    n = -(-((3 << 20) >> m.S) * m.step >> 24) + 8            # >= 3 x 2^20 final outputs
    x = synth.complex_signal(n, 2.4e6, SEED + 1)
    return m, x


def compute_units():
    """the largest CU count of a GPU of this machine, from the KFD topology the library's own device binding reads (simd_count /
    simd_per_cu of the nodes with SIMDs): an upper bound of the count launch_interp sizes its grid with.  The library does not
    expose that count, and a second HIP runtime (torch's) in a process that has the library's open finds no device."""
    import glob
    best = 0
    for path in glob.glob("/sys/class/kfd/kfd/topology/nodes/*/properties"):
        try:
            with open(path) as fh:
                prop = dict(line.split()[:2] for line in fh if len(line.split()) >= 2)
        except OSError:
            continue
        simd = int(prop.get("simd_count", 0))
        if simd > 0:
            best = max(best, simd // max(1, int(prop.get("simd_per_cu", 4))))
    if best == 0:
        pytest.fail("no GPU node in the KFD topology: cannot tell how many workgroups launch_interp starts")
    return best


def test_workgroups_take_further_tiles(gpu, oracle):
    """launch_interp caps the grid at 4 x CUs workgroups; a workgroup then loops over tiles t, t + grid, ... and reuses its LDS
    behind the __syncthreads() at the top of the loop"""
    from iq_tool_amd import ops
    r = 47.9
    m, x = long_input(oracle)
    want = numpy_msresamp_interp(m, x)
    e_f, bar = bar_of(oracle, m, r, x, want)
    n_tiles = -(-want.size // TILE)
    cus = compute_units()
    print("r = %g: %d in, %d out, %d tiles, %d CUs (grid cap %d)" % (r, x.size, want.size, n_tiles, cus, 4 * cus))
    assert want.size >= 3 << 20 and n_tiles > 4 * cus
    rs = ops.Resampler(np.float32(r))
    got = rs.execute(x)
    check_routing(rs, m, r)
    assert got.size == want.size
    err = float(np.abs(got - want).max())
    print("r = %g long: E_f %.3g, bar %.3g, device %.3g" % (r, e_f, bar, err))
    assert err <= bar
    cut = (x.size // 2) | 1
    rs.reset()
    two = run_calls(rs, x, [cut])
    same_bytes(two, got, "two calls cut at input %d" % cut)


# --------------------------------------------------------------------------------------------
# d. splits
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [1.37, 5.3])
def test_any_split_gives_the_bytes_of_one_call(gpu, oracle, r):
    from iq_tool_amd import ops
    m, x, want, e_f, bar = dense_case(oracle, r)
    rs = ops.Resampler(np.float32(r))
    base = rs.execute(x)
    assert base.size == want.size and np.abs(base - want).max() <= bar
    rs.reset()
    same_bytes(run_calls(rs, x, [1, 2, 13, 14, 15]), base, "calls of 1, 2, 13, 14, 15 and the rest")
    check_routing(rs, m, r)
    p = first_input_reaching(m, TILE)                         # the input that maps to final output 2048
    for cut in range(p - 2, p + 3):
        rs.reset()
        same_bytes(run_calls(rs, x, [cut]), base, "cut at input %d (output %d)" % (cut, -(-(cut << 24) // m.step) << m.S))


# --------------------------------------------------------------------------------------------
# 4. every pack, bit for bit
# --------------------------------------------------------------------------------------------
# format -> (scale, offset, clamp low, clamp high) of v = x scale + offset (src/sample_convert.c:213-300), bytes per frame
PACK = {"cs16": (32767.0, 0.0, -32768.0, 32767.0, 4), "sc16q11": (2048.0, 0.0, -32768.0, 32767.0, 4),
        "cu16": (32767.0, 32767.5, 0.0, 65535.0, 4), "cs8": (127.0, 0.0, -128.0, 127.0, 2), "cu8": (127.0, 127.5, 0.0, 255.0, 2),
        "cs24": (8388607.0, 0.0, -8388608.0, 8388607.0, 6), "cs32": (2147483647.0, 0.0, -2147483648.0, 2147483647.0, 8),
        "cu32": (2147483647.0, 2147483647.5, 0.0, 4294967295.0, 8)}
PACK_N = 6000
GUARD = 64                                                  # bytes behind the last frame that no store may touch


def stimulus_gain(fmt):
    """sc16q11 clamps at |x| = 16, every other format at |x| = 1: the synthetic stream times this has 0.20 - 0.21 of the output
    components beyond the clamp and 0.79 - 0.80 inside (the oracle's chain on the CPU, both ratios, with and without the shift)"""
    return 48.0 if fmt == "sc16q11" else 3.0


def pack_desc(r, shifted, out_format):
    kw = dict(in_format="cf32", out_format=out_format, input_rate_hz=1e6, resample_ratio=float(np.float32(r)))
    if shifted:
        kw.update(shift_hz=0.11e6, shift_after_resample=True)
    return kw


def odd_schedule(step, n_min):
    """(n, [a, b]): a stream length and two cuts such that the arbitrary stage emits an ODD number of outputs in each of the three
    calls (so the total is odd too)"""
    count = lambda a: -(-(a << 24) // step)
    a = next(k for k in range(n_min // 3, n_min) if count(k) % 2 == 1)
    b = next(k for k in range(a + n_min // 3, 2 * n_min) if (count(k) - count(a)) % 2 == 1)
    n = next(k for k in range(max(n_min, b + 100), 3 * n_min) if (count(k) - count(b)) % 2 == 1)
    return n, [a, b - a]


def run_device(gpu, kw, x, sizes):
    """the chain over x in calls of the given sizes and the rest, device to device, every call's output written right behind the
    last one's in ONE buffer filled with a pattern: (bytes of the frames, frames per call, guard bytes behind them, front_kernel())"""
    from iq_tool_amd.chain import DeviceBuffer
    ch = gpu.Chain(**kw)
    bpf = ch.out_bytes
    sizes = list(sizes) + [x.size - sum(sizes)]
    cap = sum(ch.max_out_frames(k) for k in sizes) * bpf + GUARD
    d_in, d_out = DeviceBuffer(x.nbytes), DeviceBuffer(cap)
    try:
        d_in.upload(x)
        d_out.upload(np.full(cap, 0xA5, np.uint8))
        pos = done = 0
        counts = []
        for k in sizes:
            got = ch.process_device(d_in.ptr + pos * 8, k, d_out.ptr + done * bpf, cap - GUARD - done * bpf)
            counts.append(got)
            pos += k
            done += got
        ch.synchronize()
        raw = d_out.download(done * bpf + GUARD)
        kernel = ch.front_kernel()
        info = ch.info()
    finally:
        d_in.free(); d_out.free()
    return raw[:done * bpf].copy(), counts, raw[done * bpf:].copy(), kernel, info


_twin = {}


def twin_of(gpu, oracle, r, shifted, gain, x, sizes):
    """the cf32-output twin's frames on the same schedule, made once per (r, shift, gain)"""
    key = (r, shifted, gain)
    if key not in _twin:
        raw, counts, guard, kernel, info = run_device(gpu, pack_desc(r, shifted, "cf32"), x, sizes)
        assert kernel == "k_front+k_interp" and (guard == 0xA5).all()
        frames = raw.view(np.complex64)
        frames.setflags(write=False)
        _twin[key] = (frames, counts)
    return _twin[key]


@pytest.mark.parametrize("shifted", [False, True], ids=["plain", "post_shift"])
@pytest.mark.parametrize("r", [1.37, 5.3])
@pytest.mark.parametrize("fmt", sorted(PACK))
def test_every_pack_is_the_reference_pack_of_the_cf32_twin(gpu, oracle, fmt, r, shifted):
    m = design(oracle, r)
    n, sizes = odd_schedule(m.step, PACK_N)
    gain = stimulus_gain(fmt)
    x = (synth.complex_signal(n, 1e6, SEED + 2) * np.float32(gain)).astype(np.complex64)
    count = lambda a: -(-(a << 24) // m.step)
    per_call = [count(sizes[0]), count(sizes[0] + sizes[1]) - count(sizes[0]), count(n) - count(sizes[0] + sizes[1])]
    assert all(c % 2 == 1 for c in per_call) and count(n) % 2 == 1
    try:
        gpu.Chain(**pack_desc(r, shifted, fmt)).close()
    except gpu.IqgpuError:
        okw = dict(pack_desc(r, shifted, fmt), target_rate_hz=1e6 * float(np.float32(r)))
        okw.pop("resample_ratio")
        with pytest.raises(ValueError):
            oracle.Chain(**okw)
        return
    twin, twin_counts = twin_of(gpu, oracle, r, shifted, gain, x, sizes)
    assert twin_counts == [c << m.S for c in per_call] and twin.size == count(n) << m.S
    # the stimulus is hard: the clamp acts on >= 5 % of the components and leaves >= 50 % alone
    scale, off, lo, hi, bpf = PACK[fmt]
    v = twin.view(np.float32).astype(np.float64) * scale + off
    clamped, inside = float(((v > hi) | (v < lo)).mean()), float(((v > lo) & (v < hi)).mean())
    print("%s r = %g %s: %d frames, %.3f of the components clamped, %.3f inside" % (fmt, r, "post shift" if shifted else "plain", twin.size, clamped, inside))
    assert clamped >= 0.05 and inside >= 0.50 and (v > hi).any() and (v < lo).any()
    want = oracle.from_cf32(twin, fmt).view(np.uint8)
    for what, sz in (("one call", []), ("three calls", sizes)):
        raw, counts, guard, kernel, info = run_device(gpu, pack_desc(r, shifted, fmt), x, sz)
        assert kernel == "k_front+k_interp" and int(info.num_halfband_stages) == m.S and int(info.arb_step) == m.step
        assert sum(counts) == twin.size and (not sz or counts == twin_counts)
        assert (guard == 0xA5).all(), (what, "a store behind the last frame")
        assert raw.size == want.size
        ne = raw != want
        assert not ne.any(), (fmt, what, int(ne.sum()), "first at frame %d" % (int(np.flatnonzero(ne)[0]) // bpf))


def measure_e_f(oracle):
    """E_f and bar of every dense case, of the long case and the worst E_f over the impulse runs, on the CPU"""
    rows = []
    for r in sorted(DENSE):
        m, x, want, e_f, bar = dense_case(oracle, r)
        rows.append(("dense r = %.9g (S = %d)" % (r, m.S), e_f, bar))
    m, x = long_input(oracle)
    want = numpy_msresamp_interp(m, x)
    rows.append(("long r = 47.9",) + bar_of(oracle, m, 47.9, x, want))
    for r in SEAM_RATIOS:
        m = design(oracle, r)
        worst = (0.0, 0.0)
        for what, n, sizes, p in seam_runs(m):
            x = impulse_input(n, p)
            worst = max(worst, bar_of(oracle, m, r, x, numpy_msresamp_interp(m, x)))
        rows.append(("impulses r = %g, worst" % r,) + worst)
    return rows


if __name__ == "__main__":
    from oracle import pyoracle
    pyoracle.build()
    for what, e_f, bar in measure_e_f(pyoracle):
        print("%-36s E_f = %.3g   bar = %.3g" % (what, e_f, bar))
