"""I/Q calibration on the device (include/iqgpu.h "I/Q calibration"; iq_calib.hip): k_iq_metric against the host metric for every
(block, candidate), its determinism, k_iq_blocks against the streaming probe bit for bit, the trace of Chain.calibrate_iq against the
host metric, the handle it must leave untouched, and iqgpu_run --iq-calibrate.

Bars.  Metric and power range: the project's 2e-4 * max(1, |ref|), the bar test_iq_optimizer.py holds between host, oracle and
float64.  It is asserted only where the gate decision is unambiguous: no compared bin pair has max(p_pos, p_neg) within 0.1 dB of
-80 dB in the numpy spectra (a float transform's error is ~1e-6 of the block's peak bin, 0.02 dB for a bin 70 dB below it).  Trace:
host_total[pick] >= (1 - 4e-4) max(host_total) -- two evaluators that each hold 2e-4 can only disagree on an argmax between
candidates closer than that.  Everything else is bit for bit.

The -80 dB gate itself is held to the host on inputs of two kinds: "open" blocks, every bin pair above the gate, and "gated" blocks,
451 of the 461 pairs clearly below it and the rest clearly above (asserted from the numpy spectra) -- in the metric comparison, in the
trace and in the mix of blocks with and without enough peak-to-average power.

Shapes are the smallest that reach every path: 1 .. 17 blocks, 1 candidate .. one more than a launch holds, strides 1024, 1024 + 4
and 4096.  Every comparison prints its figure before it asserts (pytest -s)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from test_iq_calibrate_host import (BAR, HI, LO, N, TONES, flat_noise, imbalanced_block, np_power_range, np_spectra)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "iq_tool_amd", "lib", "iqgpu_run")
RATE = 2.4e6
MAX_BLOCKS = 17
# the blocks of the metric comparison: the tones of imbalanced_block under noise strong enough to keep every bin well above the -80 dB
# gate (floor ~ -54 dB), each with its own imbalance
METRIC_NOISE = 0.1


def metric_block(b):
    return imbalanced_block(400 + b, gain_err=0.01 * (b % 5), phase_err=0.008 * (b % 3) - 0.01, noise=METRIC_NOISE)


# ... and the blocks on which the gate CLOSES: most bin pairs lie clearly below -80 dB and the rest clearly above, so that a kernel
# without the gate, with `and` for `or`, or with another threshold misses the host metric by far more than the bar.  Noise 1e-4 puts
# the floor near -114 dB, and the tones of imbalanced_block at 1 % amplitude reach above -80 dB with their main lobes only: 451 of the
# 461 pairs are closed, the open ones pair a tone's lobe with its image or the floor.  (Tones at full amplitude on bin centres close
# as many pairs, but there the host's float transform itself stands 4.5e-4 from the float64 formulation -- measured on the CPU: the
# floor under a strong tone is at the transform's rounding -- and the images sweep through -80 dB as a search closes in.)
GATED_NOISE = 1e-4
FAINT_TONES = tuple((f, 0.01 * a) for f, a in TONES)


def gated_block(seed):
    return imbalanced_block(seed, tones=FAINT_TONES, noise=GATED_NOISE)


def closed_pairs(blocks, used, cands):
    """the fewest bin pairs with max(p_pos, p_neg) <= -80 dB -- pairs the gate drops -- of any (block, candidate), numpy spectra"""
    idx = np.arange(LO, HI)
    fewest = HI - LO
    for b in used:
        S = np_spectra(blocks[b], cands["mag"], cands["phase"])
        fewest = min(fewest, int((np.maximum(S[:, idx], S[:, N - 1 - idx]) <= -80.0).sum(axis=1).min()))
    return fewest


@pytest.fixture(scope="module")
def geometry(gpu):
    from iq_tool_amd import iq_optimizer
    per_launch, tile = iq_optimizer.metric_geometry()
    assert per_launch >= 225 and 1 < tile < 81
    return per_launch, tile


@pytest.fixture(scope="module", params=["open", "gated"])
def reference(request, gpu, geometry):
    """17 blocks, one more candidate than a launch holds, the HOST metric of every pair and the host's power range of every block:
    computed once per set of blocks, read only.  "open": every bin pair above the gate; "gated": most of them below it"""
    from iq_tool_amd import iq_optimizer
    per_launch, _ = geometry
    if request.param == "open":
        blocks = np.stack([metric_block(b) for b in range(MAX_BLOCKS)])
    else:
        blocks = np.stack([gated_block(600 + b) for b in range(MAX_BLOCKS)])
    rng = np.random.default_rng(5)
    cands = np.zeros(per_launch + 1, iq_optimizer.IQ_CAND)
    cands["mag"][1:] = rng.uniform(-0.1, 0.1, per_launch).astype(np.float32)
    cands["phase"][1:] = rng.uniform(-0.1, 0.1, per_launch).astype(np.float32)
    # the precondition: no compared bin pair at the gate, under any candidate
    margin = gate_margin(blocks, range(MAX_BLOCKS), cands)
    closed = closed_pairs(blocks, range(MAX_BLOCKS), cands)
    print("%s blocks: nearest bin pair to the -80 dB gate %.3f dB; at least %d of %d pairs closed" % (request.param, margin, closed, HI - LO))
    assert margin > 0.1
    assert closed >= 400 if request.param == "gated" else closed == 0
    o = gpu.IqOptimizer(seed=1)
    want = np.array([[o.metric(blk, float(c["mag"]), float(c["phase"])) for c in cands] for blk in blocks], np.float32)
    pr = np.empty(MAX_BLOCKS, np.float32)
    for b, blk in enumerate(blocks):
        o.run_optimization(blk, 10.0 * (b + 1))            # (estimate_power runs in front of the power gate)
        pr[b] = o.stats()["power_range_db"]
    for a in (blocks, cands, want, pr):
        a.setflags(write=False)
    return blocks, cands, want, pr


def strided(blocks, stride):
    """block b at b * stride of a flat array; NaN between the blocks: a stray read shows"""
    flat = np.full((len(blocks) - 1) * stride + N, np.nan + 1j * np.nan, np.complex64)
    for b, blk in enumerate(blocks):
        flat[b * stride:b * stride + N] = blk
    return flat


# --------------------------------------------------------------------------------------------
# 5. k_iq_metric against the host metric
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_blocks", [1, 2, 5, 17])
def test_metric_batch_against_host_metric(gpu, geometry, reference, n_blocks):
    from iq_tool_amd import iq_optimizer
    per_launch, tile = geometry
    blocks, cands, want, pr = reference
    odd = 2 * tile + 5                                       # no multiple of the candidate tile
    assert odd % tile and 81 % tile and odd < per_launch
    worst = 0.0
    for stride in (N, N + 4, 4096):
        flat = strided(blocks[:n_blocks], stride)
        for n_cand in (1, 81, per_launch + 1, odd):
            got, got_pr = iq_optimizer.metric_batch(flat, cands[:n_cand], stride=stride, power=True)
            assert got.shape == (n_blocks, n_cand)
            ref = want[:n_blocks, :n_cand]
            rel = float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max())
            worst = max(worst, rel)
            assert np.isfinite(got).all() and rel <= BAR, (stride, n_cand, rel)
            rel_pr = float((np.abs(got_pr - pr[:n_blocks]) / np.maximum(1.0, np.abs(pr[:n_blocks]))).max())
            assert rel_pr <= BAR, (stride, n_cand, rel_pr)
    print("n_blocks %d: worst |metric - host| / max(1, |host|) = %.3g (bar %.3g)" % (n_blocks, worst, BAR))


# --------------------------------------------------------------------------------------------
# 6. determinism: the same bits on every call and from both forms
# --------------------------------------------------------------------------------------------
def test_metric_batch_is_deterministic_and_device_form_equals_host_form(gpu, geometry, reference):
    from iq_tool_amd import iq_optimizer
    per_launch, _ = geometry
    blocks, cands, _, _ = reference
    stride = N + 4
    flat = strided(blocks, stride)
    a, pa = iq_optimizer.metric_batch(flat, cands, stride=stride, power=True)
    b, pb = iq_optimizer.metric_batch(flat, cands, stride=stride, power=True)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(pa.view(np.uint32), pb.view(np.uint32))
    d = gpu.DeviceBuffer(flat.nbytes)
    d.upload(flat)
    c, pc = iq_optimizer.metric_batch_device(d.ptr, len(blocks), cands, stride=stride, power=True)
    assert np.array_equal(a.view(np.uint32), c.view(np.uint32)) and np.array_equal(pa.view(np.uint32), pc.view(np.uint32))
    # a candidate's metric does not depend on the list it stands in (its tile, its launch)
    one = iq_optimizer.metric_batch_device(d.ptr, len(blocks), cands[per_launch:per_launch + 1], stride=stride)
    assert np.array_equal(one[:, 0].view(np.uint32), a[:, per_launch].view(np.uint32))
    d.free()
    # refusals
    for kw in (dict(stride=N - 1), ):
        with pytest.raises(gpu.IqgpuError):
            iq_optimizer.metric_batch(flat, cands, **kw)
    with pytest.raises(gpu.IqgpuError):
        iq_optimizer.metric_batch(flat, cands[:0], stride=stride)


# --------------------------------------------------------------------------------------------
# 7. k_iq_blocks against the streaming probe, bit for bit
# --------------------------------------------------------------------------------------------
FRAMES = 5200            # 5 whole blocks; max_blocks 3 -> blocks at 0, 1733, 3466
BPF = dict(cu8=2, cs16=4, sc16q11=4, cf32=8)


def raw_of(fmt, seed=31):
    from iq_tool_amd import synth
    return np.ascontiguousarray(synth.raw_stream(FRAMES, RATE, seed, fmt)).view(np.uint8).reshape(-1)


def probe_head(gpu, fmt, raw_from, **kw):
    """the probe block of a FRESH chain whose first call starts there: I/Q correction off, no shift, probe on"""
    ch = gpu.Chain(in_format=fmt, out_format="cf32", input_rate_hz=RATE, target_rate_hz=744187.5, **kw)
    ch.enable_iq_probe()
    ch.process(raw_from)
    blk = ch.read_iq_probe()
    assert blk is not None
    ch.close()
    return blk


@pytest.mark.parametrize("dc", [False, True])
@pytest.mark.parametrize("gain", [1.0, 0.37])
@pytest.mark.parametrize("fmt", ["cu8", "cs16", "sc16q11", "cf32"])
def test_gathered_blocks_equal_the_probe_of_a_fresh_chain(gpu, fmt, gain, dc):
    raw = raw_of(fmt)
    bpf = BPF[fmt]
    # the calibrating chain has a shift and I/Q correction on: neither reaches its blocks
    ch = gpu.Chain(in_format=fmt, out_format="cf32", input_rate_hz=RATE, target_rate_hz=744187.5, gain=gain, dc_block=dc,
                   shift_hz=0.21 * RATE, iq_correct=True, iq_mag=0.05, iq_phase=-0.05)
    got = ch.calibrate_iq_blocks(raw, max_blocks=3)
    assert got.shape == (3, N)
    stride = max(N, FRAMES // 3)
    for b in range(3):
        want = probe_head(gpu, fmt, raw[b * stride * bpf:], gain=gain, dc_block=dc)
        assert np.array_equal(got[b].view(np.uint32), want.view(np.uint32)), (fmt, gain, dc, b)
    # more blocks than the input holds: all five whole ones, back to back
    assert ch.calibrate_iq_blocks(raw, max_blocks=64).shape == (5, N)
    with pytest.raises(gpu.IqgpuError):
        ch.calibrate_iq_blocks(raw[:1023 * bpf])


@pytest.mark.parametrize("fmt", ["cu8", "cs16", "sc16q11", "cf32"])
def test_gathered_blocks_from_a_device_address_one_frame_off(gpu, fmt):
    raw = raw_of(fmt)
    bpf = BPF[fmt]
    ch = gpu.Chain(in_format=fmt, out_format="cf32", input_rate_hz=RATE, target_rate_hz=744187.5, gain=0.37, dc_block=True)
    d = gpu.DeviceBuffer(raw.nbytes)
    d.upload(raw)
    got = ch.calibrate_iq_blocks_device(d.ptr + bpf, FRAMES - 1, max_blocks=3)
    stride = max(N, (FRAMES - 1) // 3)
    for b in range(3):
        want = probe_head(gpu, fmt, raw[(1 + b * stride) * bpf:], gain=0.37, dc_block=True)
        assert np.array_equal(got[b].view(np.uint32), want.view(np.uint32)), (fmt, b)
    host = ch.calibrate_iq_blocks(raw[bpf:], max_blocks=3)
    assert np.array_equal(host.view(np.uint32), got.view(np.uint32))
    d.free()


# --------------------------------------------------------------------------------------------
# 8. the trace of Chain.calibrate_iq, path-independent
# --------------------------------------------------------------------------------------------
GATED_SEED = 700
TRACE_NOISE = 0.05      # floor ~ -60 dB: the image of the imbalance (-45 dB) stands above it, and no bin pair comes near the gate


def imbalanced_stream(n_blocks, seed=500, noise=TRACE_NOISE):
    """n_blocks imbalanced blocks back to back as cs16 bytes"""
    from iq_tool_amd import synth
    x = np.concatenate([imbalanced_block(seed + b, noise=noise) for b in range(n_blocks)])
    return np.ascontiguousarray(synth.quantise(x, "cs16")).view(np.uint8).reshape(-1)


def gated_stream(n_blocks, seed=GATED_SEED):
    """n_blocks gated blocks back to back as cs16 bytes"""
    from iq_tool_amd import synth
    x = np.concatenate([gated_block(seed + b) for b in range(n_blocks)])
    return np.ascontiguousarray(synth.quantise(x, "cs16")).view(np.uint8).reshape(-1)


def host_totals(o, blocks, used, cands):
    """(totals, bars): the host metric summed over the blocks that count -- block order, in double -- and the project's bar summed alike"""
    t, bars = np.zeros(len(cands)), np.zeros(len(cands))
    for b in used:
        m = np.array([o.metric(blocks[b], float(c["mag"]), float(c["phase"])) for c in cands], np.float64)
        t += m
        bars += BAR * np.maximum(1.0, np.abs(m))
    return t, bars


def gate_margin(blocks, used, cands):
    """dB between the -80 dB gate and the nearest max(p_pos, p_neg) of any compared bin pair, numpy spectra"""
    idx = np.arange(LO, HI)
    margin = np.inf
    for b in used:
        S = np_spectra(blocks[b], cands["mag"], cands["phase"])
        margin = min(margin, float(np.abs(np.maximum(S[:, idx], S[:, N - 1 - idx]) + 80.0).min()))
    return margin


def check_trace(gpu, got, blocks, gated=False):
    """every level of the report under the HOST metric on the same blocks; gated: the input must close the -80 dB gate on many pairs"""
    from iq_tool_amd import iq_optimizer
    o = gpu.IqOptimizer(seed=1)
    used = []
    for b, blk in enumerate(blocks):
        o.run_optimization(blk, 10.0 * (b + 1))
        if o.stats()["power_range_db"] >= 20.0:
            used.append(b)
    assert got.found and got.blocks_taken == len(blocks) and got.blocks_used == len(used)
    assert len(got.levels) == 5 and got.evaluations == 5 * 81
    cm, cp = np.float32(0.0), np.float32(0.0)
    for k, lv in enumerate(got.levels):
        assert (np.float32(lv["center_mag"]), np.float32(lv["center_phase"])) == (cm, cp)
        cands = iq_optimizer.level_grid(lv["center_mag"], lv["center_phase"], lv["step"], 9)
        margin = gate_margin(blocks, used, cands)
        assert margin > 0.1, "level %d: a compared bin pair stands %.3f dB from the gate: the bars below do not apply to this input" % (k, margin)
        if gated:
            assert closed_pairs(blocks, used, cands) >= 400
        t, bars = host_totals(o, blocks, used, cands)
        print("level %d: step %.3g pick %d host total at pick %.9g, host max %.9g, device total %.9g" % (
            k, lv["step"], lv["pick"], t[lv["pick"]], t.max(), lv["total_at_pick"]))
        assert t[lv["pick"]] >= (1.0 - 4e-4) * t.max()
        assert abs(lv["total_at_pick"] - t[lv["pick"]]) <= bars[lv["pick"]]
        cm, cp = cands[lv["pick"]]["mag"], cands[lv["pick"]]["phase"]
    assert (np.float32(got.mag), np.float32(got.phase)) == (cm, cp)             # centre + offset(pick) of the last level, in float
    assert got.total_at_best > got.total_at_center0
    assert got.total_at_best == got.levels[-1]["total_at_pick"]


def test_calibrate_trace_holds_under_the_host_metric(gpu):
    raw = imbalanced_stream(8)
    ch = gpu.Chain(in_format="cs16", out_format="cs16", input_rate_hz=RATE, target_rate_hz=744187.5)
    got = ch.calibrate_iq(raw)
    blocks = ch.calibrate_iq_blocks(raw)
    assert blocks.shape == (8, N)
    check_trace(gpu, got, blocks)
    # ... and on blocks whose bin pairs mostly lie below the -80 dB gate: the reference's gate decides the totals
    rawg = gated_stream(8)
    check_trace(gpu, ch.calibrate_iq(rawg), ch.calibrate_iq_blocks(rawg), gated=True)
    # the device form: the same report
    d = gpu.DeviceBuffer(raw.nbytes)
    d.upload(raw)
    again = ch.calibrate_iq_device(d.ptr, raw.nbytes // 4)
    d.free()
    assert again.levels == got.levels and again.factors == got.factors
    # a subset of the blocks: max_blocks 3 of 8 -> blocks 0, 2 (2730 frames on), ...: the selection rule of the header
    few = ch.calibrate_iq(raw, max_blocks=3)
    assert few.blocks_taken == 3 and few.found
    stride = 8 * N // 3
    fb = ch.calibrate_iq_blocks(raw, max_blocks=3)
    cf = ch.calibrate_iq_blocks(raw[stride * 4:], max_blocks=1)
    assert np.array_equal(fb[1], cf[0])


def test_calibrate_gate_and_refusals(gpu):
    from iq_tool_amd import synth
    ch = gpu.Chain(in_format="cs16", out_format="cs16", input_rate_hz=RATE, target_rate_hz=744187.5)
    flat = np.concatenate([flat_noise(s) for s in range(4)])
    assert all(np_power_range(flat[b * N:(b + 1) * N]) < 19.0 for b in range(4))
    raw = np.ascontiguousarray(synth.quantise(flat, "cs16")).view(np.uint8).reshape(-1)
    none = ch.calibrate_iq(raw, center_mag=0.01, center_phase=-0.02)
    assert not none.found and none.blocks_used == 0 and none.blocks_taken == 4 and none.levels == []
    assert (np.float32(none.mag), np.float32(none.phase)) == (np.float32(0.01), np.float32(-0.02))
    # gated and ungated blocks: only the ungated count
    # (the ungated ones close the -80 dB gate on most bin pairs; every level is held to the HOST metric over them alone)
    mixed = np.concatenate([flat[:N], gated_block(GATED_SEED), flat[N:2 * N], gated_block(GATED_SEED + 1)])
    rawm = np.ascontiguousarray(synth.quantise(mixed, "cs16")).view(np.uint8).reshape(-1)
    got = ch.calibrate_iq(rawm)
    assert got.found and got.blocks_taken == 4 and got.blocks_used == 2
    check_trace(gpu, got, ch.calibrate_iq_blocks(rawm), gated=True)
    only = ch.calibrate_iq(np.concatenate([rawm[N * 4:2 * N * 4], rawm[3 * N * 4:]]))
    assert only.blocks_used == 2 and only.levels == got.levels and only.factors == got.factors
    for kw in (dict(grid=8), dict(grid=17), dict(span=0.0), dict(min_step=float("nan")), dict(max_blocks=0)):
        with pytest.raises(gpu.IqgpuError):
            ch.calibrate_iq(rawm, **kw)
    with pytest.raises(gpu.IqgpuError):
        ch.calibrate_iq(rawm[:1023 * 4])


# --------------------------------------------------------------------------------------------
# 9. the handle is untouched
# --------------------------------------------------------------------------------------------
def test_calibrate_leaves_the_handle_as_it_was(gpu):
    from iq_tool_amd import synth
    n = 1 << 15
    raw = np.ascontiguousarray(synth.raw_stream(2 * n, RATE, 9, "cs16")).view(np.uint8).reshape(-1)
    kw = dict(in_format="cs16", out_format="cs16", input_rate_hz=RATE, target_rate_hz=744187.5, dc_block=True, agc=True,
              agc_profile="digital", iq_correct=True, iq_mag=0.01, iq_phase=-0.02)
    a, twin = gpu.Chain(**kw), gpu.Chain(**kw)
    for ch in (a, twin):
        ch.enable_iq_probe()
    first = a.process(raw[:n * 4])
    assert np.array_equal(first, twin.process(raw[:n * 4]))          # (a block is staged in both, unread)
    before = (a.tell(), a.save_state(), bytes(a.agc_state_raw()), a.dc_state().tobytes())
    got = a.calibrate_iq(imbalanced_stream(4))
    assert got.found
    a.calibrate_iq_blocks(raw)
    after = (a.tell(), a.save_state(), bytes(a.agc_state_raw()), a.dc_state().tobytes())
    assert before == after
    assert before == (twin.tell(), twin.save_state(), bytes(twin.agc_state_raw()), twin.dc_state().tobytes())
    pa, pt = a.read_iq_probe(), twin.read_iq_probe()
    assert pa is not None and np.array_equal(pa.view(np.uint32), pt.view(np.uint32))
    assert np.array_equal(a.process(raw[n * 4:]), twin.process(raw[n * 4:]))
    assert a.tell() == twin.tell() and a.save_state() == twin.save_state()


# --------------------------------------------------------------------------------------------
# 10. iqgpu_run --iq-calibrate
# --------------------------------------------------------------------------------------------
def test_harness_calibrates_on_the_head_and_installs_the_factors(gpu, tmp_path):
    from iq_tool_amd import synth
    frames = 1 << 20
    n = np.arange(frames)
    x = sum(a * np.exp(2j * np.pi * f * n) for f, a in ((0.11, 0.5), (-0.23, 0.2), (0.31, 0.1)))
    x = x + 1e-3 * (np.random.default_rng(3).standard_normal(frames) + 1j * np.random.default_rng(4).standard_normal(frames))
    y = (x.real + 1j * (1.04 * (x.imag * np.cos(0.03) + x.real * np.sin(0.03)))).astype(np.complex64)
    raw = np.ascontiguousarray(synth.quantise(y, "cs16"))
    src = tmp_path / "in.cs16"
    raw.tofile(src)
    base = [EXE, "-i", str(src), "--raw-file-input-rate", "2400000", "--raw-file-input-sample-format", "cs16", "--output-rate", "744187.5",
            "--output-sample-format", "cs16", "--chunk-frames", "262144", "--quiet"]
    out1, out2 = tmp_path / "cal.cs16", tmp_path / "fac.cs16"
    p = subprocess.run(base + ["-o", str(out1), "--iq-calibrate"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    m = re.search(r"--iq-factors (\S+):(\S+)", p.stdout)
    assert m, p.stdout
    ch = gpu.Chain(in_format="cs16", out_format="cs16", input_rate_hz=RATE, target_rate_hz=744187.5)
    want = ch.calibrate_iq(raw.view(np.uint8).reshape(-1))
    assert want.found and want.blocks_taken == 64
    assert (np.float32(float(m.group(1))), np.float32(float(m.group(2)))) == (np.float32(want.mag), np.float32(want.phase))
    p2 = subprocess.run(base + ["-o", str(out2), "--iq-factors", "%s:%s" % (m.group(1), m.group(2))], capture_output=True, text=True, timeout=120)
    assert p2.returncode == 0, p2.stderr
    a, b = np.fromfile(out1, np.int16), np.fromfile(out2, np.int16)
    assert a.size == b.size > 0 and np.array_equal(a, b)
    # and the factors did something: the file differs from the uncorrected one
    out3 = tmp_path / "plain.cs16"
    assert subprocess.run(base + ["-o", str(out3)], capture_output=True, text=True, timeout=120).returncode == 0
    assert not np.array_equal(a, np.fromfile(out3, np.int16))
    both = subprocess.run(base + ["-o", str(out2), "--iq-calibrate", "--iq-factors", "0.01:0.02"], capture_output=True, text=True, timeout=120)
    assert both.returncode == 2 and "excludes" in both.stderr
    assert "no block" not in p.stderr
    # a head without 20 dB of peak-to-average power: the centre stands, and the harness says so
    flat = tmp_path / "flat.cs16"
    np.ascontiguousarray(synth.quantise(np.concatenate([flat_noise(s) for s in range(8)]), "cs16")).tofile(flat)
    q = subprocess.run([EXE, "-i", str(flat)] + base[3:] + ["-o", str(out2), "--iq-calibrate"], capture_output=True, text=True, timeout=120)
    assert q.returncode == 0 and "--iq-factors 0:0 found=0" in q.stdout and "no block" in q.stderr, (q.stdout, q.stderr)
