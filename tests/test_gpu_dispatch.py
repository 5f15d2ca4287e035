"""The launchers' dispatch, one case per VALUE of each axis (not the cross product): every step class of k_front_mid (six per
lane), of k_front_p0 and of k_front_fat, the formats a family accepts on either side, chains with the AGC, the cf32-out leaf,
the VARs of k_front_s1, (BPS, SPEC) of k_front_s2, (KT, BPF, S8) of k_cascade2, the transforms of k_fftconv16.

Each case runs 2^17 input frames in two calls -- both an edge run and a streaming run occur, and a mis-selected step class gives
wrong bytes at that length -- and asserts (a) the family iqgpu_chain_front_kernel reports, (b) the output against the same chain with the
family's opt-out switch.  The bar is the one tests/test_gpu_parity.py holds the pair to: equal bytes; for the radix-16 against the radix-4 transform no test compares the two
directly -- both are held to TOL against the oracle there, so 2 TOL against each other.

Rates: s = step / 2^24 = input_rate / (2^S target_rate), one s strictly inside each class bound of mid_class / p0_class / the fat classes.
Axes an existing test already launches and that are not repeated here: k_p0fft16 (LOG2N = 12 only, all three formats and four step
classes: test_resampler_and_filter_in_one_kernel_equal_the_two_kernel_path), run stealing and k_front_mid<8> (calls of 2^16 frames stay on k_front_s1 with mid8 set: 
test_mid_kernel_run_stealing_keeps_the_bytes, test_eight_per_lane_experiment_under_fixed_runs), M0 of k_front_s2 (the
stage lengths follow from the rate: its two-stage tests)."""
import numpy as np
import pytest

from iq_tool_amd import synth

pytestmark = pytest.mark.gpu

RATE = 2.4e6
N = 1 << 17
TOL = 1e-5
SWITCHES = ("FORCE_FAT", "FAT", "MID8", "NO_FAT", "NO_FAST", "NO_P0", "NO_S2", "NO_CASC2", "CASC2_MIN_RUN", "FFT_NO_R16", "FFT_LOG2N", "NO_MID_8BIT")


def hz(s, S=0):
    return RATE / (s * (1 << S))


def case(name, family, optout, env=None, bar="equal", **kw):
    kw.setdefault("in_format", "cs16"); kw.setdefault("out_format", "cs16")
    return pytest.param(family, dict(env or {}), optout, bar, dict(kw, input_rate_hz=RATE), id=name)


FF = dict(FORCE_FAT="1")          # (the size rule keeps calls this short on k_front_s1)
S1 = dict(NO_FAT="1")             # k_front_s1's own instantiations: k_front_mid / _fat / _p0 out of the way in both runs
CASES = [
    # ---- k_front_mid, six per lane: mid_class 1.5 <= s < 5/3 (l3 = 4), 5/3 <= s < 2 (l3 = 5); mixer or none; formats; AGC; cf32
    case("mid6-l3=4-nco", "k_front_mid<6,nco>", "NO_FAT", FF, target_rate_hz=hz(1.6, 1), shift_hz=200e3),
    case("mid6-l3=5-nonco", "k_front_mid<6,nonco>", "NO_FAT", FF, target_rate_hz=hz(1.8, 1)),
    # (a fresh chain's AGC is not locked yet: the front kernel hands cf32 to the AGC kernels -- the cf32 leaf with a mixer; the fused
    #  epilogue needs a locked AGC, seconds of signal: test_mid_kernel_random_schedules / test_p0_kernel_equals_the_sample_major_kernel with agc=True)
    case("mid6-agc-unlocked", "k_front_mid<6,nco,cf32>", "NO_FAT", FF, target_rate_hz=hz(1.6125, 1), shift_hz=200e3, agc=True),
    case("mid6-cf32", "k_front_mid<6,nonco,cf32>", "NO_FAT", FF, target_rate_hz=hz(1.7, 1), filters=(("lowpass", 200e3, 0.0),), out_format="cf32"),
    case("mid6-cu8-cs8", "k_front_mid<6,nco,8bit>", "NO_FAT", FF, target_rate_hz=hz(1.55, 1), shift_hz=-150e3, in_format="cu8", out_format="cs8"),
    case("mid6-cs8-cu8", "k_front_mid<6,nonco,8bit>", "NO_FAT", FF, target_rate_hz=hz(1.9, 1), in_format="cs8", out_format="cu8"),
    case("mid6-cs16-cu8", "k_front_mid<6,nonco,8bit>", "NO_FAT", FF, target_rate_hz=hz(1.6, 1), out_format="cu8"),
    case("mid6-sc16q11", "k_front_mid<6,nco,gain>", "NO_FAT", FF, target_rate_hz=hz(1.7, 1), shift_hz=100e3, in_format="sc16q11"),
    case("mid6-gain", "k_front_mid<6,nonco,gain>", "NO_FAT", FF, target_rate_hz=hz(1.6, 1), gain=0.5),
    # ---- k_front_fat: the same three classes
    case("fat-4-6", "k_front_fat", "NO_FAT", dict(FF, FAT="1"), target_rate_hz=hz(1.63, 1), shift_hz=200e3),
    case("fat-5-6", "k_front_fat", "NO_FAT", dict(FF, FAT="1"), target_rate_hz=hz(1.7, 1)),
    case("fat-5-7", "k_front_fat", "NO_FAT", dict(FF, FAT="1"), target_rate_hz=hz(1.85, 1), shift_hz=200e3),
    # ---- k_front_p0: p0_class (l2, l3, l4) = (2,3,4) s < 1.25, (2,3,5) < 4/3, (2,4,5) < 1.5, (3,4,6) < 5/3, (3,5,6) < 1.75, (3,5,7) < 2
    case("p0-2-3-4-cs8-cs16", "k_front_p0", "NO_P0", FF, target_rate_hz=hz(1.1), in_format="cs8"),
    case("p0-2-3-5-cs16-cs16", "k_front_p0", "NO_P0", FF, target_rate_hz=hz(1.29)),
    case("p0-2-4-5-cu8-cu8", "k_front_p0", "NO_P0", FF, target_rate_hz=hz(1.4), in_format="cu8", out_format="cu8"),
    case("p0-3-4-6-cu8-cs8", "k_front_p0", "NO_P0", FF, target_rate_hz=hz(1.62), in_format="cu8", out_format="cs8"),
    case("p0-3-5-6-cs16-cu8", "k_front_p0", "NO_P0", FF, target_rate_hz=hz(1.7), out_format="cu8"),
    case("p0-3-5-7-cf32", "k_front_p0", "NO_P0", FF, target_rate_hz=hz(1.85), in_format="cu8", out_format="cf32", filters=(("lowpass", 300e3, 0.0),)),
    case("p0-agc", "k_front_p0", "NO_P0", FF, target_rate_hz=hz(1.6125), in_format="cu8", out_format="cu8", agc=True),
    # ---- k_front_s1: VAR against the run-time-switched instantiation (no_fast)
    case("s1-fast", "k_front_s1", "NO_FAST", S1, target_rate_hz=hz(1.6125, 1), shift_hz=200e3),
    case("s1-var1", "k_front_s1", "NO_FAST", S1, target_rate_hz=hz(1.6125, 1)),
    case("s1-var2", "k_front_s1", "NO_FAST", S1, target_rate_hz=hz(1.6125), in_format="cu8", out_format="cu8"),
    case("s1-var3", "k_front_s1", "NO_FAST", S1, target_rate_hz=hz(1.6125), out_format="cu8"),
    case("s1-var4", "k_cascade+k_front_s1", "NO_FAST", dict(NO_CASC2="1"), target_rate_hz=hz(1.6125, 3), shift_hz=50e3),
    case("s1-var5", "k_front_s1", "NO_FAST", S1, target_rate_hz=hz(1.6125, 1), shift_hz=200e3, dc_block=True),
    case("s1-var6", "k_front_s1", "NO_FAST", S1, target_rate_hz=hz(1.6125, 1), dc_block=True),
    case("s1-var7", "k_front_s1", "NO_FAST", S1, target_rate_hz=hz(1.6125), shift_hz=200e3, in_format="cu8", out_format="cu8"),
    case("s1-var8", "k_front_s1", "NO_FAST", S1, target_rate_hz=hz(1.6125), shift_hz=200e3, in_format="cu8", out_format="cu8", dc_block=True),
    case("s1-var9", "k_front_s1", "NO_FAST", S1, target_rate_hz=hz(1.6125), in_format="cu8", out_format="cu8", dc_block=True),
    case("s1-var2-agc", "k_front_s1", "NO_FAST", S1, target_rate_hz=hz(1.6125), in_format="cu8", out_format="cu8", agc=True),
    # ---- k_front_s2: BPS 2 / 4 / 8, SPEC 0 (cs8: no switch set of its own) and some of 1 .. 7
    case("s2-cs8-spec0", "k_front_s2", "NO_S2", target_rate_hz=hz(1.6125, 2), in_format="cs8"),
    case("s2-cs16-spec2", "k_front_s2", "NO_S2", target_rate_hz=hz(1.6125, 2)),
    case("s2-cs16-spec3", "k_front_s2", "NO_S2", target_rate_hz=hz(1.7, 2), shift_hz=100e3),
    case("s2-cu8-spec6", "k_front_s2", "NO_S2", target_rate_hz=hz(1.6125, 2), in_format="cu8", out_format="cu8"),
    case("s2-cu8-spec7", "k_front_s2", "NO_S2", target_rate_hz=hz(1.85, 2), shift_hz=-100e3, in_format="cu8", out_format="cu8"),
    case("s2-cs16-spec4", "k_front_s2", "NO_S2", target_rate_hz=hz(1.6125, 2), out_format="cf32", filters=(("lowpass", 100e3, 0.0),)),
    case("s2-cf32-in", "k_front_s2", "NO_S2", target_rate_hz=hz(1.6125, 2), in_format="cf32"),
    # ---- k_cascade2: KT = 2, 3, 4 with cu8, cs8 (S8), cs16 (BPF 4); fixed runs of eight tiles (block_samples): a call this short
    #      dealt out over every wave slot has one-tile runs, which stay on k_cascade
    case("casc2-K2-cu8", "k_cascade2+k_front_s1", "NO_CASC2", dict(CASC2_MIN_RUN="2"), block_samples=65536, target_rate_hz=hz(1.6125, 3), in_format="cu8"),
    case("casc2-K3-cs8", "k_cascade2+k_front_s1", "NO_CASC2", dict(CASC2_MIN_RUN="2"), block_samples=65536, target_rate_hz=hz(1.6125, 4), in_format="cs8"),
    case("casc2-K4-cs16", "k_cascade2+k_front_s1", "NO_CASC2", dict(CASC2_MIN_RUN="2"), block_samples=65536, target_rate_hz=hz(1.6125, 5)),
] + [
    # ---- k_fftconv16: N = 2^10 .. 2^14 against the radix-4 kernel at the same N (2^14: at 2^13, the radix-4 kernel's longest)
    case("fft16-N=2^%d" % lg, "k_front_s1", "FFT_NO_R16", dict(FFT_LOG2N=str(lg)), bar="2tol", out_format="cf32", target_rate_hz=hz(1.6125, 1),
         filters=(("lowpass", 200e3, 0.0),), filter_taps=301) for lg in (10, 11, 12, 13, 14)
]


@pytest.mark.parametrize("family,env,optout,bar,kw", CASES)
def test_dispatch_axis(gpu, monkeypatch, family, env, optout, bar, kw):
    raw = synth.raw_stream(N, RATE, 7, kw["in_format"])
    per = raw.size // N

    def run(extra):
        for k in SWITCHES:
            monkeypatch.delenv("IQGPU_" + k, raising=False)
        for k, v in dict(env, **extra).items():
            monkeypatch.setenv("IQGPU_" + k, v)
        ch = gpu.Chain(**kw)
        outs, names = [], []
        for h in (0, 1):
            outs.append(ch.process(raw[per * h * (N // 2):per * (h + 1) * (N // 2)])); names.append(ch.front_kernel())
        return np.concatenate(outs), names

    got, names = run({})
    ref_extra = {optout: "1"}
    if optout == "FFT_NO_R16" and env.get("FFT_LOG2N") == "14":
        ref_extra["FFT_LOG2N"] = "13"
    ref, ref_names = run(ref_extra)
    for k in SWITCHES:
        monkeypatch.delenv("IQGPU_" + k, raising=False)
    print(family, names, ref_names, got.size)
    assert names == [family, family], names
    if optout not in ("NO_FAST", "FFT_NO_R16"):
        assert all(nm != family for nm in ref_names), ref_names       # (no_fast and the transform switch leave the family's name)
    assert got.size == ref.size and got.size > 0
    if bar == "equal":
        assert np.array_equal(got, ref), (int((got != ref).sum()), int(np.flatnonzero(got != ref)[0]))
    else:
        assert np.abs(got.view(np.float32) - ref.view(np.float32)).max() <= 2 * TOL
