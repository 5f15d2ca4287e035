"""The oracle's msresamp for r >= 1 against the float64 model of tests/interp_model.py (CPU; runs anywhere).

The decimating msresamp has had an independent numpy formulation beside it since round 1 (tests/test_oracle.py,
_numpy_msresamp_decim, bar 3e-7); for r > 1 the oracle was checked for its output count and RMS only.  Here every shape of the
interpolating cascade (S = 0 .. 8) is held to the model at the same 3e-7: dense signals, any split into calls, and single impulses
whose responses show a delay that is one sample off, a swapped branch order or a polyphase window one sample late as an error of the
size of the signal."""
import math

import numpy as np
import pytest

from interp_model import ARB_TAPS, arb_count, impulse_support, numpy_msresamp_interp, stage_order
from iq_tool_amd import synth

BAR = 3e-7
# ratio -> (interp, S): r = 1 is not "> 1" (no interpolator, the plain arbitrary stage at step 2^24); 2.0 is not "> 2" (S = 0, rate_arb 2)
CASES = {1.0: (False, 0), 1.37: (True, 0), 1.999: (True, 0), 2.0: (True, 0), 3.3: (True, 1), 5.3: (True, 2), 47.9: (True, 5),
         100.0: (True, 6), 480.0: (True, 8)}
N = 4096
IMPULSE = 0.7 - 0.3j

_x = synth.complex_signal(N, 2.4e6, 61)
_x.setflags(write=False)


def make(oracle, r):
    m = oracle.MsResamp(np.float32(r))
    assert (m.interp, m.S) == CASES[r], (r, m.interp, m.S)
    return m


@pytest.mark.parametrize("r", sorted(CASES))
def test_oracle_matches_the_model_dense(oracle, r):
    m = make(oracle, r)
    want = numpy_msresamp_interp(m, _x)
    assert want.size == arb_count(N, m.step) << m.S == math.ceil((N << 24) / m.step) << m.S
    got = m.execute(_x)
    assert got.size == want.size
    err = float(np.abs(got - want).max())
    print("r = %g (S = %d, step %d): %d outputs, max |oracle - model| %.3g (bar %.0e), peak %.3f"
          % (r, m.S, m.step, got.size, err, BAR, float(np.abs(want).max())))
    assert float(np.abs(want).max()) > 0.5
    assert err <= BAR
    # the same stream in calls of 1, 2, 1000 and the rest
    m.reset()
    parts = np.concatenate([m.execute(_x[:1]), m.execute(_x[1:3]), m.execute(_x[3:1003]), m.execute(_x[1003:])])
    assert parts.size == want.size
    assert np.abs(parts - want).max() <= BAR
    assert np.array_equal(parts.view(np.float32), got.view(np.float32))


@pytest.mark.parametrize("pos", [0, 13, 14, 1000])
@pytest.mark.parametrize("r", sorted(CASES))
def test_oracle_matches_the_model_on_one_impulse(oracle, r, pos):
    m = make(oracle, r)
    x = np.zeros(N, np.complex64)
    x[pos] = IMPULSE
    want = numpy_msresamp_interp(m, x)
    got = m.execute(x)
    assert got.size == want.size
    err = float(np.abs(got - want).max())
    lo, hi = impulse_support(m, pos)
    print("r = %g, impulse at %d: response in outputs [%d, %d], max |oracle - model| %.3g" % (r, pos, lo, hi, err))
    assert err <= BAR
    # the response is where the structure says it is, in the model and in the oracle, and it is a response
    outside = np.ones(want.size, bool)
    outside[lo:hi + 1] = False
    assert not want[outside].any() and not got[outside].any()
    assert np.abs(want[lo:hi + 1]).max() > 0.3


def test_the_model_is_not_the_oracle_restated(oracle):
    """what the model is made of: the full prototype with its even taps, one lfilter per stage, stages lowest rate first"""
    m = make(oracle, 47.9)
    assert [m.stage_m(k) for k in stage_order(m)] == [3, 3, 3, 5, 10][::-1]          # the m = 10 stage runs FIRST when interpolating
    h = m.stage_taps(0)
    assert h.size == 4 * m.stage_m(0) + 1 and abs(h[2 * m.stage_m(0)] - 1.0) < 1e-6
    assert np.abs(h[0::2][np.arange(h[0::2].size) != m.stage_m(0)]).max() < 1e-7
    assert m.arb_proto().size == 256 * ARB_TAPS


def test_a_half_band_delay_off_by_one_is_seen(oracle):
    """the guard itself: the model with one stage's output a sample late misses the oracle by the size of the signal"""
    import scipy.signal as sps
    m = make(oracle, 5.3)
    got = m.execute(_x)

    def shifted_model(which):
        level = numpy_msresamp_interp(oracle.MsResamp(np.float32(1.325)), _x)        # the arbitrary stage of r = 5.3 alone
        for k in stage_order(m):
            mm = m.stage_m(k)
            h = m.stage_taps(k).astype(np.float64).copy()
            h[0::2] = 0.0
            h[2 * mm] = 1.0
            if k == which:
                h = np.concatenate([[0.0], h])                                      # one sample late
            z = np.zeros(2 * level.size, np.complex128)
            z[0::2] = level
            level = sps.lfilter(h, [1.0], z)
        return level

    assert oracle.MsResamp(np.float32(1.325)).step == m.step
    assert np.abs(got - shifted_model(None)).max() <= BAR
    for which in stage_order(m):
        assert np.abs(got - shifted_model(which)).max() > 1e-2
