"""A float64 model of msresamp for ratios r >= 1 (SPEC B.6), written the textbook way: an explicit gather for the arbitrary
polyphase stage, then, per half-band interpolator, zero-stuffing by two and ONE scipy.signal.lfilter with the stage's full
4m+1-tap prototype.  It takes an oracle.MsResamp for its DESIGN only (S, step, stage_m, stage_taps, arb_proto) and never calls its
execute(): the oracle (windows that slide, two branches per stage) and k_interp (levels rebuilt per tile in LDS) are both held to it.

numpy / scipy only; no device, no oracle code path.  Helpers for the tests that use it: the structural support of one input sample's
response, and k_interp's tile geometry restated from its law (iq_tool_amd/csrc/interp.hip, make_interp_geometry)."""
import numpy as np
import scipy.signal as sps

ARB_TAPS = 14          # taps per polyphase arm (resamp m = 7)
TILE = 2048            # final outputs per k_interp workgroup tile (kInterpTile)


def stage_order(m):
    """run order of the interpolators, lowest rate first, as indices into stage_m / stage_taps (whose index 0 is the stage at the
    HIGHEST rate: the run order of the decimator)"""
    return list(range(int(m.S) - 1, -1, -1))


def arb_count(n_in, step, phi0=0):
    """outputs of the arbitrary stage over n_in inputs: every k with P_k = phi0 + k step < n_in 2^24"""
    span = (int(n_in) << 24) - int(phi0)
    return max(0, -(-span // int(step)))


def numpy_msresamp_interp(m, x, phi0=0):
    """complex128 output of msresamp(r >= 1) over the whole stream x from a fresh state"""
    x = np.asarray(x).astype(np.complex128)
    step = int(m.step)
    # ---- arbitrary stage: P_k = phi0 + k step, q = P_k >> 24, arm = (P_k >> 16) & 255, 14 taps ending at x[q], zeros before the stream
    K = arb_count(x.size, step, phi0)
    P = np.uint64(phi0) + np.arange(K, dtype=np.uint64) * np.uint64(step)
    q = (P >> np.uint64(24)).astype(np.int64)
    arm = ((P >> np.uint64(16)) & np.uint64(255)).astype(np.int64)
    proto = m.arb_proto().astype(np.float64)
    xp = np.concatenate([np.zeros(ARB_TAPS - 1, np.complex128), x])
    level = np.zeros(K, np.complex128)
    for n in range(ARB_TAPS):
        level += proto[arm + 256 * n] * xp[q + (ARB_TAPS - 1) - n]
    # ---- half-band interpolators, lowest rate first
    for k in stage_order(m):
        mm = int(m.stage_m(k))
        h = m.stage_taps(k).astype(np.float64).copy()
        assert h.size == 4 * mm + 1
        h[0::2] = 0.0
        h[2 * mm] = 1.0                                    # centre tap exactly 1, the other even taps exactly 0
        z = np.zeros(2 * level.size, np.complex128)
        z[0::2] = level                                   # zero-stuff by two: z[2 i] = level[i]
        # y[u] = sum_j h[j] z[u - j].  z is zero at odd indices, so only j of u's parity contribute:
        #   u = 2 i     : j even -> only the centre j = 2 m:  y[2 i] = z[2 i - 2 m] = level[i - m]                    (delay branch)
        #   u = 2 i + 1 : j = 2 t + 1, t = 0 .. 2 m - 1:      y[2 i + 1] = sum_t h[2 t + 1] level[i - t]
        #                 = sum_t' h[4 m - 1 - 2 t'] level[i - 2 m + 1 + t']  (t' = 2 m - 1 - t), the 2 m-tap branch over
        #                 level[i - 2 m + 1 ..] of interp.hip's header, whose branch taps are the odd prototype taps reversed.
        # So the plain causal lfilter IS the stage: no extra delay, no advance, 2 outputs per input from the first input on.
        level = sps.lfilter(h, [1.0], z)
    return level


def impulse_support(m, p, phi0=0):
    """[lo, hi]: the final outputs that input sample p can reach, from the structure alone (which taps exist, not their values)"""
    step = int(m.step)
    # arbitrary stage: outputs k with p <= q_k <= p + 13, i.e. P_k in [p 2^24, (p + 14) 2^24)
    a = max(0, -(-((int(p) << 24) - int(phi0)) // step))
    b = -(-(((int(p) + ARB_TAPS) << 24) - int(phi0)) // step) - 1
    for k in stage_order(m):
        mm = int(m.stage_m(k))
        # even u = 2 i reads level[i - m]; odd u = 2 i + 1 reads level[i - 2 m + 1 .. i]
        a, b = 2 * a + 1, 2 * (b + 2 * mm - 1) + 1
    return a, b


def interp_geometry(m):
    """(ext, hist): ext[s] = samples of level s that k_interp rebuilds in front of a tile, and the input history it keeps from call
    to call -- make_interp_geometry's law restated: ext[S] = 0, ext[s] = ceil(ext[s + 1] / 2) + 2 m_s - 1 (m_s in run order),
    hist = ((ext[0] step) >> 24) + 1 + 14"""
    S = int(m.S)
    mm = [int(m.stage_m(k)) for k in stage_order(m)]
    ext = [0] * (S + 1)
    for s in range(S - 1, -1, -1):
        ext[s] = (ext[s + 1] + 1) // 2 + 2 * mm[s] - 1
    return ext, ((ext[0] * int(m.step)) >> 24) + 1 + ARB_TAPS


def first_input_reaching(m, j):
    """the last input sample p whose response STARTS at or before final output j (impulse_support(p)[0] <= j)"""
    S, step = int(m.S), int(m.step)
    # support start of p: k_a(p) = ceil(p 2^24 / step), then S times a -> 2 a + 1, i.e. lo = (k_a + 1) 2^S - 1
    k = (j + 1) // (1 << S) - 1                            # the largest k_a with lo <= j
    if k < 0:
        return None
    return (k * step) >> 24                                # the largest p with ceil(p 2^24 / step) <= k
