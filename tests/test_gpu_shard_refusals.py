"""Which seek family takes which chain: every entry point of the six seamless-sharding families (include/iqgpu.h: iqgpu_chain_seek*,
iqgpu_chain_dc_*, iqgpu_chain_dcagc_*, iqgpu_chain_dcrms_*, iqgpu_chain_measure) against every combination of DC blocker and output
AGC, and nothing but the refusal: the return code, and that the message of a refusal starts with the name of the entry point that
was called.

The chains are the smallest on which every family check can be reached -- cs16 in and out at 96 kS/s, pointwise (no resampler, no
filter: no check reads either) -- and no call moves more than 16384 frames.  A seek at frame 16384 comes with an empty preroll, so
it ends in the first refusal of its entry point, whichever that is: the family's check where the chain is not the family's, an
argument check behind it where it is.

EXPECTED is what the library answered before the family rules were gathered in one table (seek.cpp, shard_family); this file
passes on that library and on every one since.  OTHER_NAME lists the refusals whose message starts with another entry point's
name: recorded as they are, not endorsed."""
import functools

import numpy as np
import pytest

from shard_support import EINVAL, EUNSUPPORTED, OK

pytestmark = pytest.mark.gpu
BASE = dict(in_format="cs16", out_format="cs16", input_rate_hz=96e3, target_rate_hz=96e3, no_resample=True)
SHAPES = {
    "plain": dict(),
    "dc": dict(dc_block=True),
    "agc": dict(agc=True),
    "rms": dict(agc=True, agc_profile="local"),
    "dc_agc": dict(dc_block=True, agc=True),
    "dc_rms": dict(dc_block=True, agc=True, agc_profile="local"),
}
AT = 16384                  # the seek position behind frame 0, and the call grid where one is taken: one AGC chunk
EMPTY = np.empty(0, np.int16)


def zeros(frames):
    return np.zeros(2 * frames, np.int16)


def no_dc_rows():
    from iq_tool_amd.chain import DC_ROW
    return np.zeros(0, DC_ROW)


# name of the cell -> (Chain method, its arguments)
CALLS = {}
for _at in (0, AT):
    CALLS["seek@%d" % _at] = ("seek", lambda at=_at: (at, EMPTY))
    CALLS["seek_agc@%d" % _at] = ("seek_agc", lambda at=_at: (at, EMPTY))
    CALLS["seek_rms@%d" % _at] = ("seek_rms", lambda at=_at: (at, EMPTY))
    CALLS["seek_dc@%d" % _at] = ("seek_dc", lambda at=_at: (at, EMPTY, AT))
    CALLS["dcagc_seek@%d" % _at] = ("dcagc_seek", lambda at=_at: (at, EMPTY, AT))
    CALLS["dcrms_seek@%d" % _at] = ("dcrms_seek", lambda at=_at: (at, EMPTY, AT))
for _m in ("dc_measure", "dcagc_dc_measure", "dcrms_dc_measure"):
    CALLS[_m] = (_m, lambda: (0, zeros(1024)))
for _m in ("dc_advance", "dcagc_dc_advance", "dcrms_dc_advance"):
    CALLS[_m] = (_m, lambda: (None, no_dc_rows()))
for _m in ("measure", "dcagc_measure"):
    CALLS[_m] = (_m, lambda: (zeros(AT),))

# cell -> the code per chain, in SHAPES' order:  plain, dc, agc, rms, dc_agc, dc_rms
EXPECTED = {
    "seek@0": (OK, OK, OK, OK, OK, OK),
    "seek_agc@0": (EINVAL, EINVAL, OK, EUNSUPPORTED, OK, EUNSUPPORTED),
    "seek_rms@0": (EINVAL, EINVAL, EUNSUPPORTED, OK, EUNSUPPORTED, EUNSUPPORTED),
    "seek_dc@0": (EINVAL, OK, EINVAL, EINVAL, EUNSUPPORTED, EUNSUPPORTED),
    "dcagc_seek@0": (EINVAL, EINVAL, EINVAL, EINVAL, OK, EUNSUPPORTED),
    "dcrms_seek@0": (EINVAL, EINVAL, EINVAL, EINVAL, EUNSUPPORTED, OK),
    "seek@16384": (OK, EINVAL, EUNSUPPORTED, EUNSUPPORTED, EUNSUPPORTED, EUNSUPPORTED),
    "seek_agc@16384": (EINVAL, EINVAL, OK, EUNSUPPORTED, EINVAL, EUNSUPPORTED),
    "seek_rms@16384": (EINVAL, EINVAL, EUNSUPPORTED, EINVAL, EUNSUPPORTED, EUNSUPPORTED),
    "seek_dc@16384": (EINVAL, OK, EINVAL, EINVAL, EUNSUPPORTED, EUNSUPPORTED),
    "dcagc_seek@16384": (EINVAL, EINVAL, EINVAL, EINVAL, OK, EUNSUPPORTED),
    "dcrms_seek@16384": (EINVAL, EINVAL, EINVAL, EINVAL, EUNSUPPORTED, EINVAL),
    "dc_measure": (EINVAL, OK, EINVAL, EINVAL, EUNSUPPORTED, EUNSUPPORTED),
    "dcagc_dc_measure": (EINVAL, EINVAL, EINVAL, EINVAL, OK, EUNSUPPORTED),
    "dcrms_dc_measure": (EINVAL, EINVAL, EINVAL, EINVAL, EUNSUPPORTED, OK),
    "dc_advance": (EINVAL, OK, EINVAL, EINVAL, EUNSUPPORTED, EUNSUPPORTED),
    "dcagc_dc_advance": (EINVAL, EINVAL, EINVAL, EINVAL, OK, EUNSUPPORTED),
    "dcrms_dc_advance": (EINVAL, EINVAL, EINVAL, EINVAL, EUNSUPPORTED, OK),
    "measure": (EINVAL, EINVAL, OK, EUNSUPPORTED, OK, EUNSUPPORTED),
    "dcagc_measure": (EINVAL, EINVAL, EINVAL, EINVAL, OK, EUNSUPPORTED),
}
# (cell, chain) -> the entry point a refusal names where it is not the one called.  None today: the one message that names
# iqgpu_chain_seek whatever the family (the output AGC behind frame 0) is only reached through iqgpu_chain_seek itself
OTHER_NAME = {}


@functools.lru_cache(maxsize=None)
def chain(gpu, shape):
    return gpu.Chain(**dict(BASE, **SHAPES[shape]))


def observe(gpu, shape, cell):
    """(code, the name in front of the refusal's first colon or None)"""
    method, args = CALLS[cell]
    try:
        getattr(chain(gpu, shape), method)(*args())
    except gpu.IqgpuError as e:
        text = str(e).split("): ", 1)[1]
        print("%-18s %-7s %s" % (cell, shape, text))
        return e.code, text.split(":", 1)[0]
    return OK, None


def test_the_table_is_complete():
    assert set(EXPECTED) == set(CALLS) and all(len(row) == len(SHAPES) for row in EXPECTED.values())
    assert all(cell in CALLS and shape in SHAPES for cell, shape in OTHER_NAME)


@pytest.mark.parametrize("cell", sorted(CALLS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_refusal(gpu, shape, cell):
    code, name = observe(gpu, shape, cell)
    assert code in (OK, EINVAL, EUNSUPPORTED)
    assert code == EXPECTED[cell][list(SHAPES).index(shape)]
    if code != OK:
        assert name == OTHER_NAME.get((cell, shape), "iqgpu_chain_" + CALLS[cell][0])
