"""Capture statistics of a stream on the device (include/iqgpu.h "capture statistics"): counts, rails, extrema, the peak, an amplitude
histogram and the first two moments of one stream of frames in one sample format, independent of any chain.  The result is a function
of the pushed frames alone, bit for bit, however the stream was cut into pushes; results of consecutive streams merge exactly in
every integer, extremum and peak field."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import BYTES_PER_FRAME, FMT, StatsDerived, StatsResult, check
from .psd import _Accumulator

_ARRAYS = dict(rail_lo=np.uint64, rail_hi=np.uint64, hist=np.uint64, min=np.float32, max=np.float32, sum=np.float64, sum_sq=np.float64)


def geometry():
    """frames per page of the accumulator's summation order (diagnostics, for tests)"""
    g = C.c_size_t(0)
    _lib.load().iqgpu_stats_geometry(C.byref(g))
    return int(g.value)


def view(result, name):
    """a numpy view (no copy) of one array field of a StatsResult: rail_lo, rail_hi, min, max, sum, sum_sq [2]; hist [2][256]"""
    return np.ctypeslib.as_array(getattr(result, name)).view(_ARRAYS[name])


def as_dict(result):
    """every field of a StatsResult (or StatsDerived) as plain Python values, arrays as nested lists"""
    out = {}
    for name, _ in result._fields_:
        v = getattr(result, name)
        out[name] = np.ctypeslib.as_array(v).tolist() if isinstance(v, C.Array) else v
    return out


def copy(result):
    """an independent StatsResult with the same bytes"""
    r = StatsResult()
    C.memmove(C.byref(r), C.byref(result), C.sizeof(StatsResult))
    return r


def merge(into, nxt):
    """iqgpu_stats_merge: `nxt` is the result of the stream directly behind `into`'s; `into` is updated in place and returned -- no device"""
    check(_lib.load().iqgpu_stats_merge(C.byref(into), C.byref(nxt)))
    return into


def derive(result):
    """iqgpu_stats_derive: the StatsDerived of a result -- no device"""
    d = StatsDerived()
    check(_lib.load().iqgpu_stats_derive(C.byref(result), C.byref(d)))
    return d


class Stats(_Accumulator):
    """One accumulator (iqgpu_stats).  push takes host frames (any array: its bytes), push_device a device pointer; read returns a
    StatsResult (a ctypes structure; view(r, "hist") and the like give numpy views) and synchronises."""
    _destroy = "iqgpu_stats_destroy"

    def __init__(self, fmt, device=0):
        self._h = C.c_void_p()
        self._lib = _lib.load()
        self.format = FMT[fmt] if isinstance(fmt, str) else int(fmt)
        check(self._lib.iqgpu_stats_create(int(device), self.format, C.byref(self._h)))
        self.bytes_per_frame = BYTES_PER_FRAME[self.format]

    def push(self, frames):
        raw, n = self._whole_frames(frames)
        check(self._lib.iqgpu_stats_push(self._h, raw.ctypes.data_as(C.c_void_p), n))

    def push_device(self, ptr, frames, stream=None):
        check(self._lib.iqgpu_stats_push_device(self._h, C.c_void_p(ptr), int(frames), C.c_void_p(stream)))

    def read(self):
        r = StatsResult()
        check(self._lib.iqgpu_stats_read(self._h, C.byref(r)))
        return r

    def reset(self):
        check(self._lib.iqgpu_stats_reset(self._h))
