"""Power against time on the device (include/iqgpu.h "envelope"): the sum and the peak of the frame power and the count of rail-valued
components per block of block_frames consecutive frames, emitted as the stream goes by.  Rows and the open row are a function of the
pushed frames and block_frames alone, bit for bit, however the stream was cut into pushes.  bursts() and floor() turn finished rows into
(first_frame, frames) ranges for Chain.seek and the harness's range modes -- no device."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import BYTES_PER_FRAME, FMT, EnvBurst, EnvBurstOpts, EnvInfo, EnvOpts, check
from .psd import _Accumulator


def env_opts(block_frames=None):
    """iqgpu_env_opts: the library's default with the given field on top"""
    o = EnvOpts()
    _lib.load().iqgpu_env_opts_init(C.byref(o))
    if block_frames is not None:
        o.block_frames = int(block_frames)
    return o


def rows(frames, block_frames=None):
    """rows a stream of `frames` frames finishes -- no device"""
    o, n = env_opts(block_frames), C.c_uint64(0)
    check(_lib.load().iqgpu_env_rows(C.byref(o), int(frames), C.byref(n)))
    return int(n.value)


def bursts(row_sum, block_frames, on, off, min_rows=1, hang_rows=0, pad_rows=0):
    """iqgpu_env_bursts: the bursts of finished rows as a list of dicts (first_frame, frames, peak_row, peak_mean) -- no device"""
    lib = _lib.load()
    v = np.ascontiguousarray(row_sum, np.float32)
    o = EnvBurstOpts(int(block_frames), int(min_rows), int(hang_rows), int(pad_rows), float(on), float(off))
    n = C.c_size_t(0)
    rc = lib.iqgpu_env_bursts(v.ctypes.data_as(C.c_void_p), v.size, C.byref(o), None, 0, C.byref(n))
    if rc != -8:                                 # (IQGPU_ECAPACITY: the count asked for)
        check(rc)
    out = (EnvBurst * max(1, n.value))()
    check(lib.iqgpu_env_bursts(v.ctypes.data_as(C.c_void_p), v.size, C.byref(o), C.cast(out, C.c_void_p), n.value, C.byref(n)))
    return [{k: getattr(out[i], k) for k, _ in EnvBurst._fields_} for i in range(n.value)]


def floor(row_sum, block_frames, fraction=0.1):
    """iqgpu_env_floor: the mean power of the row at rank floor(fraction (rows - 1)) of the ascending order -- no device"""
    v, m = np.ascontiguousarray(row_sum, np.float32), C.c_double(0.0)
    check(_lib.load().iqgpu_env_floor(v.ctypes.data_as(C.c_void_p), v.size, int(block_frames), float(fraction), C.byref(m)))
    return m.value


class Env(_Accumulator):
    """One envelope accumulator (iqgpu_env).  push takes host frames (any array: its bytes) and returns the rows they finish as
    (row_sum float32, row_peak float32, row_rail uint32); push_device takes device pointers for the input and the three planes
    (0 / None: that plane is not produced) and returns the row count; read_open returns the open row and synchronises."""
    _destroy = "iqgpu_env_destroy"

    def __init__(self, format, block_frames=None, device=0):
        self._h = C.c_void_p()
        self._lib = _lib.load()
        self.format = FMT[format] if isinstance(format, str) else int(format)
        self.opts = env_opts(block_frames)
        self.block_frames = int(self.opts.block_frames)
        check(self._lib.iqgpu_env_create(int(device), self.format, C.byref(self.opts), C.byref(self._h)))
        self.bytes_per_frame = BYTES_PER_FRAME[self.format]

    def max_rows(self, frames):
        """rows the next push of `frames` frames finishes, from the handle's position: exact"""
        return int(self._lib.iqgpu_env_max_rows(self._h, int(frames)))

    def push(self, frames):
        raw, n = self._whole_frames(frames)
        cap, got = self.max_rows(n), C.c_size_t(0)
        s, k, r = np.empty(cap, np.float32), np.empty(cap, np.float32), np.empty(cap, np.uint32)
        check(self._lib.iqgpu_env_push(self._h, raw.ctypes.data_as(C.c_void_p), n, s.ctypes.data_as(C.c_void_p), k.ctypes.data_as(C.c_void_p),
                                       r.ctypes.data_as(C.c_void_p), cap, C.byref(got)))
        assert got.value == cap
        return s, k, r

    def push_device(self, ptr, frames, out_sum_ptr, out_peak_ptr, out_rail_ptr, cap_rows, stream=None):
        got = C.c_size_t(0)
        check(self._lib.iqgpu_env_push_device(self._h, C.c_void_p(ptr), int(frames), C.c_void_p(out_sum_ptr or None),
                                              C.c_void_p(out_peak_ptr or None), C.c_void_p(out_rail_ptr or None), int(cap_rows),
                                              C.byref(got), C.c_void_p(stream)))
        return int(got.value)

    def read_open(self):
        """(sum float, peak float, rail int, info dict) of the open row: the sum and the peak are the unrounded doubles"""
        s, k, r, info = C.c_double(0.0), C.c_double(0.0), C.c_uint32(0), EnvInfo()
        check(self._lib.iqgpu_env_read_open(self._h, C.byref(s), C.byref(k), C.byref(r), C.byref(info)))
        return s.value, k.value, int(r.value), {n: getattr(info, n) for n, _ in EnvInfo._fields_}

    def reset(self):
        check(self._lib.iqgpu_env_reset(self._h))
