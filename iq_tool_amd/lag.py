"""Frequency against time on the device (include/iqgpu.h "lag products"): R_d = sum x[n] conj(x[n - d]) for up to four lags d, and the
power, per block of block_frames consecutive frames, emitted as the stream goes by.  Rows and the open row are a function of the pushed
frames and the options alone, bit for bit, however the stream was cut into pushes.  freq() and estimate() turn finished rows into a
frequency and a coherence -- no device.  A burst estimated at hz is centred by a chain with shift_hz = -hz."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import BYTES_PER_FRAME, FMT, LagEstimate, LagInfo, LagOpts, check
from .psd import _Accumulator


def lag_opts(block_frames=None, lags=None):
    """iqgpu_lag_opts: the library's defaults with the given fields on top"""
    o = LagOpts()
    _lib.load().iqgpu_lag_opts_init(C.byref(o))
    if block_frames is not None:
        o.block_frames = int(block_frames)
    if lags is not None:
        lags = [int(d) for d in lags]
        o.n_lags = len(lags)
        for i in range(4):
            o.lags[i] = lags[i] if i < len(lags) and 0 <= lags[i] < 1 << 32 else 0
        if len(lags) > 4:
            o.n_lags = 5                         # (the library refuses it)
    return o


def rows(frames, block_frames=None, lags=None):
    """rows a stream of `frames` frames finishes -- no device"""
    o, n = lag_opts(block_frames, lags), C.c_uint64(0)
    check(_lib.load().iqgpu_lag_rows(C.byref(o), int(frames), C.byref(n)))
    return int(n.value)


def freq(re, im, lag, sample_rate):
    """iqgpu_lag_freq: atan2(im, re) / (2 pi lag) * sample_rate -- no device"""
    hz = C.c_double(0.0)
    check(_lib.load().iqgpu_lag_freq(float(re), float(im), int(lag), float(sample_rate), C.byref(hz)))
    return hz.value


def estimate(row_lag, row_sum, block_frames, lags, lag_index, sample_rate, first_row=0, n_rows=None):
    """iqgpu_lag_estimate_rows over rows first_row .. first_row + n_rows - 1 (default: to the last) as a dict (re, im, power, hz,
    coherence, span_hz); row_lag is what Lag.push returned (complex64 [rows, n_lags]) or its floats, row_sum may be None -- no device"""
    o = lag_opts(block_frames, lags)
    v = np.ascontiguousarray(row_lag).view(np.float32).reshape(-1)
    n = v.size // (2 * max(1, int(o.n_lags)))
    s = None if row_sum is None else np.ascontiguousarray(row_sum, np.float32)
    if s is not None and s.size != n:
        raise ValueError("row_sum holds %d rows, row_lag %d" % (s.size, n))
    out = LagEstimate()
    check(_lib.load().iqgpu_lag_estimate_rows(v.ctypes.data_as(C.c_void_p), None if s is None else s.ctypes.data_as(C.c_void_p), n, C.byref(o),
                                              int(lag_index), int(first_row), n - int(first_row) if n_rows is None else int(n_rows),
                                              float(sample_rate), C.byref(out)))
    return {k: getattr(out, k) for k, _ in LagEstimate._fields_}


class Lag(_Accumulator):
    """One lag-product accumulator (iqgpu_lag).  push takes host frames (any array: its bytes) and returns the rows they finish as
    (row_lag complex64 [rows, n_lags], row_sum float32 [rows]); push_device takes device pointers for the input and the two planes
    (0 / None: that plane is not produced) and returns the row count; read_open returns the open row and synchronises."""
    _destroy = "iqgpu_lag_destroy"

    def __init__(self, format, block_frames=4096, lags=(1,), device=0):
        self._h = C.c_void_p()
        self._lib = _lib.load()
        self.format = FMT[format] if isinstance(format, str) else int(format)
        self.opts = lag_opts(block_frames, lags)
        self.block_frames, self.lags = int(self.opts.block_frames), tuple(int(d) for d in lags)
        check(self._lib.iqgpu_lag_create(int(device), self.format, C.byref(self.opts), C.byref(self._h)))
        self.bytes_per_frame = BYTES_PER_FRAME[self.format]

    def max_rows(self, frames):
        """rows the next push of `frames` frames finishes, from the handle's position: exact"""
        return int(self._lib.iqgpu_lag_max_rows(self._h, int(frames)))

    def push(self, frames):
        raw, n = self._whole_frames(frames)
        cap, got = self.max_rows(n), C.c_size_t(0)
        r, s = np.empty((cap, len(self.lags)), np.complex64), np.empty(cap, np.float32)
        check(self._lib.iqgpu_lag_push(self._h, raw.ctypes.data_as(C.c_void_p), n, r.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p),
                                       cap, C.byref(got)))
        assert got.value == cap
        return r, s

    def push_device(self, ptr, frames, out_lag_ptr, out_sum_ptr, cap_rows, stream=None):
        got = C.c_size_t(0)
        check(self._lib.iqgpu_lag_push_device(self._h, C.c_void_p(ptr), int(frames), C.c_void_p(out_lag_ptr or None),
                                              C.c_void_p(out_sum_ptr or None), int(cap_rows), C.byref(got), C.c_void_p(stream)))
        return int(got.value)

    def read_open(self):
        """(lag complex128[n_lags], sum float, info dict) of the open row: the unrounded doubles"""
        v, s, info = (C.c_double * 8)(), C.c_double(0.0), LagInfo()
        check(self._lib.iqgpu_lag_read_open(self._h, v, C.byref(s), C.byref(info)))
        d = {n: getattr(info, n) for n, _ in LagInfo._fields_}
        d["lags"] = list(info.lags)[:info.n_lags]
        return np.array([complex(v[2 * i], v[2 * i + 1]) for i in range(len(self.lags))], np.complex128), s.value, d

    def reset(self):
        check(self._lib.iqgpu_lag_reset(self._h))
