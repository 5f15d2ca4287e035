"""Time-resolved spectrum of a stream on the device (include/iqgpu.h "spectrogram"): the power spectrum per row of row_segments
consecutive segments, emitted as the stream goes by.  Rows and the open row are a function of the pushed frames and the options alone,
bit for bit, however the stream was cut into pushes; a row equals a fresh Psd pushed that row's frames."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import BYTES_PER_FRAME, FMT, PSD_WINDOW, SgramInfo, SgramOpts, check
from .psd import _Accumulator


def sgram_opts(nfft=1024, hop=None, window="hann", gain=1.0, row_segments=32):
    """iqgpu_sgram_opts: the library's defaults with the given fields on top (hop None: nfft / 2)"""
    o = SgramOpts()
    _lib.load().iqgpu_sgram_opts_init(C.byref(o))
    o.nfft = int(nfft)
    o.hop = int(nfft) // 2 if hop is None else int(hop)
    o.window = PSD_WINDOW[window] if isinstance(window, str) else int(window)
    o.gain = float(gain)
    o.row_segments = int(row_segments)
    return o


def rows(frames, nfft=1024, hop=None, row_segments=32):
    """rows a stream of `frames` frames finishes -- no device"""
    o = sgram_opts(nfft=nfft, hop=hop, row_segments=row_segments)
    n = C.c_uint64(0)
    check(_lib.load().iqgpu_sgram_rows(C.byref(o), int(frames), C.byref(n)))
    return int(n.value)


class Sgram(_Accumulator):
    """One row accumulator (iqgpu_sgram).  push takes host frames (any array: its bytes) and returns the rows they finish as
    (row_sum, row_peak), float32 [rows, nfft] in natural bin order; push_device takes device pointers for input and output planes
    (0 / None: that plane is not produced) and returns the row count; read_open returns the partial last row and synchronises."""
    _destroy = "iqgpu_sgram_destroy"

    def __init__(self, format, nfft=1024, hop=None, window="hann", gain=1.0, row_segments=32, device=0):
        self._h = C.c_void_p()
        self._lib = _lib.load()
        self.format = FMT[format] if isinstance(format, str) else int(format)
        self.opts = sgram_opts(nfft, hop, window, gain, row_segments)
        self.nfft, self.hop, self.row_segments = int(self.opts.nfft), int(self.opts.hop), int(self.opts.row_segments)
        check(self._lib.iqgpu_sgram_create(int(device), self.format, C.byref(self.opts), C.byref(self._h)))
        self.bytes_per_frame = BYTES_PER_FRAME[self.format]

    def max_rows(self, frames):
        """rows the next push of `frames` frames finishes, from the handle's position: exact"""
        return int(self._lib.iqgpu_sgram_max_rows(self._h, int(frames)))

    def push(self, frames):
        raw, n = self._whole_frames(frames)
        cap, got = self.max_rows(n), C.c_size_t(0)
        row_sum, row_peak = np.empty((cap, self.nfft), np.float32), np.empty((cap, self.nfft), np.float32)
        check(self._lib.iqgpu_sgram_push(self._h, raw.ctypes.data_as(C.c_void_p), n, row_sum.ctypes.data_as(C.c_void_p),
                                         row_peak.ctypes.data_as(C.c_void_p), cap, C.byref(got)))
        assert got.value == cap
        return row_sum, row_peak

    def push_device(self, ptr, frames, out_sum_ptr, out_peak_ptr, cap_rows, stream=None):
        got = C.c_size_t(0)
        check(self._lib.iqgpu_sgram_push_device(self._h, C.c_void_p(ptr), int(frames), C.c_void_p(out_sum_ptr or None),
                                                C.c_void_p(out_peak_ptr or None), int(cap_rows), C.byref(got), C.c_void_p(stream)))
        return int(got.value)

    def read_open(self):
        """(sum_power float64[nfft], peak_power float32[nfft], info dict) of the open row"""
        s, k, info = np.empty(self.nfft, np.float64), np.empty(self.nfft, np.float32), SgramInfo()
        check(self._lib.iqgpu_sgram_read_open(self._h, s.ctypes.data_as(C.c_void_p), k.ctypes.data_as(C.c_void_p), C.byref(info)))
        return s, k, {n: getattr(info, n) for n, _ in SgramInfo._fields_}

    def reset(self):
        check(self._lib.iqgpu_sgram_reset(self._h))
