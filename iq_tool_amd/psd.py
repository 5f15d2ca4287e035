"""Power spectrum of a stream on the device (include/iqgpu.h "power spectrum"): an averaged (Welch) periodogram with a max-hold
trace over one stream of frames in one sample format, independent of any chain.  The result is a function of the pushed frames and
the options alone, bit for bit, however the stream was cut into pushes."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import BYTES_PER_FRAME, FMT, PSD_WINDOW, PsdInfo, PsdOpts, check


def psd_opts(nfft=1024, hop=None, window="hann", gain=1.0):
    """iqgpu_psd_opts: the library's defaults with the given fields on top (hop None: nfft / 2)"""
    o = PsdOpts()
    _lib.load().iqgpu_psd_opts_init(C.byref(o))
    o.nfft = int(nfft)
    o.hop = int(nfft) // 2 if hop is None else int(hop)
    o.window = PSD_WINDOW[window] if isinstance(window, str) else int(window)
    o.gain = float(gain)
    return o


def window(nfft=1024, window="hann"):
    """(the float32 window table the accumulator uploads, its sum, the sum of its squares) -- no device"""
    o = psd_opts(nfft=nfft, window=window)
    w = np.empty(o.nfft, np.float32)
    s, q = C.c_double(0), C.c_double(0)
    check(_lib.load().iqgpu_psd_window(C.byref(o), w.ctypes.data_as(C.c_void_p), w.size, C.byref(s), C.byref(q)))
    return w, s.value, q.value


def segments(frames, nfft=1024, hop=None):
    """whole segments of a stream of `frames` frames -- no device"""
    o = psd_opts(nfft=nfft, hop=hop)
    n = C.c_uint64(0)
    check(_lib.load().iqgpu_psd_segments(C.byref(o), int(frames), C.byref(n)))
    return int(n.value)


def geometry():
    """segments per page of the accumulator's summation order (diagnostics, for tests)"""
    g = C.c_size_t(0)
    _lib.load().iqgpu_psd_geometry(C.byref(g))
    return int(g.value)


class _Accumulator:
    """What Psd and Sgram (sgram.py) share: the life of the handle `_h`, destroyed by the library call named `_destroy`, and the
    bytes of a host push."""

    def close(self):
        if getattr(self, "_h", None):
            getattr(self._lib, self._destroy)(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _whole_frames(self, frames):
        """(the bytes of `frames` as a contiguous uint8 array, how many frames they are)"""
        raw = np.ascontiguousarray(frames).view(np.uint8).reshape(-1)
        if raw.size % self.bytes_per_frame:
            raise ValueError("%d bytes are no whole number of %d-byte frames" % (raw.size, self.bytes_per_frame))
        return raw, raw.size // self.bytes_per_frame


class Psd(_Accumulator):
    """One accumulator (iqgpu_psd).  push takes host frames (any array: its bytes), push_device a device pointer; read returns
    (sum_power float64[nfft], peak_power float32[nfft], info dict) in natural bin order and synchronises."""
    _destroy = "iqgpu_psd_destroy"

    def __init__(self, format, nfft=1024, hop=None, window="hann", gain=1.0, device=0):
        self._h = C.c_void_p()
        self._lib = _lib.load()
        self.format = FMT[format] if isinstance(format, str) else int(format)
        self.opts = psd_opts(nfft, hop, window, gain)
        self.nfft, self.hop = int(self.opts.nfft), int(self.opts.hop)
        check(self._lib.iqgpu_psd_create(int(device), self.format, C.byref(self.opts), C.byref(self._h)))
        self.bytes_per_frame = BYTES_PER_FRAME[self.format]

    def push(self, frames):
        raw, n = self._whole_frames(frames)
        check(self._lib.iqgpu_psd_push(self._h, raw.ctypes.data_as(C.c_void_p), n))

    def push_device(self, ptr, frames, stream=None):
        check(self._lib.iqgpu_psd_push_device(self._h, C.c_void_p(ptr), int(frames), C.c_void_p(stream)))

    def read(self):
        s, k, info = np.empty(self.nfft, np.float64), np.empty(self.nfft, np.float32), PsdInfo()
        check(self._lib.iqgpu_psd_read(self._h, s.ctypes.data_as(C.c_void_p), k.ctypes.data_as(C.c_void_p), C.byref(info)))
        return s, k, {n: getattr(info, n) for n, _ in PsdInfo._fields_}

    def reset(self):
        check(self._lib.iqgpu_psd_reset(self._h))

    def spectrum(self, rate_hz):
        """fft-shifted (freqs in Hz, mean power in dBFS, max-hold power in dBFS), computed on the host from read(): a full-scale
        tone reads 0 dBFS.  Bins without power read -inf; before the first whole segment all of them do."""
        s, k, info = self.read()
        n, ws = info["segments"], info["window_sum"]
        with np.errstate(divide="ignore"):
            mean = 10.0 * np.log10(s / (max(n, 1) * ws * ws))
            peak = 10.0 * np.log10(k.astype(np.float64) / (ws * ws))
        freqs = np.fft.fftshift(np.fft.fftfreq(self.nfft, 1.0 / float(rate_hz)))
        return freqs, np.fft.fftshift(mean), np.fft.fftshift(peak)
