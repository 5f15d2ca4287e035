"""Template correlation on the device (include/iqgpu.h "template correlation"): the matched filter of up to eight known waveforms
over one stream, reduced per block of block_frames start positions to the largest correlation power, where it is and the sum of the
block's powers.  Rows and the open row are a function of the pushed frames and the options alone, bit for bit, however the stream was
cut into pushes.  shift_bank() makes frequency-shifted copies of a template and peaks() turns finished rows into detections -- no
device.  A burst that correlates with a member shifted by hz is centred by a chain with shift_hz = -hz."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import BYTES_PER_FRAME, FMT, MatchInfo, MatchOpts, MatchPeak, check
from .psd import _Accumulator


def _templates(templates):
    """complex64 [n_templates, L] of one template or several"""
    t = np.ascontiguousarray(templates, np.complex64)
    return t.reshape(1, -1) if t.ndim == 1 else t.reshape(t.shape[0], -1)


def match_opts(template_frames, n_templates=1, block_frames=None, nfft=0):
    """iqgpu_match_opts: the library's defaults with the given fields on top"""
    o = MatchOpts()
    _lib.load().iqgpu_match_opts_init(C.byref(o))
    o.nfft, o.n_templates, o.template_frames = int(nfft), int(n_templates), int(template_frames)
    if block_frames is not None:
        o.block_frames = int(block_frames)
    return o


def rows(frames, template_frames, n_templates=1, block_frames=None, nfft=0):
    """rows a stream of `frames` frames finishes -- no device"""
    o, n = match_opts(template_frames, n_templates, block_frames, nfft), C.c_uint64(0)
    check(_lib.load().iqgpu_match_rows(C.byref(o), int(frames), C.byref(n)))
    return int(n.value)


def shift_bank(template, hz, sample_rate):
    """iqgpu_match_shift_bank: complex64 [len(hz), L], member i = template[k] exp(+j 2 pi hz[i] k / sample_rate) -- no device"""
    t = np.ascontiguousarray(template, np.complex64).reshape(-1)
    f = np.ascontiguousarray(hz, np.float64).reshape(-1)
    out = np.empty((f.size, t.size), np.complex64)
    check(_lib.load().iqgpu_match_shift_bank(t.ctypes.data_as(C.c_void_p), t.size, f.ctypes.data_as(C.c_void_p), f.size, float(sample_rate),
                                             out.ctypes.data_as(C.c_void_p)))
    return out


def peaks(row_peak, row_at, row_sum, block_frames, template_frames, ratio, nfft=0, cap=None):
    """iqgpu_match_peaks over rows as Match.push returned them ([rows, n_templates] each): a list of dicts (first_frame, template, peak,
    ratio), by row then template.  cap: room for that many (None: as many as there are); too small raises ECAPACITY -- no device"""
    pk = np.ascontiguousarray(row_peak, np.float32)
    pk = pk.reshape(pk.shape[0], int(np.prod(pk.shape[1:]))) if pk.ndim > 1 else pk.reshape(-1, 1)
    at, sm = np.ascontiguousarray(row_at, np.uint32).reshape(pk.shape), np.ascontiguousarray(row_sum, np.float32).reshape(pk.shape)
    o = match_opts(template_frames, pk.shape[1], block_frames, nfft)
    room = pk.size if cap is None else int(cap)
    out, n = (MatchPeak * max(room, 1))(), C.c_size_t(0)
    check(_lib.load().iqgpu_match_peaks(pk.ctypes.data_as(C.c_void_p), at.ctypes.data_as(C.c_void_p), sm.ctypes.data_as(C.c_void_p), pk.shape[0],
                                        C.byref(o), float(ratio), out, room, C.byref(n)))
    return [dict(first_frame=int(d.first_frame), template=int(d.template_index), peak=float(d.peak), ratio=float(d.ratio)) for d in out[:n.value]]


class Match(_Accumulator):
    """One template-correlation accumulator (iqgpu_match).  templates: complex [L] or [n_templates, L].  push takes host frames (any
    array: its bytes) and returns the rows they finish as (row_peak float32, row_at uint32, row_sum float32), [rows, n_templates] each;
    push_device takes device pointers for the input and the three planes (0 / None: that plane is not produced) and returns the row
    count; read_open returns the open row and synchronises."""
    _destroy = "iqgpu_match_destroy"

    def __init__(self, format, templates, block_frames=4096, nfft=0, device=0):
        self._h = C.c_void_p()
        self._lib = _lib.load()
        self.format = FMT[format] if isinstance(format, str) else int(format)
        t = _templates(templates)
        self.n_templates, self.template_frames = int(t.shape[0]), int(t.shape[1])
        self.opts = match_opts(self.template_frames, self.n_templates, block_frames, nfft)
        self.block_frames = int(self.opts.block_frames)
        check(self._lib.iqgpu_match_create(int(device), self.format, C.byref(self.opts), t.ctypes.data_as(C.c_void_p), C.byref(self._h)))
        self.bytes_per_frame = BYTES_PER_FRAME[self.format]
        self.nfft = self.read_open()[3]["nfft"]

    def max_rows(self, frames):
        """rows the next push of `frames` frames finishes, from the handle's position: exact"""
        return int(self._lib.iqgpu_match_max_rows(self._h, int(frames)))

    def push(self, frames):
        raw, n = self._whole_frames(frames)
        cap, got, shape = self.max_rows(n), C.c_size_t(0), (self.max_rows(n), self.n_templates)
        pk, at, sm = np.empty(shape, np.float32), np.empty(shape, np.uint32), np.empty(shape, np.float32)
        check(self._lib.iqgpu_match_push(self._h, raw.ctypes.data_as(C.c_void_p), n, pk.ctypes.data_as(C.c_void_p), at.ctypes.data_as(C.c_void_p),
                                         sm.ctypes.data_as(C.c_void_p), cap, C.byref(got)))
        assert got.value == cap
        return pk, at, sm

    def push_device(self, ptr, frames, out_peak_ptr, out_at_ptr, out_sum_ptr, cap_rows, stream=None):
        got = C.c_size_t(0)
        check(self._lib.iqgpu_match_push_device(self._h, C.c_void_p(ptr), int(frames), C.c_void_p(out_peak_ptr or None), C.c_void_p(out_at_ptr or None),
                                                C.c_void_p(out_sum_ptr or None), int(cap_rows), C.byref(got), C.c_void_p(stream)))
        return int(got.value)

    def read_open(self):
        """(sum float64[n_templates], peak float32[n_templates], at uint32[n_templates], info dict) of the open row"""
        nt = self.n_templates
        s, k, a, info = np.empty(nt, np.float64), np.empty(nt, np.float32), np.empty(nt, np.uint32), MatchInfo()
        check(self._lib.iqgpu_match_read_open(self._h, s.ctypes.data_as(C.c_void_p), k.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p),
                                              C.byref(info)))
        d = {n: getattr(info, n) for n, _ in MatchInfo._fields_ if n != "reserved"}
        d["template_energy"] = list(info.template_energy)[:nt]
        return s, k, a, d

    def reset(self):
        check(self._lib.iqgpu_match_reset(self._h))
