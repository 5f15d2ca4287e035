"""Host-side mirror of the reference's I/Q imbalance optimiser (src/iq_correct.c:154-219, 315-393; thread
src/utility_threads.c:35-47) over the C ABI of include/iqgpu.h.  The optimiser itself is host code in the
reference and here; the GPU chain only supplies the probe block and consumes the factors."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import IqCalibOpts, IqCalibReport, IqOptimizerStats, RAND_DIR_FN, check

FFT_SIZE = 1024            # IQ_CORRECTION_FFT_SIZE, include/constants.h:157
# iqgpu_iq_cand as a numpy record: the candidate lists metric_batch takes
IQ_CAND = np.dtype([("mag", np.float32), ("phase", np.float32)])


# ---- I/Q calibration (include/iqgpu.h): the utility over many blocks and a grid of candidates, searched deterministically ----
class IqCalibration:
    """what a calibration returns (iqgpu_iq_calib_report): found, mag, phase, the totals before and after, the block counts and
    levels -- one dict per level with center_mag, center_phase, step, pick and total_at_pick"""

    def __init__(self, rep, opts):
        self.found = bool(rep.found)
        self.mag, self.phase = float(rep.mag), float(rep.phase)
        self.total_at_center0, self.total_at_best = float(rep.total_at_center0), float(rep.total_at_best)
        self.blocks_taken, self.blocks_used = int(rep.blocks_taken), int(rep.blocks_used)
        self.evaluations = int(rep.evaluations)
        self.grid = int(opts.grid)
        self.levels = [dict(center_mag=float(lv.center_mag), center_phase=float(lv.center_phase), step=float(lv.step),
                            pick=int(lv.pick), total_at_pick=float(lv.total_at_pick)) for lv in rep.level[:rep.n_levels]]

    @property
    def factors(self):
        return self.mag, self.phase

    def __repr__(self):
        return "IqCalibration(found=%s, mag=%.9g, phase=%.9g, levels=%d, blocks_used=%d/%d)" % (
            self.found, self.mag, self.phase, len(self.levels), self.blocks_used, self.blocks_taken)


def calib_opts(**kw):
    """iqgpu_iq_calib_opts with the library's defaults (max_blocks 64, grid 9, span 0.1, min_step 1e-4, power_threshold_db 20,
    centre (0, 0)) and the given fields on top"""
    o = IqCalibOpts()
    _lib.load().iqgpu_iq_calib_opts_init(C.byref(o))
    names = {n for n, _ in IqCalibOpts._fields_}
    for k, v in kw.items():
        if k not in names:
            raise TypeError("unknown calibration option %r" % k)
        setattr(o, k, v)
    return o


def level_grid(center_mag, center_phase, step, grid):
    """the candidates of one level as IQ_CAND records, in float as the library builds them: index im * grid + ip"""
    h = (int(grid) - 1) // 2
    off = (np.arange(grid, dtype=np.int32) - h).astype(np.float32) * np.float32(step)
    out = np.empty(grid * grid, IQ_CAND)
    out["mag"] = np.repeat(np.float32(center_mag) + off, grid)
    out["phase"] = np.tile(np.float32(center_phase) + off, grid)
    return out


def _blocks(blocks, stride):
    """(array, n_blocks, stride) of cf32 blocks: a 2-D array of rows of 1024, or a flat one with block b at b * stride"""
    b = np.ascontiguousarray(blocks, np.complex64)
    if b.ndim == 2:
        if b.shape[1] != FFT_SIZE:
            raise ValueError("blocks are rows of %d samples" % FFT_SIZE)
        return b, b.shape[0], FFT_SIZE
    stride = FFT_SIZE if stride is None else int(stride)
    n = 0 if b.size < FFT_SIZE or stride < 1 else (b.size - FFT_SIZE) // stride + 1
    return b, n, stride


def metric_geometry():
    """(candidates per launch, candidates per wave) of the device metric"""
    a, b = C.c_size_t(0), C.c_size_t(0)
    _lib.load().iqgpu_iq_metric_geometry(C.byref(a), C.byref(b))
    return int(a.value), int(b.value)


def _cands(cands):
    c = np.asarray(cands)
    if c.dtype != IQ_CAND:
        c = np.asarray(cands, np.float32).reshape(-1, 2).copy().view(IQ_CAND).reshape(-1)
    return np.ascontiguousarray(c)


def metric_batch(blocks, cands, stride=None, device=0, power=False):
    """the optimiser's utility of every (block, candidate) on the GPU (iqgpu_iq_metric_batch): an array [n_blocks, n_cand]; with
    power=True also power_range_db per block.  cands: IQ_CAND records or (mag, phase) pairs"""
    b, n, stride = _blocks(blocks, stride)
    c = _cands(cands)
    metric = np.empty((n, c.size), np.float32)
    pr = np.empty(n, np.float32) if power else None
    check(_lib.load().iqgpu_iq_metric_batch(int(device), b.ctypes.data_as(C.c_void_p), n, stride, c.ctypes.data_as(C.c_void_p), c.size,
                                            metric.ctypes.data_as(C.c_void_p), pr.ctypes.data_as(C.c_void_p) if power else None))
    return (metric, pr) if power else metric


def metric_batch_device(d_blocks, n_blocks, cands, stride=FFT_SIZE, device=0, power=False, hip_stream=None):
    """metric_batch() with the blocks already in device memory (a device address as an int), block b at frame b * stride"""
    c = _cands(cands)
    metric = np.empty((int(n_blocks), c.size), np.float32)
    pr = np.empty(int(n_blocks), np.float32) if power else None
    check(_lib.load().iqgpu_iq_metric_batch_device(int(device), C.c_void_p(d_blocks), int(n_blocks), int(stride), c.ctypes.data_as(C.c_void_p),
                                                   c.size, metric.ctypes.data_as(C.c_void_p), pr.ctypes.data_as(C.c_void_p) if power else None,
                                                   C.c_void_p(hip_stream)))
    return (metric, pr) if power else metric


class IqOptimizer:
    def __init__(self, seed=None, rng=None):
        """seed: private deterministic direction source; rng: callable returning +1 / -1; neither: libc rand()
        as the reference (src/iq_correct.c:391-393)."""
        self._lib = _lib.load()
        h = C.c_void_p()
        check(self._lib.iqgpu_iq_optimizer_create(C.byref(h)))
        self._h = h
        self._cb = None
        if rng is not None:
            self._cb = RAND_DIR_FN(lambda _u: float(rng()))
            check(self._lib.iqgpu_iq_optimizer_set_rng(self._h, self._cb, None))
        elif seed is not None:
            check(self._lib.iqgpu_iq_optimizer_seed(self._h, int(seed)))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.iqgpu_iq_optimizer_destroy(self._h)
            self._h = None

    __del__ = close

    @staticmethod
    def _block(block):
        b = np.ascontiguousarray(block, np.complex64)
        if b.size != FFT_SIZE:
            raise ValueError("the optimiser works on blocks of %d samples" % FFT_SIZE)
        return b

    def set_factors(self, mag, phase):
        check(self._lib.iqgpu_iq_optimizer_set_factors(self._h, mag, phase))

    def factors(self):
        m, p = C.c_float(0), C.c_float(0)
        check(self._lib.iqgpu_iq_optimizer_get_factors(self._h, C.byref(m), C.byref(p)))
        return m.value, p.value

    def metric(self, block, mag, phase):
        """_calculate_imbalance_metric (src/iq_correct.c:339-360)"""
        b = self._block(block)
        return self._lib.iqgpu_iq_optimizer_metric(self._h, b.ctypes.data_as(C.c_void_p), mag, phase)

    def calibrate(self, blocks, stride=None, **opts):
        """the calibration search with the HOST metric (iqgpu_iq_optimizer_calibrate; no device) over cf32 blocks -- rows of 1024,
        or a flat array with block b at b * stride.  opts: the fields of iqgpu_iq_calib_opts.  Returns an IqCalibration"""
        b, n, stride = _blocks(blocks, stride)
        o = calib_opts(**opts)
        rep = IqCalibReport()
        check(self._lib.iqgpu_iq_optimizer_calibrate(self._h, b.ctypes.data_as(C.c_void_p), n, stride, C.byref(o), C.byref(rep)))
        return IqCalibration(rep, o)

    def run_optimization(self, block, now_sec=-1.0):
        """iq_correct_run_optimization (src/iq_correct.c:154-219); True if the factors were updated"""
        b = self._block(block)
        upd = C.c_int(0)
        check(self._lib.iqgpu_iq_optimizer_run(self._h, b.ctypes.data_as(C.c_void_p), float(now_sec), C.byref(upd)))
        return bool(upd.value)

    def touch(self, now_sec=-1.0):
        check(self._lib.iqgpu_iq_optimizer_touch(self._h, float(now_sec)))

    def stats(self):
        st = IqOptimizerStats()
        check(self._lib.iqgpu_iq_optimizer_get_stats(self._h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in IqOptimizerStats._fields_}

    def service(self, chain, now_sec=-1.0):
        """the optimiser thread's loop body (src/utility_threads.c:35-47): probe -> run -> set_iq_factors"""
        upd = C.c_int(0)
        check(self._lib.iqgpu_iq_optimizer_service(self._h, chain._h, float(now_sec), C.byref(upd)))
        return bool(upd.value)
