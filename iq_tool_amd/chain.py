"""Host-side handle for one I/Q stream on one MI355X: a thin object over the C ABI of
include/iqgpu.h.  It stands where the reference's pre-processor, resampler and post-processor
stage threads stand (src/pipeline.c:436-595); argument names follow AppConfig
(include/app_context.h:66-138)."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import (BYTES_PER_FRAME, FILTER, FILTER_IMPL, FMT, AgcState, ChainDesc, ChainInfo, DcState, FilterReq,
                   IqgpuError, Profile, StateInfo, check)

AGC_PROFILE = {"off": 0, "dx": 1, "local": 2, "digital": 3}
# iqgpu_agc_chunk as a numpy record: what Chain.measure returns and Chain.agc_advance takes
AGC_ROW = np.dtype([("peak2", np.float64), ("frames_out", np.uint32), ("reserved", np.uint32)])
# iqgpu_dc_state / iqgpu_dc_row as numpy records: what Chain.dc_state, .dc_measure and .dc_advance return and take
DC_STATE = np.dtype([("re", np.float64), ("im", np.float64)])
DC_ROW = np.dtype([("f", np.float64), ("g_re", np.float64), ("g_im", np.float64), ("frames", np.uint64)])

_NP_VIEW = {8: np.uint8, 9: np.int8, 10: np.uint16, 11: np.int16, 16: np.int16, 12: np.uint8,
            13: np.uint32, 14: np.int32, 15: np.float32}


def _fmt(f):
    return FMT[f] if isinstance(f, str) else int(f)


def make_desc(in_format="cs16", out_format="cs16", input_rate_hz=2.4e6, target_rate_hz=744187.5,
              resample_ratio=0.0, gain=1.0, shift_hz=0.0, shift_after_resample=False,
              dc_block=False, iq_correct=False, iq_mag=0.0, iq_phase=0.0, no_resample=False,
              filters=(), transition_width_hz=0.0, attenuation_db=0.0, filter_taps=0,
              filter_impl="auto", fft_size=0, device=0, block_samples=0,
              agc=False, agc_profile="digital", agc_target=0.0, agc_clock="samples", agc_chunk_frames=0):
    lib = _lib.load()
    _lib.apply_debug_env()          # (the test / bench mirror forwards IQGPU_<NAME> variables to iqgpu_debug_set; the library reads none)
    d = ChainDesc()
    lib.iqgpu_chain_desc_init(C.byref(d))
    d.in_format = _fmt(in_format)
    d.out_format = _fmt(out_format)
    d.input_rate_hz = float(input_rate_hz)
    d.target_rate_hz = float(target_rate_hz)
    d.resample_ratio = float(resample_ratio)
    d.gain = float(gain)
    d.shift_hz = float(shift_hz)
    d.shift_after_resample = int(bool(shift_after_resample))
    d.dc_block_enable = int(bool(dc_block))
    d.iq_correct_enable = int(bool(iq_correct))
    d.iq_mag = float(iq_mag)
    d.iq_phase = float(iq_phase)
    d.no_resample = int(bool(no_resample))
    d.n_filters = len(filters)
    for i, (t, f1, f2) in enumerate(filters[:5]):
        d.filters[i] = FilterReq(FILTER[t] if isinstance(t, str) else int(t), float(f1), float(f2))
    d.transition_width_hz = float(transition_width_hz)
    d.attenuation_db = float(attenuation_db)
    # the reference bumps an even --filter-taps to the next odd number (src/config.c:233-236)
    ft = int(filter_taps)
    if ft != 0 and ft % 2 == 0:
        ft += 1
    d.filter_taps = ft
    d.filter_impl = FILTER_IMPL[filter_impl] if isinstance(filter_impl, str) else int(filter_impl)
    d.fft_size = int(fft_size)
    d.device_ordinal = int(device)
    d.block_samples = int(block_samples)
    d.agc_enable = int(bool(agc))
    d.agc_profile = AGC_PROFILE[agc_profile] if isinstance(agc_profile, str) else int(agc_profile)
    d.agc_target = float(agc_target)
    d.agc_clock = {"samples": 0, "wall": 1}[agc_clock] if isinstance(agc_clock, str) else int(agc_clock)
    d.agc_chunk_frames = int(agc_chunk_frames)
    return d


def design_out_frames(frames_in, **kw):
    """frames a FRESH chain of this description emits for a stream of frames_in frames (iqgpu_design_out_frames: the closed
    form a stitching writer places shard outputs with; no device needed)"""
    d = make_desc(**kw)
    n = C.c_size_t(0)
    check(_lib.load().iqgpu_design_out_frames(C.byref(d), int(frames_in), C.byref(n)))
    return int(n.value)


def design_preroll_frames(**kw):
    """input frames in front of a seam that a chain of this description has to see, output dropped, so that what it emits afterwards
    is what the single stream emits (iqgpu_design_preroll_frames; no device needed)"""
    d = make_desc(**kw)
    n = C.c_uint64(0)
    check(_lib.load().iqgpu_design_preroll_frames(C.byref(d), C.byref(n)))
    return int(n.value)


def design_preroll_frames_rms(desc=None, **kw):
    """P_rms: the preroll Chain.seek_rms asks for on a chain with the dx / local output AGC -- the FIR memory plus the input frames
    that make the chain emit warm + chunk outputs anywhere in the stream (iqgpu_design_preroll_frames_rms; no device needed).  desc: a
    ChainDesc, or the description as make_desc keywords"""
    d = desc if desc is not None else make_desc(**kw)
    n = C.c_uint64(0)
    check(_lib.load().iqgpu_design_preroll_frames_rms(C.byref(d), C.byref(n)))
    return int(n.value)


def design_preroll_frames_dcrms(desc=None, **kw):
    """P of Chain.dcrms_seek, for a chain with the DC blocker and the dx / local output AGC: design_preroll_frames_rms of the same
    description without the blocker (iqgpu_design_preroll_frames_dcrms; no device needed).  desc: a ChainDesc, or make_desc keywords"""
    d = desc if desc is not None else make_desc(**kw)
    n = C.c_uint64(0)
    check(_lib.load().iqgpu_design_preroll_frames_dcrms(C.byref(d), C.byref(n)))
    return int(n.value)


def design_out_frames_range(first_frame, frames_in, **kw):
    """(out_first, frames_out): what ONE stream of this description emits while it consumes input frames
    [first_frame, first_frame + frames_in) -- where a seamless shard's output goes and how long it is (no device needed)"""
    d = make_desc(**kw)
    first, n = C.c_uint64(0), C.c_uint64(0)
    check(_lib.load().iqgpu_design_out_frames_range(C.byref(d), int(first_frame), int(frames_in), C.byref(first), C.byref(n)))
    return int(first.value), int(n.value)


def design_state_size(**kw):
    """bytes of the blob Chain.save_state() returns for a chain of this description (iqgpu_design_state_size; no device needed)"""
    d = make_desc(**kw)
    n = C.c_size_t(0)
    check(_lib.load().iqgpu_design_state_size(C.byref(d), C.byref(n)))
    return int(n.value)


def state_inspect(blob):
    """validates a saved state's magic, version, size and checksum (iqgpu_state_inspect; no device needed) and returns its header
    figures: dict(format_version, bytes, fingerprint, frames_in, frames_out).  Raises IqgpuError (EINVAL) on anything else."""
    blob = bytes(blob) if blob is not None else None
    info = StateInfo()
    check(_lib.load().iqgpu_state_inspect(blob, len(blob) if blob is not None else 0, C.byref(info)))
    return dict(format_version=int(info.format_version), bytes=int(info.bytes), fingerprint=int(info.fingerprint),
                frames_in=int(info.frames_in), frames_out=int(info.frames_out))


def bind_thread_to_device(ordinal):
    """iqgpu_bind_thread_to_device: the calling thread onto the NUMA node of HIP device `ordinal` (sysfs only, no HIP call --
    meant to run before the first GPU call and before pinned buffers are allocated).  Returns (node, pci_bus_id, error): node -1
    when the host does not say or nothing could be bound, error None or the library's message."""
    lib = _lib.load()
    _lib.apply_debug_env()
    node, bus = C.c_int(-1), C.create_string_buffer(64)
    rc = lib.iqgpu_device_numa_node(int(ordinal), C.byref(node), bus, 64)
    if rc != 0:
        return -1, "", lib.iqgpu_last_error().decode("utf-8", "replace")
    rc = lib.iqgpu_bind_thread_to_device(int(ordinal), C.byref(node))
    return node.value, bus.value.decode(), (None if rc == 0 else lib.iqgpu_last_error().decode("utf-8", "replace"))


class Chain:
    """pre_processor -> resampler -> post_processor for one stream, on one GPU."""

    def __init__(self, desc=None, **kw):
        self._lib = _lib.load()
        self.desc = desc if desc is not None else make_desc(**kw)
        _lib.apply_debug_env()
        h = C.c_void_p()
        check(self._lib.iqgpu_chain_create(C.byref(self.desc), C.byref(h)))
        self._h = h
        self.device = self.desc.device_ordinal
        self.in_bytes = BYTES_PER_FRAME[self.desc.in_format]
        self.out_bytes = BYTES_PER_FRAME[self.desc.out_format]

    def close(self):
        if getattr(self, "_h", None):
            self._lib.iqgpu_chain_destroy(self._h)
            self._h = None

    __del__ = close

    # ---- description ----
    def info(self):
        i = ChainInfo()
        check(self._lib.iqgpu_chain_get_info(self._h, C.byref(i)))
        return i

    def filter_taps(self):
        n = self._lib.iqgpu_chain_get_filter_taps(self._h, None, 0)
        buf = np.zeros(2 * n, np.float32)
        self._lib.iqgpu_chain_get_filter_taps(self._h, buf.ctypes.data_as(C.c_void_p), n)
        return buf.view(np.complex64)

    def max_out_frames(self, frames_in):
        return self._lib.iqgpu_chain_max_out_frames(self._h, frames_in)

    def next_out_frames(self, frames_in):
        return self._lib.iqgpu_chain_next_out_frames(self._h, frames_in)

    # ---- stream ----
    def process(self, raw):
        """raw: numpy array holding whole frames in in_format (any dtype).  Returns the output
        frames as a numpy array of the output format's component type."""
        raw = np.ascontiguousarray(raw)
        n = raw.nbytes // self.in_bytes
        cap = (self.next_out_frames(n) + 1) * self.out_bytes
        out = np.empty(cap, np.uint8)
        got = C.c_size_t(0)
        check(self._lib.iqgpu_chain_process(self._h, raw.ctypes.data_as(C.c_void_p), n,
                                            out.ctypes.data_as(C.c_void_p), cap, C.byref(got)))
        return out[:got.value * self.out_bytes].view(_NP_VIEW[self.desc.out_format]).copy()

    def process_device(self, d_in, frames_in, d_out, out_capacity_bytes):
        """Both pointers are device addresses (ints) on this chain's GPU; asynchronous."""
        got = C.c_size_t(0)
        check(self._lib.iqgpu_chain_process_device(self._h, C.c_void_p(d_in), frames_in,
                                                   C.c_void_p(d_out), out_capacity_bytes, C.byref(got)))
        return got.value

    def submit(self, in_ptr, frames_in, out_ptr, out_capacity_bytes):
        """Queues H2D copy -> kernels -> D2H copy of one batch (host addresses, preferably pinned) and
        returns (frames_out, ticket) at once; collect(ticket) waits for the output bytes."""
        got, ticket = C.c_size_t(0), C.c_uint64(0)
        check(self._lib.iqgpu_chain_submit(self._h, C.c_void_p(in_ptr), frames_in, C.c_void_p(out_ptr),
                                           out_capacity_bytes, C.byref(got), C.byref(ticket)))
        return got.value, ticket.value

    def collect(self, ticket):
        check(self._lib.iqgpu_chain_collect(self._h, C.c_uint64(ticket)))

    def process_pipelined(self, raw, batch_frames):
        """process() through submit / collect: the stream in batches of batch_frames with up to
        iqgpu_chain_pipeline_depth() of them in flight, pinned staging buffers on both sides."""
        raw = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
        n = raw.nbytes // self.in_bytes
        depth = self._lib.iqgpu_chain_pipeline_depth()
        cap = self.max_out_frames(batch_frames) * self.out_bytes
        slots = [(PinnedBuffer(batch_frames * self.in_bytes), PinnedBuffer(cap)) for _ in range(depth)]
        outs, flight = [], []

        def drain_one():
            t, got, ob = flight.pop(0)
            self.collect(t)
            outs.append(ob.array[:got * self.out_bytes].copy())

        pos = i = 0
        while pos < n:
            f = min(batch_frames, n - pos)
            if len(flight) == depth:
                drain_one()
            ib, ob = slots[i % depth]
            ib.array[:f * self.in_bytes] = raw[pos * self.in_bytes:(pos + f) * self.in_bytes]
            got, t = self.submit(ib.ptr, f, ob.ptr, cap)
            flight.append((t, got, ob))
            pos += f
            i += 1
        while flight:
            drain_one()
        out = np.concatenate(outs) if outs else np.empty(0, np.uint8)
        return out.view(_NP_VIEW[self.desc.out_format]).copy()

    def reset(self):
        check(self._lib.iqgpu_chain_reset(self._h))

    # ---- marshalling the seamless-sharding calls below share ----
    def _host_input(self, preroll_raw):
        """(pointer or None, frames) of raw frames on the host: a call's input, or a seek's preroll (None: no frames).  The pointer
        keeps the array alive (ndarray.ctypes.data_as)"""
        raw = np.ascontiguousarray(preroll_raw if preroll_raw is not None else np.empty(0, np.uint8))
        n = raw.nbytes // self.in_bytes
        return (raw.ctypes.data_as(C.c_void_p) if n else None), n

    @staticmethod
    def _dc_ptr(state):
        """a DC_STATE record as the POINTER(DcState) the library takes, or None (zero)"""
        if state is None:
            return None
        st = np.zeros((), DC_STATE)
        st[...] = state
        return st.ctypes.data_as(C.POINTER(DcState))

    @staticmethod
    def _agc_ptr(entry):
        return C.byref(entry) if entry is not None else None

    def _agc_rows(self, frames):
        """an empty AGC_ROW table for a call of `frames` input frames: one row per chunk"""
        chunk = int(self.desc.agc_chunk_frames) or 16384
        return np.zeros(-(-int(frames) // chunk), AGC_ROW)

    def _measure(self, fn, ptr, n):
        """measure, dcagc_measure and their _device forms: the rows the call has filled"""
        rows = self._agc_rows(n)
        got = C.c_size_t(0)
        check(fn(self._h, ptr, n, rows.ctypes.data_as(C.c_void_p), rows.size, C.byref(got)))
        return rows[:got.value]

    def _dc_measure(self, fn, first_frame, ptr, n):
        row = np.zeros((), DC_ROW)
        check(fn(self._h, int(first_frame), ptr, n, row.ctypes.data_as(C.POINTER(_lib.DcRow))))
        return row

    def _dcagc_dc_measure(self, fn, first_frame, ptr, n):
        rows = np.zeros(2, DC_ROW)
        got = C.c_size_t(0)
        check(fn(self._h, int(first_frame), ptr, n, rows.ctypes.data_as(C.c_void_p), rows.size, C.byref(got)))
        return rows[:got.value]

    def _dc_measure_range(self, fn, first_frame, ptr, n, call_frames):
        """the three families' range forms and their _device forms: (rows, first_row) -- the DC_ROW records of every grid call of
        the range in order, and the index of every call's first row"""
        n, call_frames = int(n), int(call_frames)
        calls = -(-n // call_frames) if call_frames > 0 else 0
        rows = np.zeros(2 * calls + 1, DC_ROW)              # (a call is at most two pieces)
        first_row = np.zeros(calls + 1, np.uint32)
        got = C.c_size_t(0)
        check(fn(self._h, int(first_frame), ptr, n, call_frames, rows.ctypes.data_as(C.c_void_p), rows.size, C.byref(got),
                 first_row.ctypes.data_as(C.c_void_p)))
        return rows[:got.value], first_row[:calls]

    def _dc_advance(self, fn, state, rows):
        rows = np.ascontiguousarray(rows, DC_ROW).reshape(-1)
        st = np.zeros((), DC_STATE)
        if state is not None:
            st[...] = state
        before = np.zeros(rows.size, DC_STATE)
        check(fn(self._h, st.ctypes.data_as(C.POINTER(DcState)), rows.ctypes.data_as(C.c_void_p) if rows.size else None, rows.size,
                 before.ctypes.data_as(C.c_void_p) if rows.size else None))
        return st, before

    def seek(self, first_frame, preroll_raw=None):
        """puts the chain at frame first_frame of the stream: preroll_raw is a numpy array with the input frames that END at
        first_frame (at least min(first_frame, design_preroll_frames) of them); what the chain emits afterwards is what one chain
        emits behind frames [0, first_frame) (iqgpu_chain_seek)"""
        check(self._lib.iqgpu_chain_seek(self._h, int(first_frame), *self._host_input(preroll_raw)))

    def seek_device(self, first_frame, d_preroll, preroll_frames):
        """seek() with the preroll already in device memory of this chain's GPU (a device address as an int)"""
        check(self._lib.iqgpu_chain_seek_device(self._h, int(first_frame), C.c_void_p(d_preroll), int(preroll_frames)))

    # ---- seamless sharding of digital-AGC chains: measure, walk, seek with the walked state (include/iqgpu.h, ABI v8 / v9) ----
    def measure(self, raw):
        """consumes raw exactly as process() would, emits nothing, leaves the AGC state alone; returns one AGC_ROW record per
        agc_chunk_frames-sized chunk of this call: the peak (squared, double) in front of the gain and the chunk's frames"""
        return self._measure(self._lib.iqgpu_chain_measure, *self._host_input(raw))

    def measure_device(self, d_in, frames_in):
        """measure() with the input already in device memory of this chain's GPU (a device address as an int)"""
        return self._measure(self._lib.iqgpu_chain_measure_device, C.c_void_p(d_in), int(frames_in))

    def measure_submit(self, in_ptr, frames_in, rows_ptr, cap):
        """measure() through the pipeline of submit(): queues one batch (host addresses, preferably pinned; rows_ptr holds cap
        AGC_ROW records) and returns (n_rows, ticket) at once; the rows are there once collect(ticket) returns"""
        got, ticket = C.c_size_t(0), C.c_uint64(0)
        check(self._lib.iqgpu_chain_measure_submit(self._h, C.c_void_p(in_ptr), int(frames_in), C.c_void_p(rows_ptr), int(cap),
                                                   C.byref(got), C.byref(ticket)))
        return got.value, ticket.value

    def measure_pipelined(self, raw, batch_frames):
        """measure() through measure_submit / collect: the stream in batches of batch_frames (each cut into AGC chunks from its
        first frame, like a measure() call of that batch) with up to iqgpu_chain_pipeline_depth() of them in flight, pinned
        buffers on both sides.  Returns the rows of all batches in order."""
        raw = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
        n = raw.nbytes // self.in_bytes
        depth = self._lib.iqgpu_chain_pipeline_depth()
        cap = self._agc_rows(batch_frames).size
        slots = [(PinnedBuffer(batch_frames * self.in_bytes), PinnedBuffer(cap * AGC_ROW.itemsize)) for _ in range(depth)]
        outs, flight = [], []

        def drain_one():
            t, got, rb = flight.pop(0)
            self.collect(t)
            outs.append(rb.array[:got * AGC_ROW.itemsize].view(AGC_ROW).copy())

        pos = i = 0
        while pos < n:
            f = min(batch_frames, n - pos)
            if len(flight) == depth:
                drain_one()
            ib, rb = slots[i % depth]
            ib.array[:f * self.in_bytes] = raw[pos * self.in_bytes:(pos + f) * self.in_bytes]
            got, t = self.measure_submit(ib.ptr, f, rb.ptr, cap)
            flight.append((t, got, rb))
            pos += f
            i += 1
        while flight:
            drain_one()
        return np.concatenate(outs) if outs else np.zeros(0, AGC_ROW)

    def agc_initial_state(self):
        """the AGC state of a fresh stream as an AgcState (what agc_advance and seek_agc take)"""
        st = AgcState()
        check(self._lib.iqgpu_chain_agc_initial_state(self._h, C.byref(st)))
        return st

    def agc_advance(self, state, rows, gains=False):
        """agc_apply's state machine over a table of measure() rows: returns the AgcState behind them (state itself is not
        changed), or (state, gains) with the gain every row is multiplied with"""
        rows = np.ascontiguousarray(rows, AGC_ROW)
        st = AgcState.from_buffer_copy(bytes(state))
        g = np.zeros(rows.size, np.float32) if gains else None
        check(self._lib.iqgpu_chain_agc_advance(self._h, C.byref(st), rows.ctypes.data_as(C.c_void_p) if rows.size else None, rows.size,
                                                g.ctypes.data_as(C.c_void_p) if gains and rows.size else None))
        return (st, g) if gains else st

    def seek_agc(self, first_frame, preroll_raw=None, entry=None):
        """seek() for a chain with the digital AGC: the preroll runs with the AGC out of the way, then the chain carries `entry`
        (an AgcState from agc_advance) as its AGC state; entry None leaves the fresh state, which is all a measuring chain needs"""
        check(self._lib.iqgpu_chain_seek_agc(self._h, int(first_frame), *self._host_input(preroll_raw), self._agc_ptr(entry)))

    def seek_agc_device(self, first_frame, d_preroll, preroll_frames, entry=None):
        check(self._lib.iqgpu_chain_seek_agc_device(self._h, int(first_frame), C.c_void_p(d_preroll), int(preroll_frames), self._agc_ptr(entry)))

    # ---- seamless sharding of dx / local AGC chains: a bounded window, certified at the seam (include/iqgpu.h) ----
    def seek_rms(self, first_frame, preroll_raw=None):
        """seek() for a chain with the dx / local AGC: preroll_raw holds the input frames that END at first_frame, at least
        min(first_frame, design_preroll_frames_rms) of them; the AGC loop's state at first_frame is rebuilt from the preroll's own
        output.  The seam is certified when agc_state_raw() right after this call equals, in gain, peak_memory and samples_seen, the
        state of the chain that processed the range in front; otherwise load_state() that chain's blob and process the range again"""
        check(self._lib.iqgpu_chain_seek_rms(self._h, int(first_frame), *self._host_input(preroll_raw)))

    def seek_rms_device(self, first_frame, d_preroll, preroll_frames):
        """seek_rms() with the preroll already in device memory of this chain's GPU (a device address as an int)"""
        check(self._lib.iqgpu_chain_seek_rms_device(self._h, int(first_frame), C.c_void_p(d_preroll), int(preroll_frames)))

    # ---- exact seamless sharding of DC-blocker chains: measure, walk, seek with the walked state (include/iqgpu.h) ----
    def dc_state(self):
        """the DC blocker's state behind the last call as a DC_STATE record, every bit of it (synchronises)"""
        st = np.zeros((), DC_STATE)
        check(self._lib.iqgpu_chain_get_dc_state(self._h, st.ctypes.data_as(C.POINTER(DcState))))
        return st

    def dc_measure(self, first_frame, raw):
        """the map v_after = f v_before + g of the call process(raw) would be at stream frame first_frame, as a DC_ROW record;
        the chain itself stays exactly as it was"""
        return self._dc_measure(self._lib.iqgpu_chain_dc_measure, first_frame, *self._host_input(raw))

    def dc_measure_device(self, first_frame, d_in, frames_in):
        """dc_measure() with the input already in device memory of this chain's GPU (a device address as an int)"""
        return self._dc_measure(self._lib.iqgpu_chain_dc_measure_device, first_frame, C.c_void_p(d_in), int(frames_in))

    def dc_measure_range(self, first_frame, raw, call_frames):
        """dc_measure() of every grid call of a range in one submission: raw holds the frames from stream frame first_frame (a
        multiple of call_frames) on, cut into calls of call_frames (the last may be shorter).  Returns (rows, first_row): the rows a
        dc_measure() loop over those calls gives, bit for bit, and the index of every call's first row"""
        return self._dc_measure_range(self._lib.iqgpu_chain_dc_measure_range, first_frame, *self._host_input(raw), call_frames)

    def dc_measure_range_device(self, first_frame, d_in, frames_in, call_frames):
        """dc_measure_range() with the range already in device memory of this chain's GPU (a device address as an int)"""
        return self._dc_measure_range(self._lib.iqgpu_chain_dc_measure_range_device, first_frame, C.c_void_p(d_in), frames_in, call_frames)

    def dc_advance(self, state, rows):
        """walks a DC state (a DC_STATE record, or None for zero) over dc_measure() rows on the device: returns (state behind the
        last row, before) where before[k] is the state in front of row k"""
        return self._dc_advance(self._lib.iqgpu_chain_dc_advance, state, rows)

    def seek_dc(self, first_frame, preroll_raw=None, call_frames=0, state=None):
        """seek() for a chain with the DC blocker, exact: the preroll is only the filters' memory, it runs in calls of call_frames
        (0: one call) and `state` (a DC_STATE record from dc_advance; None: zero) is the blocker's state in front of it"""
        check(self._lib.iqgpu_chain_seek_dc(self._h, int(first_frame), *self._host_input(preroll_raw), int(call_frames), self._dc_ptr(state)))

    def seek_dc_device(self, first_frame, d_preroll, preroll_frames, call_frames=0, state=None):
        check(self._lib.iqgpu_chain_seek_dc_device(self._h, int(first_frame), C.c_void_p(d_preroll), int(preroll_frames), int(call_frames),
                                                   self._dc_ptr(state)))

    # ---- exact seamless sharding of chains with the DC blocker AND the digital AGC (include/iqgpu.h, iqgpu_chain_dcagc_*) ----
    def dcagc_dc_measure(self, first_frame, raw):
        """the DC maps of the call process(raw) would be at stream frame first_frame: DC_ROW records, ONE PER PIECE (two for the
        call the stream cuts at the AGC's lock), in order; the chain itself stays exactly as it was"""
        return self._dcagc_dc_measure(self._lib.iqgpu_chain_dcagc_dc_measure, first_frame, *self._host_input(raw))

    def dcagc_dc_measure_device(self, first_frame, d_in, frames_in):
        """dcagc_dc_measure() with the input already in device memory of this chain's GPU (a device address as an int)"""
        return self._dcagc_dc_measure(self._lib.iqgpu_chain_dcagc_dc_measure_device, first_frame, C.c_void_p(d_in), int(frames_in))

    def dcagc_dc_measure_range(self, first_frame, raw, call_frames):
        """dcagc_dc_measure() of every grid call of a range in one submission: (rows, first_row) with ONE ROW PER PIECE, the rows of
        call k from first_row[k] on -- the rows of a dcagc_dc_measure() loop, bit for bit"""
        return self._dc_measure_range(self._lib.iqgpu_chain_dcagc_dc_measure_range, first_frame, *self._host_input(raw), call_frames)

    def dcagc_dc_measure_range_device(self, first_frame, d_in, frames_in, call_frames):
        """dcagc_dc_measure_range() with the range already in device memory of this chain's GPU (a device address as an int)"""
        return self._dc_measure_range(self._lib.iqgpu_chain_dcagc_dc_measure_range_device, first_frame, C.c_void_p(d_in), frames_in,
                                      call_frames)

    def dcagc_dc_advance(self, state, rows):
        """dc_advance() for these chains: (state behind the last row, before) with before[k] the state in front of row k"""
        return self._dc_advance(self._lib.iqgpu_chain_dcagc_dc_advance, state, rows)

    def dcagc_seek(self, first_frame, preroll_raw=None, call_frames=0, dc_state=None, entry=None):
        """puts the chain at first_frame, exact in both states: `dc_state` (a DC_STATE record from dcagc_dc_advance; None: zero) is
        the blocker's state in front of the preroll, which runs as shadow calls of call_frames (0: one call); then the chain carries
        `entry` (an AgcState from agc_advance; None: the fresh state, for a measuring chain)"""
        check(self._lib.iqgpu_chain_dcagc_seek(self._h, int(first_frame), *self._host_input(preroll_raw), int(call_frames),
                                               self._dc_ptr(dc_state), self._agc_ptr(entry)))

    def dcagc_seek_device(self, first_frame, d_preroll, preroll_frames, call_frames=0, dc_state=None, entry=None):
        check(self._lib.iqgpu_chain_dcagc_seek_device(self._h, int(first_frame), C.c_void_p(d_preroll), int(preroll_frames), int(call_frames),
                                                      self._dc_ptr(dc_state), self._agc_ptr(entry)))

    def dcagc_measure(self, raw):
        """the AGC_ROW records of the call process(raw) would be at the chain's position, as a shadow call: consumes raw like
        process() (position, histories, DC state), emits nothing, leaves the AGC state alone"""
        return self._measure(self._lib.iqgpu_chain_dcagc_measure, *self._host_input(raw))

    def dcagc_measure_device(self, d_in, frames_in):
        """dcagc_measure() with the input already in device memory of this chain's GPU (a device address as an int)"""
        return self._measure(self._lib.iqgpu_chain_dcagc_measure_device, C.c_void_p(d_in), int(frames_in))

    # ---- exact seamless sharding of chains with the DC blocker AND the dx / local AGC (include/iqgpu.h, iqgpu_chain_dcrms_*) ----
    def dcrms_dc_measure(self, first_frame, raw):
        """dc_measure() for these chains: the map of the call process(raw) would be at stream frame first_frame, ONE DC_ROW record
        (a dx / local chain never cuts a call); the chain itself stays exactly as it was"""
        return self._dc_measure(self._lib.iqgpu_chain_dcrms_dc_measure, first_frame, *self._host_input(raw))

    def dcrms_dc_measure_device(self, first_frame, d_in, frames_in):
        """dcrms_dc_measure() with the input already in device memory of this chain's GPU (a device address as an int)"""
        return self._dc_measure(self._lib.iqgpu_chain_dcrms_dc_measure_device, first_frame, C.c_void_p(d_in), int(frames_in))

    def dcrms_dc_measure_range(self, first_frame, raw, call_frames):
        """dcrms_dc_measure() of every grid call of a range in one submission: (rows, first_row), one row per call"""
        return self._dc_measure_range(self._lib.iqgpu_chain_dcrms_dc_measure_range, first_frame, *self._host_input(raw), call_frames)

    def dcrms_dc_measure_range_device(self, first_frame, d_in, frames_in, call_frames):
        """dcrms_dc_measure_range() with the range already in device memory of this chain's GPU (a device address as an int)"""
        return self._dc_measure_range(self._lib.iqgpu_chain_dcrms_dc_measure_range_device, first_frame, C.c_void_p(d_in), frames_in,
                                      call_frames)

    def dcrms_dc_advance(self, state, rows):
        """dc_advance() for these chains: (state behind the last row, before) with before[k] the state in front of row k"""
        return self._dc_advance(self._lib.iqgpu_chain_dcrms_dc_advance, state, rows)

    def dcrms_seek(self, first_frame, preroll_raw=None, call_frames=0, dc_state=None):
        """puts the chain at first_frame: `dc_state` (a DC_STATE record from dcrms_dc_advance; None: zero) is the blocker's state in
        front of the preroll, which runs in calls of call_frames (0: one call) with the AGC out of the way; the AGC loop's state at
        first_frame is then rebuilt from the preroll's own output, as by seek_rms -- and certified at the seam in the same way"""
        check(self._lib.iqgpu_chain_dcrms_seek(self._h, int(first_frame), *self._host_input(preroll_raw), int(call_frames),
                                               self._dc_ptr(dc_state)))

    def dcrms_seek_device(self, first_frame, d_preroll, preroll_frames, call_frames=0, dc_state=None):
        """dcrms_seek() with the preroll already in device memory of this chain's GPU (a device address as an int)"""
        check(self._lib.iqgpu_chain_dcrms_seek_device(self._h, int(first_frame), C.c_void_p(d_preroll), int(preroll_frames), int(call_frames),
                                                      self._dc_ptr(dc_state)))

    # ---- checkpoint / resume (include/iqgpu.h): the whole carried state in a blob, into a chain of the same description ----
    def tell(self):
        """(frames_in, frames_out) since the last reset -- after a seek: of the stream -- behind every batch already submitted"""
        fi, fo = C.c_uint64(0), C.c_uint64(0)
        check(self._lib.iqgpu_chain_tell(self._h, C.byref(fi), C.byref(fo)))
        return int(fi.value), int(fo.value)

    def state_size(self):
        """bytes of this chain's saved state: fixed per description (a size query of iqgpu_chain_save_state)"""
        n = C.c_size_t(0)
        rc = self._lib.iqgpu_chain_save_state(self._h, None, 0, C.byref(n))
        if rc != -8:                # IQGPU_ECAPACITY is the answer of a size query
            check(rc)
        return int(n.value)

    def save_state(self):
        """everything the chain carries from call to call, as bytes; the chain itself continues as if it had not been asked"""
        buf = C.create_string_buffer(self.state_size())
        n = C.c_size_t(0)
        check(self._lib.iqgpu_chain_save_state(self._h, buf, len(buf), C.byref(n)))
        return buf.raw[:n.value]

    def load_state(self, blob):
        """puts a save_state() blob of a chain of the same description into this chain: it continues that chain's stream byte for
        byte.  A refused blob (IqgpuError, EINVAL) leaves this chain exactly as it was."""
        blob = bytes(blob)
        check(self._lib.iqgpu_chain_load_state(self._h, blob, len(blob)))

    def agc_state_raw(self):
        """the chain's AGC state as an AgcState structure: every field with its bits (synchronises)"""
        st = AgcState()
        check(self._lib.iqgpu_chain_get_agc_state(self._h, C.byref(st)))
        return st

    def agc_state(self):
        """dict of the AGC fields the reference keeps in AppResources (synchronises)"""
        st = AgcState()
        check(self._lib.iqgpu_chain_get_agc_state(self._h, C.byref(st)))
        return dict(locked=bool(st.locked), peak_memory=st.peak_memory, gain=st.current_gain,
                    last_strong_peak_time=st.last_strong_peak_time, samples_seen=st.samples_seen)

    def set_iq_factors(self, mag, phase):
        check(self._lib.iqgpu_chain_set_iq_factors(self._h, mag, phase))

    def enable_iq_probe(self, on=True):
        check(self._lib.iqgpu_chain_enable_iq_probe(self._h, int(on)))

    def read_iq_probe(self):
        """the block the reference hands its optimiser (src/pipeline.c:468-476): first 1024 pre-processed samples of the first
        ordinary call (process, process_device, submit) of >= 1024 frames since the previous read -- then that block until a later
        call has left the next one -- or None: none yet, or dropped by reset / seek* / load_state (the rules in include/iqgpu.h)"""
        blk = np.empty(1024, np.complex64)
        valid = C.c_int(0)
        check(self._lib.iqgpu_chain_read_iq_probe(self._h, blk.ctypes.data_as(C.c_void_p), C.byref(valid)))
        return blk if valid.value else None

    # ---- I/Q calibration (include/iqgpu.h): the optimiser's utility over many blocks of the input and a grid of candidates ----
    def _calibrate_iq(self, fn, ptr, n, opts):
        from .iq_optimizer import IqCalibration, calib_opts
        o = calib_opts(**opts)
        rep = _lib.IqCalibReport()
        check(fn(self._h, ptr, n, C.byref(o), C.byref(rep)))
        return IqCalibration(rep, o)

    def _calibrate_iq_blocks(self, fn, ptr, n, max_blocks):
        cap = max(1, min(int(max_blocks), n // 1024))
        blocks = np.empty((cap, 1024), np.complex64)
        got = C.c_size_t(0)
        check(fn(self._h, ptr, n, int(max_blocks), blocks.ctypes.data_as(C.c_void_p), cap, C.byref(got)))
        return blocks[:got.value]

    def calibrate_iq(self, raw, **opts):
        """one (mag, phase) pair for this input, a pure function of its bytes and the options: the deterministic grid search of the
        optimiser's utility over up to max_blocks blocks of raw (frames in in_format), evaluated on the GPU.  Returns an
        IqCalibration; the chain itself stays exactly as it was -- publish the result with set_iq_factors or in the description"""
        return self._calibrate_iq(self._lib.iqgpu_chain_calibrate_iq, *self._host_input(raw), opts)

    def calibrate_iq_device(self, d_in, frames_in, **opts):
        """calibrate_iq() with the input already in device memory of this chain's GPU (a device address as an int)"""
        return self._calibrate_iq(self._lib.iqgpu_chain_calibrate_iq_device, C.c_void_p(d_in), int(frames_in), opts)

    def calibrate_iq_blocks(self, raw, max_blocks=64):
        """the cf32 blocks calibrate_iq() evaluates, [n, 1024]: behind unpack, gain and the DC blocker from a zero state"""
        return self._calibrate_iq_blocks(self._lib.iqgpu_chain_calibrate_iq_blocks, *self._host_input(raw), max_blocks)

    def calibrate_iq_blocks_device(self, d_in, frames_in, max_blocks=64):
        return self._calibrate_iq_blocks(self._lib.iqgpu_chain_calibrate_iq_blocks_device, C.c_void_p(d_in), int(frames_in), max_blocks)

    # ---- plumbing ----
    def set_stream(self, hip_stream):
        check(self._lib.iqgpu_chain_set_stream(self._h, C.c_void_p(hip_stream)))

    def get_stream(self):
        return self._lib.iqgpu_chain_get_stream(self._h)

    def synchronize(self):
        check(self._lib.iqgpu_chain_synchronize(self._h))

    def set_profiling(self, on=True):
        check(self._lib.iqgpu_chain_set_profiling(self._h, int(on)))

    def front_kernel(self):
        """name of the front kernel the last process call launched (iqgpu_chain_front_kernel)"""
        return self._lib.iqgpu_chain_front_kernel(self._h).decode()

    def profile(self):
        p = Profile()
        check(self._lib.iqgpu_chain_get_profile(self._h, C.byref(p)))
        return {name: dict(launches=int(p.launches[i]), ms=float(p.ms[i]))
                for i, name in enumerate(_lib.K_NAMES)}


class PinnedBuffer:
    """hipHostMalloc'd (page-locked) host buffer with a numpy view, for submit() / collect()."""

    def __init__(self, nbytes):
        self._lib = _lib.load()
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        check(self._lib.iqgpu_host_malloc_pinned(self.nbytes, C.byref(p)))
        self.ptr = p.value
        self.array = np.ctypeslib.as_array((C.c_uint8 * max(self.nbytes, 1)).from_address(self.ptr))[:self.nbytes]

    def free(self):
        if getattr(self, "ptr", None):
            self.array = None
            self._lib.iqgpu_host_free_pinned(C.c_void_p(self.ptr))
            self.ptr = None

    __del__ = free


class DeviceBuffer:
    """hipMalloc'd buffer through the C ABI (for hosts without their own HIP binding)."""

    def __init__(self, nbytes, device=0):
        self._lib = _lib.load()
        self.device, self.nbytes = device, int(nbytes)
        p = C.c_void_p()
        check(self._lib.iqgpu_device_malloc(device, self.nbytes, C.byref(p)))
        self.ptr = p.value

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        check(self._lib.iqgpu_memcpy_h2d(self.device, C.c_void_p(self.ptr), arr.ctypes.data_as(C.c_void_p), arr.nbytes))

    def download(self, nbytes=None, dtype=np.uint8):
        nbytes = self.nbytes if nbytes is None else int(nbytes)
        out = np.empty(nbytes, np.uint8)
        check(self._lib.iqgpu_memcpy_d2h(self.device, out.ctypes.data_as(C.c_void_p), C.c_void_p(self.ptr), nbytes))
        return out.view(dtype)

    def free(self):
        if getattr(self, "ptr", None):
            self._lib.iqgpu_device_free(self.device, C.c_void_p(self.ptr))
            self.ptr = None

    __del__ = free
