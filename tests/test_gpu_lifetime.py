"""Create, use, destroy: free device memory comes back, once per group of device resources a handle owns.

The chain and accumulator handles hold their device resources in owning members (DevBuf, DevMem, HostMem, Event, Stream in
csrc/chain.hpp) that free themselves when the handle is deleted.  A member that did not would leak on every destroy and nothing
else in the suite would notice, so each case below builds one handle, makes one small call that touches the lazily created
resources the case is about, and destroys it -- once unmeasured, so that the runtime's own first-use allocations are out of the
picture, then R = 64 times between two readings of free device memory behind a device synchronise.  64 rounds turn the
smallest single resource (the 64 KB diagnostic scratch, d_sink) into 4 MB.

The reading is hipMemGetInfo -- what torch.cuda.mem_get_info returns -- called on the HIP runtime libiqgpu.so has loaded: torch
cannot initialise its device in a process where libiqgpu.so was loaded first (bench.py, which needs both, imports torch first for
that reason), and in the suite it always was.

The bar: profiles/lifetime_refactor.md.  The same cases on the commit before the owners (a hand-kept release list) drifted by
0 bytes in every case, and free memory as hipMalloc hands it out moved in steps of 2 MiB there; the bar is that largest drift
plus one such step, and a drift has to stay below it: a single step gone is a leak already.

Calls are 4096 input frames for the chains.  The accumulators take nfft = 1024, 2048 or 4096 only, so their push is 16 x nfft
frames at nfft = 1024, the smallest they accept.

What this cannot see: events and streams do not show in free memory.  For them the guarantee is the member's type -- no host
source outside the owners destroys an event or a stream by hand -- and no stand-in is measured here."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

R = 64
GRANULE = 2 << 20                  # step of free memory per hipMalloc as observed (profiles/lifetime_refactor.md)
PARENT_MAX_DRIFT = 0               # largest drift of any case on the parent commit (same file)
BAR = PARENT_MAX_DRIFT + GRANULE
FRAMES = 4096
RATE = 2.4e6
S1 = dict(input_rate_hz=RATE, target_rate_hz=RATE / (1.6125 * 2))


def cs16(n, seed=1):
    return np.random.default_rng(seed).integers(-20000, 20000, 2 * n).astype(np.int16)


RAW = cs16(FRAMES)


def with_chain(gpu, use=lambda ch: ch.process(RAW), **kw):
    ch = gpu.Chain(**kw)
    try:
        use(ch)
    finally:
        ch.close()


def plain(gpu):
    with_chain(gpu, **S1)


def cascade(gpu):                  # S = 3 without a DC blocker: k_cascade in front (d_hist2, mid)
    with_chain(gpu, input_rate_hz=RATE, target_rate_hz=RATE / (1.6125 * 8))


def interp(gpu):                   # r >= 1: k_interp (ibuf, d_ihb)
    with_chain(gpu, input_rate_hz=1.0e6, target_rate_hz=2.5e6)


def fft_filter(gpu):               # overlap-save (d_hfreq, d_twiddle, fbuf)
    with_chain(gpu, filters=(("lowpass", 200e3, 0.0),), filter_taps=129, filter_impl="fft", **S1)


def agc_digital(gpu):              # flag, mapped verdict word, peak arrays
    with_chain(gpu, agc=True, agc_profile="digital", **S1)


def agc_dx(gpu):                   # agc_hist
    with_chain(gpu, agc=True, agc_profile="dx", **S1)


def dc_range(gpu):                 # the host variant over three slices of one call each: both staging slices, copy stream, events
    def use(ch):
        ch.process(RAW)
        rows, _ = ch.dc_measure_range(0, cs16(3 * FRAMES), FRAMES)
        assert rows.size == 3
    with_chain(gpu, use, dc_block=True, **S1)


def pipeline(gpu):                 # one submit / collect round trip: slots, eight copy streams
    def use(ch):
        cap = ch.max_out_frames(FRAMES) * ch.out_bytes
        ib, ob = gpu.PinnedBuffer(RAW.nbytes), gpu.PinnedBuffer(cap)
        try:
            ib.array[:] = RAW.view(np.uint8)
            _, ticket = ch.submit(ib.ptr, FRAMES, ob.ptr, cap)
            ch.collect(ticket)
        finally:
            ch.synchronize()
            ib.free(); ob.free()
    with_chain(gpu, use, **S1)


def iq_probe(gpu):
    def use(ch):
        ch.enable_iq_probe(True)
        ch.process(RAW)
        assert ch.read_iq_probe() is not None
    with_chain(gpu, use, **S1)


def profiling(gpu):                # event pool
    def use(ch):
        ch.set_profiling(True)
        ch.process(RAW)
        assert sum(k["launches"] for k in ch.profile().values()) > 0
    with_chain(gpu, use, **S1)


def psd(gpu):
    with gpu.Psd("cs16", nfft=1024) as p:
        p.push(cs16(16 * 1024))
        assert p.read()[2]["segments"] > 0


def sgram(gpu):
    with gpu.Sgram("cs16", nfft=1024, row_segments=4) as s:
        s.push(cs16(16 * 1024))


CASES = [plain, cascade, interp, fft_filter, agc_digital, agc_dx, dc_range, pipeline, iq_probe, profiling, psd, sgram]


def hip_runtime():
    """the HIP runtime this process has loaded (libiqgpu.so's), as a ctypes library"""
    with open("/proc/self/maps") as maps:
        path = next(line.split()[-1] for line in maps if "libamdhip64" in line)
    return C.CDLL(path)


def free_bytes():
    hip = hip_runtime()
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipDeviceSynchronize() == 0
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


@pytest.mark.parametrize("case", CASES, ids=lambda f: f.__name__)
def test_destroy_gives_the_device_memory_back(gpu, monkeypatch, case):
    monkeypatch.setenv("IQGPU_DC_RANGE_SLICE_FRAMES", str(FRAMES))     # (dc_range: a staging slice is one call; no other case reads it)
    case(gpu)                      # unmeasured: first-use allocations of the runtime and of the library
    before = free_bytes()
    for _ in range(R):
        case(gpu)
    drift = before - free_bytes()
    print("lifetime %-12s drift %d bytes over %d rounds (bar %d)" % (case.__name__, drift, R, BAR))
    assert drift < BAR, "%s: %d bytes of device memory gone after %d create / use / destroy rounds" % (case.__name__, drift, R)
