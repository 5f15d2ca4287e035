"""The device code's one definition of each sample format, seen from outside (dsp_device.hpp: pack_b16 / pack_b8 behind pack_store and
pack_store_group, unpack_b16 / unpack_b8 behind unpack_four_fast and k_dc_prefix's streaming loop).

  * k_front's no-resampler path stores a thread's four frames as one piece where all four are new and frame by frame elsewhere: both
    must be the reference's convert_cf32_to_block, byte for byte, in every output format, on calls that hold whole quads, a ragged
    tail and fewer frames than a quad.
  * k_dc_prefix reads long, aligned segments of 16-bit and 8-bit frames with several vector loads in flight and everything else
    frame by frame: the same frames from an aligned and from an unaligned buffer must give the same bytes.
"""
import numpy as np
import pytest

from iq_tool_amd import synth

pytestmark = pytest.mark.gpu

TOL = 1e-5                                                  # cf32 results of liquid-derived operators (test_gpu_parity.py, test_dc_block_operator)
GUARD = 64                                                  # bytes behind the last frame that no store may touch

# (scale, offset, lowest code, highest code): src/sample_convert.c:213-309
PACK = {"cs8": (127.0, 0.0, -128.0, 127.0), "cu8": (127.0, 127.5, 0.0, 255.0),
        "cs16": (32767.0, 0.0, -32768.0, 32767.0), "cu16": (32767.0, 32767.5, 0.0, 65535.0), "sc16q11": (2048.0, 0.0, -32768.0, 32767.0),
        "cs24": (8388607.0, 0.0, -8388608.0, 8388607.0), "cs32": (2147483647.0, 0.0, -2147483648.0, 2147483647.0),
        "cu32": (2147483647.0, 2147483647.5, 0.0, 4294967295.0), "cf32": (1.0, 0.0, -1.0, 1.0)}
CALLS = [4099, 6, 3, 1]                                     # two interior tiles + a 3-frame tile; a quad + 2; less than a quad; one frame
RATE = 2.4e6


def grid(fmt):
    """finite cf32 frames for sum(CALLS) frames: a 1/64 grid over [-1.5, 1.5] (0 and +-1 are on it), -0.0, both sides of the format's
    two clamps (for sc16q11 they sit at +-16, beyond the grid) and the (k + 0.5) / scale ties, every value at several positions of a quad"""
    scale, off, lo, hi = PACK[fmt]
    f32 = np.float32
    up, down = f32(np.inf), f32(-np.inf)
    vals = [np.arange(-96, 97, dtype=np.float32) / f32(64), np.array([0.0, -0.0, 1.0, -1.0], np.float32)]
    clamps = np.array([(lo - off) / scale, (hi - off) / scale, (lo - off - 0.5) / scale, (hi - off + 0.5) / scale,
                       (lo - off + 1.0) / scale, (hi - off - 1.0) / scale], np.float64).astype(np.float32)
    ties = (np.arange(-40, 40, dtype=np.float32) + f32(0.5)) / f32(scale)
    for v in (clamps, ties):
        vals += [v, np.nextafter(v, up), np.nextafter(v, down)]
    vals = np.concatenate(vals)
    assert np.isfinite(vals).all()
    n = sum(CALLS)
    i = np.arange(n)
    x = np.empty(n, np.complex64)
    x.real = vals[i % vals.size]
    x.imag = vals[(7 * i + 3) % vals.size]
    assert n >= 4 * vals.size                               # every value in every lane of a quad, as a real part
    return x


def run_calls(gpu, kw, x, calls, in_offset=0):
    """the chain over the frames of x (any dtype, whole frames) in the given calls, device to device, the input in_offset bytes behind a
    16-byte boundary, every call's output right behind the last one's in one buffer filled with a pattern.  (bytes, front kernel)"""
    from iq_tool_amd.chain import DeviceBuffer
    ch = gpu.Chain(**kw)
    ibpf, obpf = ch.in_bytes, ch.out_bytes
    raw = np.ascontiguousarray(x).view(np.uint8)
    assert raw.size == sum(calls) * ibpf
    cap = sum(ch.max_out_frames(k) for k in calls) * obpf + GUARD
    d_in, d_out = DeviceBuffer(raw.size + 16), DeviceBuffer(cap)
    try:
        assert d_in.ptr % 16 == 0
        d_in.upload(np.concatenate([np.zeros(in_offset, np.uint8), raw]))
        d_out.upload(np.full(cap, 0xA5, np.uint8))
        pos = done = 0
        for k in calls:
            got = ch.process_device(d_in.ptr + in_offset + pos * ibpf, k, d_out.ptr + done * obpf, cap - GUARD - done * obpf)
            assert got == k                                 # no resampler: frames map one to one
            pos += k
            done += got
        ch.synchronize()
        out = d_out.download(done * obpf + GUARD)
        kernel = ch.front_kernel()
    finally:
        d_in.free(); d_out.free()
    assert (out[done * obpf:] == 0xA5).all(), "a store behind the last frame"
    return out[:done * obpf].copy(), kernel


def plain_desc(fmt, shifted):
    # cf32 in, no resampler (the target rate is the input rate), no pre-shift, no DC blocker, no I/Q correction, gain 1
    kw = dict(in_format="cf32", out_format=fmt, input_rate_hz=RATE, target_rate_hz=RATE, no_resample=True)
    if shifted:
        kw.update(shift_hz=200e3, shift_after_resample=True)
    return kw


@pytest.mark.parametrize("fmt", sorted(PACK))
def test_group_store_is_the_reference_pack(gpu, oracle, fmt):
    """the chain's cf32 output is its input, so its output in `fmt` is the reference's pack of the input: whole quads (one vector store),
    the ragged tail and the short calls (pack_store frame by frame) alike"""
    x = grid(fmt)
    got, kernel = run_calls(gpu, plain_desc(fmt, False), x, CALLS)
    assert kernel == "k_front"
    if fmt != "cf32":
        same, _ = run_calls(gpu, plain_desc("cf32", False), x, CALLS)
        assert np.array_equal(same, x.view(np.uint8))       # (what the comparison below rests on: cf32 out is cf32 in, -0.0 included)
    want = oracle.from_cf32(x, fmt).view(np.uint8)
    assert got.size == want.size
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (fmt, bad[:8], got[bad[:8]], want[bad[:8]])


_shifted_twin = {}


@pytest.mark.parametrize("fmt", ["cs16", "cu8", "cf32"])
def test_group_store_behind_the_post_shift(gpu, oracle, fmt):
    """with the post mixer in front of the store the frames are no longer the input: the format's bytes are the reference's pack of
    the chain's own cf32 output"""
    x = grid(fmt)
    if fmt not in _shifted_twin:
        twin, kernel = run_calls(gpu, plain_desc("cf32", True), x, CALLS)
        assert kernel == "k_front"
        frames = twin.view(np.complex64)
        assert np.isfinite(frames.view(np.float32)).all() and not np.array_equal(frames, x)
        _shifted_twin[fmt] = frames
    frames = _shifted_twin[fmt]
    got, kernel = run_calls(gpu, plain_desc(fmt, True), x, CALLS)
    assert kernel == "k_front"
    want = oracle.from_cf32(frames, fmt).view(np.uint8)
    assert got.size == want.size
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (fmt, bad[:8], got[bad[:8]], want[bad[:8]])


# k_dc_prefix, one workgroup per segment (kernels.hpp dc_seg_start, mode 0: the blocks of k_front).  block_samples = 32768 makes a block
# 16 tiles of 2048 frames, and a chain without a resampler has no warm-up tile and no group remainder, so dc_seg_start(s) = 32768 s.
# The first call's 32768 + 22 * 1024 + 40 frames are two segments:
#   [0, 32768)       32 chunks of 1024, none padded: chunk 0, then 7 rounds of four (16-bit) / 3 rounds of eight (8-bit), then the tail
#   [32768, 55336)   22568 frames = 23 chunks, the first one padded with 984 zeros: the padded chunk, 5 rounds of four and a tail of 2
#                    (16-bit) / 2 rounds of eight and a tail of 6 (8-bit) -- beyond both thresholds (more than 5 / more than 9 chunks)
# The streaming loop wants the padded segment to start on a 16-byte boundary, that is the segment to END on one: the odd frames are 40
# (a multiple of 8 frames: 16 bytes of an 8-bit format), not 37.  The first segment's aggregate is the second one's state inside the call;
# the second one's is the stream's state behind the call, which the 2053 frames of the second call show.
DC_BLOCK = 32768
DC_CALLS = [DC_BLOCK + 22 * 1024 + 40, 2048 + 5]


@pytest.mark.parametrize("fmt", ["cs16", "cu16", "sc16q11", "cu8", "cs8"])
def test_dc_prefix_streaming_loop_is_the_general_loop(gpu, oracle, fmt):
    n = sum(DC_CALLS)
    raw = synth.raw_stream(n, RATE, 23, fmt)
    kw = dict(in_format=fmt, out_format="cf32", input_rate_hz=RATE, target_rate_hz=RATE, no_resample=True, dc_block=True)
    bpf = raw.nbytes // n
    assert (DC_CALLS[0] * bpf) % 16 == 0 and DC_CALLS[0] % 1024 != 0
    aligned, kernel = run_calls(gpu, dict(kw, block_samples=DC_BLOCK), raw, DC_CALLS)
    assert kernel == "k_front"
    # the same frames one frame behind a 16-byte boundary: no vector load anywhere, every frame through the any-alignment path
    shifted, _ = run_calls(gpu, dict(kw, block_samples=DC_BLOCK), raw, DC_CALLS, in_offset=bpf)
    assert np.array_equal(aligned, shifted), np.flatnonzero(aligned != shifted)[:8] // 8
    want = oracle.Chain(**kw).process(raw).view(np.complex64)
    got = aligned.view(np.complex64)
    assert got.size == want.size == n
    err = float(np.abs(got - want).max())
    print("dc_prefix %s: max |gpu - oracle| = %.3g" % (fmt, err))
    assert err <= TOL
