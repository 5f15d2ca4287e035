#!/usr/bin/env python3
"""Time of the power-spectrum accumulator (Psd.push_device: k_psd_pages + k_psd_fold + k_psd_carry) on a resident cs16 buffer, for each
nfft at hop = nfft / 2 and the Hann window.  A recorded measurement, not a bar:

    timeout -k 10 600 python tools/bench_psd.py [--log2-frames 28] [--reps 5] [--out profiles/psd.json]

The buffer is 2^28 frames (1 GiB) of the counter-hash stream, uploaded once; every repetition pushes the whole buffer in one call into
a reset accumulator, timed with events on a stream of its own (the first push of each size -- allocations -- is reported apart and
not in the median).  Per size: ms, MS/s, and the ratio to the bare HBM read time of those bytes at the 8 TB/s of the project's
roofline."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-frames", type=int, default=28)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import iq_tool_amd
    from iq_tool_amd import _lib, synth
    from iq_tool_amd._lib import check
    lib = iq_tool_amd.load()
    frames = 1 << a.log2_frames
    d = iq_tool_amd.DeviceBuffer(frames * 4)
    piece = 1 << 24                                        # generated and uploaded in pieces
    for at in range(0, frames, piece):
        n = min(piece, frames - at)
        raw = synth.hash_stream(n, 1, "cs16", first=at)
        check(lib.iqgpu_memcpy_h2d(0, C.c_void_p(d.ptr + at * 4), raw.ctypes.data_as(C.c_void_p), raw.nbytes))
    stream, e0, e1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    check(lib.iqgpu_stream_create(0, C.byref(stream)))
    check(lib.iqgpu_event_create(C.byref(e0)))
    check(lib.iqgpu_event_create(C.byref(e1)))
    floor_ms = frames * 4 / HBM_BYTES_PER_S * 1e3
    rows = []
    for nfft in (1024, 2048, 4096):
        acc = iq_tool_amd.Psd("cs16", nfft=nfft, hop=nfft // 2)

        def timed():
            acc.reset()
            check(lib.iqgpu_event_record(e0, stream))
            acc.push_device(d.ptr, frames, stream.value)
            check(lib.iqgpu_event_record(e1, stream))
            check(lib.iqgpu_stream_synchronize(stream))
            ms = C.c_float(0)
            check(lib.iqgpu_event_elapsed_ms(e0, e1, C.byref(ms)))
            return float(ms.value)

        first = timed()
        ms = [timed() for _ in range(a.reps)]
        s, _, info = acc.read()
        med = statistics.median(ms)
        rows.append(dict(nfft=nfft, hop=nfft // 2, window="hann", format="cs16", frames=frames, segments=info["segments"],
                         ms_median=med, ms_min=min(ms), ms_first=first, msps=frames / med / 1e3,
                         hbm_read_floor_ms=floor_ms, ratio_to_hbm_read=med / floor_ms, reps=a.reps,
                         mean_power=float(s.sum() / max(info["segments"], 1))))
        print(json.dumps(rows[-1]), flush=True)
        acc.close()
    check(lib.iqgpu_event_destroy(e0))
    check(lib.iqgpu_event_destroy(e1))
    check(lib.iqgpu_stream_destroy(stream))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")


if __name__ == "__main__":
    main()
