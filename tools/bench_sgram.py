#!/usr/bin/env python3
"""Time of the row accumulator (Sgram.push_device: k_sgram_cells + k_sgram_fold + k_psd_carry) on a resident cs16 buffer at nfft 1024,
hop 512, the Hann window, for R = 1, 32 and 1024 segments a row, both planes produced; beside it the power-spectrum accumulator
(Psd.push_device) on the same buffer, whose transform work is the same.  A recorded measurement, not a bar:

    timeout -k 10 600 python tools/bench_sgram.py [--log2-frames 26] [--reps 5] [--out profiles/sgram.json]

The buffer is 2^26 frames (256 MiB) of the counter-hash stream, uploaded once; every repetition pushes the whole buffer in one call into
a reset accumulator, timed with events on a stream of its own (the first push of each case -- allocations -- is reported apart and not
in the median).  Per case: ms, MS/s, the rows and the bytes they take (8 bytes a bin and row), and the bytes per second moved:
input read plus rows written, over the median."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-frames", type=int, default=26)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import iq_tool_amd
    from iq_tool_amd import synth
    from iq_tool_amd._lib import check
    lib = iq_tool_amd.load()
    frames, nfft, hop = 1 << a.log2_frames, 1024, 512
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

    def timed(reset, push):
        reset()
        check(lib.iqgpu_event_record(e0, stream))
        push()
        check(lib.iqgpu_event_record(e1, stream))
        check(lib.iqgpu_stream_synchronize(stream))
        ms = C.c_float(0)
        check(lib.iqgpu_event_elapsed_ms(e0, e1, C.byref(ms)))
        return float(ms.value)

    def record(what, reset, push, rows_out, **more):
        first = timed(reset, push)
        ms = [timed(reset, push) for _ in range(a.reps)]
        med = statistics.median(ms)
        row_bytes = rows_out * nfft * 8
        out.append(dict(what=what, nfft=nfft, hop=hop, window="hann", format="cs16", frames=frames, ms_median=med, ms_min=min(ms), ms_first=first,
                        msps=frames / med / 1e3, rows=rows_out, row_bytes=row_bytes, bytes_per_s=(frames * 4 + row_bytes) / (med * 1e-3), reps=a.reps, **more))
        print(json.dumps(out[-1]), flush=True)

    out = []
    ref = iq_tool_amd.Psd("cs16", nfft=nfft, hop=hop)
    record("psd", ref.reset, lambda: ref.push_device(d.ptr, frames, stream.value), 0)
    ref.close()
    for R in (1, 32, 1024):
        acc = iq_tool_amd.Sgram("cs16", nfft=nfft, hop=hop, row_segments=R)
        cap = acc.max_rows(frames)
        planes = [iq_tool_amd.DeviceBuffer(cap * nfft * 4) for _ in range(2)]
        record("sgram", acc.reset, lambda: acc.push_device(d.ptr, frames, planes[0].ptr, planes[1].ptr, cap, stream.value), cap, row_segments=R)
        info = acc.read_open()[2]
        assert info["rows"] == cap
        acc.close()
        for p in planes:
            p.free()
    check(lib.iqgpu_event_destroy(e0))
    check(lib.iqgpu_event_destroy(e1))
    check(lib.iqgpu_stream_destroy(stream))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("[\n" + ",\n".join(json.dumps(r) for r in out) + "\n]\n")


if __name__ == "__main__":
    main()
