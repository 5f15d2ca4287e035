#!/usr/bin/env python3
"""Time of the capture-statistics accumulator (Stats.push_device: k_stats_pages + k_stats_fold) on a resident buffer, for cs16, cu8 and
cf32, on the synthetic counter-hash stream and on an all-zero stream (digital silence: every lane of every wave on one histogram bin).
A recorded measurement, not a bar:

    timeout -k 10 600 python tools/bench_stats.py [--log2-frames 28] [--reps 7] [--out profiles/stats.json]

Per format the buffer is 2^28 frames, filled once; every repetition pushes the whole buffer in one call into a reset accumulator, timed
with events on a stream of its own (the first push is reported apart and not in the median).  In the same job, for the same bytes, a
plain read pass by code that exists already: iqgpu_chain_dc_measure_device (k_dc_prefix) of a dc_block chain in the same input format,
timed with events on the chain's stream.  Per row: ms, MS/s, TB/s of input, the ratio to that read pass, and per format the
zero-stream / synthetic-stream ratio."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BPF = dict(cs16=4, cu8=2, cf32=8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-frames", type=int, default=28)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import iq_tool_amd
    from iq_tool_amd import synth
    from iq_tool_amd._lib import check
    lib = iq_tool_amd.load()
    frames = 1 << a.log2_frames
    stream, e0, e1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    check(lib.iqgpu_stream_create(0, C.byref(stream)))
    check(lib.iqgpu_event_create(C.byref(e0)))
    check(lib.iqgpu_event_create(C.byref(e1)))

    def elapsed(s, work):
        check(lib.iqgpu_event_record(e0, s))
        work()
        check(lib.iqgpu_event_record(e1, s))
        check(lib.iqgpu_stream_synchronize(s))
        ms = C.c_float(0)
        check(lib.iqgpu_event_elapsed_ms(e0, e1, C.byref(ms)))
        return float(ms.value)

    rows = []
    for fmt in ("cs16", "cu8", "cf32"):
        bpf = BPF[fmt]
        d = iq_tool_amd.DeviceBuffer(frames * bpf)
        acc = iq_tool_amd.Stats(fmt)
        ch = iq_tool_amd.Chain(in_format=fmt, out_format="cs16", input_rate_hz=2.4e6, target_rate_hz=744187.5, dc_block=True)
        per_fmt = {}
        for data in ("synthetic", "zeros"):
            piece = 1 << 24                                # generated and uploaded in pieces
            for at in range(0, frames, piece):
                n = min(piece, frames - at)
                if data == "zeros":
                    raw = np.zeros(n * bpf, np.uint8)
                elif fmt == "cf32":
                    raw = (synth.hash_stream(n, 1, "cs16", first=at).astype(np.float32) / np.float32(32768.0))
                else:
                    raw = synth.hash_stream(n, 1, fmt, first=at)
                raw = np.ascontiguousarray(raw)
                assert raw.nbytes == n * bpf
                check(lib.iqgpu_memcpy_h2d(0, C.c_void_p(d.ptr + at * bpf), raw.ctypes.data_as(C.c_void_p), raw.nbytes))

            def push():
                acc.reset()
                return elapsed(stream, lambda: acc.push_device(d.ptr, frames, stream.value))

            def read_pass():
                return elapsed(C.c_void_p(ch.get_stream()), lambda: ch.dc_measure_device(0, d.ptr, frames))

            first = push()
            ms = [push() for _ in range(a.reps)]
            r = acc.read()
            read_pass()
            rd = [read_pass() for _ in range(a.reps)]
            med, rmed = statistics.median(ms), statistics.median(rd)
            per_fmt[data] = med
            rows.append(dict(format=fmt, data=data, frames=frames, ms_median=med, ms_min=min(ms), ms_max=max(ms), ms_first=first,
                             msps=frames / med / 1e3, tb_per_s=frames * bpf / med / 1e9, read_pass_ms_median=rmed, read_pass_ms_min=min(rd),
                             read_pass_tb_per_s=frames * bpf / rmed / 1e9, ratio_to_read_pass=med / rmed, reps=a.reps,
                             frames_counted=int(r.frames), bins_used=[int(np.count_nonzero(np.ctypeslib.as_array(r.hist)[c])) for c in range(2)]))
            if data == "zeros":
                rows[-1]["zeros_over_synthetic"] = per_fmt["zeros"] / per_fmt["synthetic"]
            print(json.dumps(rows[-1]), flush=True)
        acc.close()
        del ch
        d.free()
    check(lib.iqgpu_event_destroy(e0))
    check(lib.iqgpu_event_destroy(e1))
    check(lib.iqgpu_stream_destroy(stream))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")


if __name__ == "__main__":
    main()
