#!/usr/bin/env python3
"""Time of the lag-product accumulator (Lag.push_device: k_lag_rows) on a resident buffer, B = 4096, for the lag sets (1,), (1, 2, 3, 4),
(2048,) and (1, 2048, 40000, 65536) on cs16, and for (1,) and (2048,) on cu8 and cf32, beside the envelope accumulator (Env.push_device:
k_env_rows, the same skeleton without partners, as tools/bench_env.py times it) on the same bytes in the same process.  A recorded
measurement, not a bar:

    timeout -k 10 600 python tools/bench_lag.py [--log2-frames 28] [--reps 5] [--out profiles/lag.json]

The buffer is 2^28 frames of the synthetic counter-hash stream, filled once per format; every repetition pushes the whole buffer in
one call into a reset accumulator, with the row planes in device memory, timed with events on a stream of its own (the first push is
reported apart and not in the median).  Per line: ms (median, min, max), GB/s of input bytes, the ratio to the envelope's median on the
same bytes.  The envelope is timed in front of and behind the lag sets of its format: the session's own drift."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B = 4096
SETS = {"cs16": ((1,), (1, 2, 3, 4), (2048,), (1, 2048, 40000, 65536)), "cu8": ((1,), (2048,)), "cf32": ((1,), (2048,))}
BPF = dict(cs16=4, cu8=2, cf32=8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-frames", type=int, default=28)
    ap.add_argument("--reps", type=int, default=5)
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

    def elapsed(work):
        check(lib.iqgpu_event_record(e0, stream))
        work()
        check(lib.iqgpu_event_record(e1, stream))
        check(lib.iqgpu_stream_synchronize(stream))
        ms = C.c_float(0)
        check(lib.iqgpu_event_elapsed_ms(e0, e1, C.byref(ms)))
        return float(ms.value)

    rows = []
    cap = frames // B
    planes = iq_tool_amd.DeviceBuffer(36 * cap)
    for fmt, sets in SETS.items():
        bpf = BPF[fmt]
        d = iq_tool_amd.DeviceBuffer(frames * bpf)
        piece = 1 << 24                                    # generated and uploaded in pieces
        for at in range(0, frames, piece):
            n = min(piece, frames - at)
            raw = np.ascontiguousarray(synth.hash_stream(n, 1, "cs16" if fmt == "cf32" else fmt, first=at))
            if fmt == "cf32":                              # the same codes as finite floats
                raw = (raw.astype(np.float32) / np.float32(32768.0))
            check(lib.iqgpu_memcpy_h2d(0, C.c_void_p(d.ptr + at * bpf), raw.ctypes.data_as(C.c_void_p), raw.nbytes))

        def record(name, acc, push):
            def once():
                acc.reset()
                return elapsed(push)
            first = once()
            ms = [once() for _ in range(a.reps)]
            med = statistics.median(ms)
            return dict(what=name, format=fmt, frames=frames, block_frames=B, ms_median=med, ms_min=min(ms), ms_max=max(ms), ms_first=first,
                        gb_per_s=frames * bpf / med / 1e6, reps=a.reps)

        def env_line(name):
            acc = iq_tool_amd.Env(fmt, B)
            r = record(name, acc, lambda: acc.push_device(d.ptr, frames, planes.ptr, planes.ptr + 4 * cap, planes.ptr + 8 * cap, cap, stream.value))
            acc.close()
            rows.append(r)
            print(json.dumps(r), flush=True)
            return r

        env = env_line("env")
        for lags in sets:
            acc = iq_tool_amd.Lag(fmt, B, lags)
            r = record("lag %s" % (lags,), acc, lambda: acc.push_device(d.ptr, frames, planes.ptr, planes.ptr + 32 * cap, cap, stream.value))
            r["lags"], r["ratio_to_env"] = list(lags), r["ms_median"] / env["ms_median"]
            acc.close()
            rows.append(r)
            print(json.dumps(r), flush=True)
        env_line("env (again)")
        d.free()
    planes.free()
    check(lib.iqgpu_event_destroy(e0))
    check(lib.iqgpu_event_destroy(e1))
    check(lib.iqgpu_stream_destroy(stream))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")


if __name__ == "__main__":
    main()
