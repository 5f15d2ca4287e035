#!/usr/bin/env python3
"""Time of the envelope accumulator (Env.push_device: k_env_rows, and k_env_fold where B > 65536) on a resident cs16 buffer, at
B = 64, 4096 and 2^20, beside the capture-statistics accumulator (Stats.push_device, as tools/bench_stats.py times it) on the same
bytes in the same process.  A recorded measurement, not a bar:

    timeout -k 10 600 python tools/bench_env.py [--log2-frames 28] [--reps 5] [--out profiles/env.json]

The buffer is 2^28 frames of the synthetic counter-hash stream, filled once; every repetition pushes the whole buffer in one call into a
reset accumulator, with the three row planes in device memory, timed with events on a stream of its own (the first push is reported
apart and not in the median).  Per row: ms (median, min, max), TB/s of input, the ratio to the statistics accumulator's median and to
the bare read of the bytes at 8 TB/s."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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
    frames, bpf = 1 << a.log2_frames, 4
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

    d = iq_tool_amd.DeviceBuffer(frames * bpf)
    piece = 1 << 24                                        # generated and uploaded in pieces
    for at in range(0, frames, piece):
        n = min(piece, frames - at)
        raw = np.ascontiguousarray(synth.hash_stream(n, 1, "cs16", first=at))
        check(lib.iqgpu_memcpy_h2d(0, C.c_void_p(d.ptr + at * bpf), raw.ctypes.data_as(C.c_void_p), raw.nbytes))
    bare_ms = frames * bpf / 8e12 * 1e3

    def record(name, acc, push):
        def once():
            acc.reset()
            return elapsed(push)
        first = once()
        ms = [once() for _ in range(a.reps)]
        med = statistics.median(ms)
        return dict(what=name, frames=frames, ms_median=med, ms_min=min(ms), ms_max=max(ms), ms_first=first, tb_per_s=frames * bpf / med / 1e9,
                    ratio_to_bare_read=med / bare_ms, reps=a.reps)

    rows = []
    st = iq_tool_amd.Stats("cs16")
    rows.append(record("stats", st, lambda: st.push_device(d.ptr, frames, stream.value)))
    print(json.dumps(rows[-1]), flush=True)
    for lb in (6, 12, 20):
        b = 1 << lb
        cap = frames // b
        planes = iq_tool_amd.DeviceBuffer(12 * cap)
        acc = iq_tool_amd.Env("cs16", b)
        r = record("env B=2^%d" % lb, acc, lambda: acc.push_device(d.ptr, frames, planes.ptr, planes.ptr + 4 * cap, planes.ptr + 8 * cap, cap, stream.value))
        r["block_frames"], r["ratio_to_stats"] = b, r["ms_median"] / rows[0]["ms_median"]
        r["slower_than_stats_by_more_than_its_spread"] = r["ms_median"] > rows[0]["ms_median"] + (rows[0]["ms_max"] - rows[0]["ms_min"])
        rows.append(r)
        print(json.dumps(r), flush=True)
        acc.close()
        planes.free()
    # the statistics again behind the envelope runs: the session's own drift
    rows.append(record("stats (again)", st, lambda: st.push_device(d.ptr, frames, stream.value)))
    print(json.dumps(rows[-1]), flush=True)
    st.close()
    d.free()
    check(lib.iqgpu_event_destroy(e0))
    check(lib.iqgpu_event_destroy(e1))
    check(lib.iqgpu_stream_destroy(stream))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")


if __name__ == "__main__":
    main()
