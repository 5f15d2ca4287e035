#!/usr/bin/env python3
"""Time of the template-correlation accumulator (Match.push_device: k_match_segs + k_match_fold + k_psd_carry) on a resident cs16
buffer, at nfft 1024 and 4096 with 1, 2 and 8 templates, against the power spectrum (Psd.push_device: k_psd_pages at hop = nfft / 2) on
the same bytes in the same process.  A recorded measurement, not a bar:

    timeout -k 10 600 python tools/bench_match.py [--log2-frames 28] [--reps 5] [--out profiles/match.json]

The buffer is 2^28 frames (1 GiB) of the counter-hash stream, uploaded once; every repetition pushes the whole buffer in one call into
a reset accumulator, timed with events on a stream of its own (the first push of each shape -- allocations -- is reported apart and
not in the median).  Per input frame the matcher transforms 2 (1 + n_templates) points where the power spectrum transforms 2: the
column `ratio_to_psd` is to be read against 1 + n_templates."""
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
    ap.add_argument("--block-frames", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import iq_tool_amd
    from iq_tool_amd import synth
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

    def timed(reset, push):
        reset()
        check(lib.iqgpu_event_record(e0, stream))
        push()
        check(lib.iqgpu_event_record(e1, stream))
        check(lib.iqgpu_stream_synchronize(stream))
        ms = C.c_float(0)
        check(lib.iqgpu_event_elapsed_ms(e0, e1, C.byref(ms)))
        return float(ms.value)

    rng = np.random.default_rng(1)
    rows = []
    for nfft in (1024, 4096):
        psd = iq_tool_amd.Psd("cs16", nfft=nfft, hop=nfft // 2, window="rect")
        first = timed(psd.reset, lambda: psd.push_device(d.ptr, frames, stream.value))
        psd_ms = statistics.median(timed(psd.reset, lambda: psd.push_device(d.ptr, frames, stream.value)) for _ in range(a.reps))
        psd.close()
        rows.append(dict(kernel="k_psd_pages", nfft=nfft, frames=frames, ms_median=psd_ms, ms_first=first, msps=frames / psd_ms / 1e3, reps=a.reps))
        print(json.dumps(rows[-1]), flush=True)
        B = max(a.block_frames, nfft // 2)
        for nt in (1, 2, 8):
            tmpl = np.exp(2j * np.pi * rng.random((nt, nfft // 2))).astype(np.complex64)
            acc = iq_tool_amd.Match("cs16", tmpl, B, nfft)
            cap = acc.max_rows(frames)
            out = iq_tool_amd.DeviceBuffer(3 * 4 * nt * cap)
            plane = 4 * nt * cap

            def push():
                assert acc.push_device(d.ptr, frames, out.ptr, out.ptr + plane, out.ptr + 2 * plane, cap, stream.value) == cap

            first = timed(acc.reset, push)
            ms = [timed(acc.reset, push) for _ in range(a.reps)]
            info = acc.read_open()[3]
            med = statistics.median(ms)
            rows.append(dict(kernel="k_match_segs", nfft=nfft, n_templates=nt, template_frames=nfft // 2, block_frames=B, frames=frames,
                             segments=info["segments"], rows=info["rows"], ms_median=med, ms_min=min(ms), ms_first=first, msps=frames / med / 1e3,
                             ratio_to_psd=med / psd_ms, transform_points_ratio=1 + nt, reps=a.reps))
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
