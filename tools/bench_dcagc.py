"""Cost of the exact recipe for chains with the DC blocker and the digital AGC (iqgpu_chain_dcagc_*, include/iqgpu.h) beside the
ordinary pass, on NRSC-5 cs16 + dc_block + digital AGC, device-resident, behind the lock:

    pass 1  iqgpu_chain_dcagc_dc_measure_device   (k_dc_prefix + the scan's map, one row copy per call)
    pass 1  iqgpu_chain_dcagc_dc_measure_range_device   (the same rows, every call of the range in ONE submission: k_dc_prefix_batch +
            k_dc_scan_batch, one copy of all rows, one synchronisation) -- beside the per-call loop, interleaved with it
    pass 3  iqgpu_chain_dcagc_measure_device      (shadow calls: the ordinary kernels, no output kept, one row copy per call)
    pass 5  iqgpu_chain_process_device            (the ordinary pass: what a shard runs behind its seek -- and the yardstick)

    python tools/bench_dcagc.py [--log2 28] [--call-log2 22] [--rounds 7] [--ordinary-only] [--host-fed] [--out FILE.json]

One range of 2^log2 frames in device memory, walked in calls of 2^call-log2 frames.  One warm ordinary pass (it holds the lock), then
`rounds` interleaved rounds of one pass of each kind, host wall clock around the pass + synchronise (ms); median, minimum and maximum
per kind.  --ordinary-only times pass 5 alone (a library without the new entry points: the parent's figure on the same box).
--host-fed adds pass 1 through the range form's HOST variant from pinned memory (staging slices, copy and kernels overlapping)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import iq_tool_amd as gpu                                   # noqa: E402
from iq_tool_amd import synth                                # noqa: E402
from iq_tool_amd._lib import check                           # noqa: E402

KW = dict(in_format="cs16", out_format="cs16", input_rate_hz=2.4e6, target_rate_hz=744187.5, shift_hz=200e3, dc_block=True, agc=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=28)
    ap.add_argument("--call-log2", type=int, default=22)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--ordinary-only", action="store_true")
    ap.add_argument("--host-fed", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    n, call = 1 << args.log2, 1 << args.call_log2
    assert n % call == 0 and call % 16384 == 0
    seg = synth.raw_stream(min(n, 1 << 22), 2.4e6, 7, "cs16").astype(np.int32).reshape(-1, 2)
    seg = np.clip(seg // 2 + np.array([983, -655]), -32768, 32767).astype(np.int16).reshape(-1).view(np.uint8)     # half scale + a DC offset
    buf = gpu.DeviceBuffer(n * 4)
    for at in range(0, n * 4, seg.nbytes):
        check(gpu.load().iqgpu_memcpy_h2d(0, buf.ptr + at, seg.ctypes.data, min(seg.nbytes, n * 4 - at)))
    ch = gpu.Chain(**KW)
    cap = ch.max_out_frames(call) * 4
    out = gpu.DeviceBuffer(cap)

    def ordinary():
        for a in range(0, n, call):
            ch.process_device(buf.ptr + a * 4, call, out.ptr, cap)
        ch.synchronize()

    def dc_measure():
        first = ch.tell()[0]
        for a in range(0, n, call):
            ch.dcagc_dc_measure_device(first + a, buf.ptr + a * 4, call)

    def dc_measure_range():
        rows, _ = ch.dcagc_dc_measure_range_device(ch.tell()[0], buf.ptr, n, call)
        assert rows.size >= n // call

    pinned = None
    if args.host_fed:
        pinned = gpu.PinnedBuffer(n * 4)
        for at in range(0, n * 4, seg.nbytes):
            m = min(seg.nbytes, n * 4 - at)
            pinned.array[at:at + m] = seg[:m]

    def dc_measure_range_host():
        rows, _ = ch.dcagc_dc_measure_range(ch.tell()[0], pinned.array[:n * 4], call)
        assert rows.size >= n // call

    def shadow():
        for a in range(0, n, call):
            ch.dcagc_measure_device(buf.ptr + a * 4, call)

    kinds = {"pass5_process": ordinary}
    if not args.ordinary_only:
        kinds = {"pass1_dc_measure": dc_measure, "pass1_dc_measure_range": dc_measure_range, "pass3_shadow_measure": shadow,
                 "pass5_process": ordinary}
        if args.host_fed:
            kinds["pass1_dc_measure_range_host_pinned"] = dc_measure_range_host
    ordinary()                                               # warm: allocations, and the stream locks
    ordinary()
    assert ch.agc_state()["locked"]
    ms = {k: [] for k in kinds}
    for _ in range(args.rounds):
        for k, fn in kinds.items():
            ch.synchronize()
            t0 = time.perf_counter()
            fn()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    res = dict(shape="nrsc5-cs16+dc_block+agc", frames=n, call_frames=call, rounds=args.rounds, front_kernel=ch.front_kernel(),
               ms={k: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v))) for k, v in ms.items()})
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
