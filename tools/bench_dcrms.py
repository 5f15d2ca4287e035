"""Cost of the exact recipe for chains with the DC blocker and the dx / local AGC (iqgpu_chain_dcrms_*, include/iqgpu.h) beside the
ordinary single-stream pass, on NRSC-5 cs16 + dc_block + AGC local (or dx), device-resident:

    pass 1  iqgpu_chain_dcrms_dc_measure_device   (k_dc_prefix + the scan's map, one row copy per call)
    pass 1  iqgpu_chain_dcrms_dc_measure_range_device   (the same rows, every call of the range in ONE submission) -- beside the loop
    pass 2  iqgpu_chain_dcrms_dc_advance          (one walk over all rows)
    pass 3  iqgpu_chain_dcrms_seek_device         (the preroll in grid calls with the AGC out of the way, then k_agc_rms_seek) ...
            ... + iqgpu_chain_process_device      (the ordinary pass over the range: what a shard runs behind its seek -- and the
                                                   single-stream yardstick the three passes are compared with)

    python tools/bench_dcrms.py [--profile local|dx] [--log2 28] [--call-log2 22] [--rounds 7] [--out FILE.json]

One range of 2^log2 frames in device memory, walked in calls of 2^call-log2 frames.  Two warm ordinary passes, then `rounds`
interleaved rounds of one pass of each kind, host wall clock around the pass + synchronise (ms); median, minimum and maximum per
kind.  Nothing is asserted on the figures."""
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
    ap.add_argument("--profile", default="local", choices=("local", "dx"))
    ap.add_argument("--log2", type=int, default=28)
    ap.add_argument("--call-log2", type=int, default=22)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out")
    args = ap.parse_args()
    n, call = 1 << args.log2, 1 << args.call_log2
    assert n % call == 0 and call % 4096 == 0
    kw = dict(KW, agc_profile=args.profile)
    seg = synth.raw_stream(min(n, 1 << 22), 2.4e6, 7, "cs16").astype(np.int32).reshape(-1, 2)
    seg = np.clip(seg // 2 + np.array([983, -655]), -32768, 32767).astype(np.int16).reshape(-1).view(np.uint8)     # half scale + a DC offset
    buf = gpu.DeviceBuffer(n * 4)
    for at in range(0, n * 4, seg.nbytes):
        check(gpu.load().iqgpu_memcpy_h2d(0, buf.ptr + at, seg.ctypes.data, min(seg.nbytes, n * 4 - at)))
    ch = gpu.Chain(**kw)
    cap = ch.max_out_frames(call) * 4
    out = gpu.DeviceBuffer(cap)
    pre = min(n, -(-gpu.design_preroll_frames_dcrms(**kw) // call) * call)       # the preroll of a cut, in whole grid calls
    rows = []

    def ordinary():
        for a in range(0, n, call):
            ch.process_device(buf.ptr + a * 4, call, out.ptr, cap)
        ch.synchronize()

    def dc_measure():
        rows[:] = [ch.dcrms_dc_measure_device(a, buf.ptr + a * 4, call) for a in range(0, n, call)]

    def dc_measure_range():
        got, _ = ch.dcrms_dc_measure_range_device(0, buf.ptr, n, call)
        assert got.size == n // call

    def dc_walk():
        ch.dcrms_dc_advance(None, np.concatenate([r.reshape(1) for r in rows]))

    def seek():
        # (a cut at frame n of a stream that repeats the buffer: its preroll is the buffer's last grid calls)
        ch.dcrms_seek_device(n, buf.ptr + (n - pre) * 4, pre, call, None)

    kinds = {"pass1_dc_measure": dc_measure, "pass1_dc_measure_range": dc_measure_range, "pass2_dc_walk": dc_walk, "pass3_seek": seek, "pass3_process_single_stream": ordinary}
    ordinary()                                               # warm: allocations
    ordinary()
    ms = {k: [] for k in kinds}
    for _ in range(args.rounds):
        for k, fn in kinds.items():
            ch.synchronize()
            t0 = time.perf_counter()
            fn()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    res = dict(shape="nrsc5-cs16+dc_block+agc-" + args.profile, frames=n, call_frames=call, preroll_frames=pre, rounds=args.rounds,
               front_kernel=ch.front_kernel(), ms={k: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v))) for k, v in ms.items()})
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
