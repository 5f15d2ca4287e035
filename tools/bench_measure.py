"""Cost of the measure pass of seamless AGC sharding (iqgpu_chain_measure_device) against an ordinary pass
(iqgpu_chain_process_device) on the same chain, device-resident, past the lock, and of both routes of the measure pass where a
chain has both: the unfused route (the chain's fastest kernels with cf32 out + k_agc_measure) and k_front_s1<.., AGC> with its
packed output into a sink (iqgpu_debug_set("measure_route", "s1")).

    python tools/bench_measure.py [--log2 28] [--pairs 5] [--out FILE.json]

Per shape: two warm ordinary calls (the first holds the lock), then `pairs` interleaved rounds of one call of each kind, host wall
clock around call + synchronise (ms), and the library's per-kernel event times of one more call of each kind.  The rows of both
routes are compared bit for bit."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import iq_tool_amd as gpu                                   # noqa: E402
from iq_tool_amd import _lib, synth                          # noqa: E402

SHAPES = {
    "nrsc5-cs16+agc": dict(in_format="cs16", out_format="cs16", input_rate_hz=2.4e6, target_rate_hz=744187.5, shift_hz=200e3, agc=True),
    "cu8-nrsc5": dict(in_format="cu8", out_format="cu8", input_rate_hz=2.4e6, target_rate_hz=1488375.0, agc=True),
    "cs16-fm-nrsc5-usb": dict(in_format="cs16", out_format="cs16", input_rate_hz=2.4e6, target_rate_hz=744187.5, agc=True,
                              filters=(("passband", 158.5e3, 113e3),)),
}


def chain(kw, route):
    _lib.check(_lib.load().iqgpu_debug_set(b"measure_route", route.encode() if route else None))
    ch = gpu.Chain(**kw)
    _lib.check(_lib.load().iqgpu_debug_set(b"measure_route", None))
    return ch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=28)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    n = 1 << args.log2
    res = {}
    for name, kw in SHAPES.items():
        seg = synth.raw_stream(1 << 22, 2.4e6, 7, kw["in_format"])
        raw = np.tile(seg, max(1, n >> 22))
        routes = {"unfused": chain(kw, "unfused")}
        if "filters" not in kw:
            routes["s1"] = chain(kw, "s1")                   # (chains with a filter behind the resampler have no such kernel)
        ch = routes["unfused"]
        d_in = gpu.DeviceBuffer(raw.nbytes); d_in.upload(raw)
        d_out = gpu.DeviceBuffer(ch.max_out_frames(n) * ch.out_bytes)
        del raw
        for c in routes.values():
            for _ in range(2):
                c.process_device(d_in.ptr, n, d_out.ptr, d_out.nbytes); c.synchronize()
            c.measure_device(d_in.ptr, n)
        t = {"process": []}
        t.update({"measure_" + r: [] for r in routes})
        rows = {}
        for _ in range(args.pairs):
            t0 = time.perf_counter(); ch.process_device(d_in.ptr, n, d_out.ptr, d_out.nbytes); ch.synchronize()
            t["process"].append((time.perf_counter() - t0) * 1e3)
            for r, c in routes.items():
                t0 = time.perf_counter(); rows[r] = c.measure_device(d_in.ptr, n)
                t["measure_" + r].append((time.perf_counter() - t0) * 1e3)
        out = {k: [round(x, 4) for x in v] for k, v in t.items()}
        out["ratio_of_medians"] = {r: round(float(np.median(t["measure_" + r]) / np.median(t["process"])), 3) for r in routes}
        for r, c in routes.items():
            c.set_profiling(True)
            c.measure_device(d_in.ptr, n)
            out["kernels_ms_measure_" + r] = {k: round(v["ms"], 4) for k, v in c.profile().items() if v["launches"]}
            out["front_kernel_measure_" + r] = c.front_kernel()
        ch.process_device(d_in.ptr, n, d_out.ptr, d_out.nbytes)
        out["kernels_ms_process"] = {k: round(v["ms"], 4) for k, v in ch.profile().items() if v["launches"]}
        out["front_kernel_process"] = ch.front_kernel()
        if "s1" in routes:
            # (the timed chains stand at different stream positions by now: two fresh ones, one call each from frame 0)
            fresh = {r: chain(kw, r).measure_device(d_in.ptr, n) for r in routes}
            out["routes_agree_bit_for_bit"] = bool(np.array_equal(fresh["s1"].view(np.uint8), fresh["unfused"].view(np.uint8)))
        res[name] = out
        print(name, json.dumps(out), flush=True)
        d_in.free(); d_out.free()
        for c in routes.values():
            c.close()
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
