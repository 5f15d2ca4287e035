"""Cost of the measure pass of seamless AGC sharding (iqgpu_chain_measure_device) against an ordinary pass
(iqgpu_chain_process_device) on the same chain, device-resident, past the lock, and of both routes of the measure pass where a
chain has both: the unfused route (the chain's fastest kernels with cf32 out + k_agc_measure) and k_front_s1<.., AGC> with its
packed output into a sink (iqgpu_debug_set("measure_route", "s1")).

    python tools/bench_measure.py [--log2 28] [--pairs 5] [--out FILE.json]
    python tools/bench_measure.py --host-fed [--log2 28] [--batches 16,64] [--pairs 5] [--legs a,b,c] [--out FILE.json]

Per shape: two warm ordinary calls (the first holds the lock), then `pairs` interleaved rounds of one call of each kind, host wall
clock around call + synchronise (ms), and the library's per-kernel event times of one more call of each kind.  The rows of both
routes are compared bit for bit.

--host-fed: the job as a host sees it.  One range of NRSC-5 cs16 + digital AGC in pinned memory, cut into N batches, run three
ways, interleaved, `pairs` rounds (at least five), medians: (a) the loop of iqgpu_chain_measure calls, (b) iqgpu_chain_measure_submit /
_collect, (c) iqgpu_chain_submit / _collect of the ordinary pass, the yardstick -- it runs at the copy engine's rate.  Host wall clock
around the whole range (ms, and GS/s of input), then the library's per-kernel event times of one more pass of (b) and (c)."""
import argparse
import ctypes as C
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


def host_fed(args):
    kw = dict(SHAPES["nrsc5-cs16+agc"])
    n, chunk = 1 << args.log2, 16384
    legs = args.legs.split(",")
    seg = synth.raw_stream(min(n, 1 << 22), 2.4e6, 7, "cs16").view(np.uint8)
    src = gpu.chain.PinnedBuffer(n * 4)
    for at in range(0, src.nbytes, seg.nbytes):
        src.array[at:at + seg.nbytes] = seg[:src.nbytes - at]
    chains = {leg: gpu.Chain(**kw) for leg in legs}
    depth = _lib.load().iqgpu_chain_pipeline_depth()
    res = {}
    for nb in [int(v) for v in args.batches.split(",")]:
        per = n // nb
        assert per * nb == n and per % chunk == 0, "batches must cut the range on the AGC chunk grid"
        rows = gpu.chain.PinnedBuffer((n // chunk) * 16)
        out_cap = chains[legs[0]].max_out_frames(per) * 4
        out = gpu.chain.PinnedBuffer(out_cap * nb) if "c" in legs else None
        rpb = per // chunk                                        # rows per batch

        def leg_a(ch):
            got = 0
            for i in range(nb):
                k = C.c_size_t(0)
                _lib.check(ch._lib.iqgpu_chain_measure(ch._h, C.c_void_p(src.ptr + i * per * 4), per, C.c_void_p(rows.ptr + i * rpb * 16), rpb, C.byref(k)))
                got += k.value
            return got

        def piped(ch, submit):
            flight, got = [], 0
            for i in range(nb):
                if len(flight) == depth:
                    ch.collect(flight.pop(0))
                k, t = submit(ch, i)
                got += k
                flight.append(t)
            for t in flight:
                ch.collect(t)
            return got

        run = {"a": leg_a,
               "b": lambda ch: piped(ch, lambda c, i: c.measure_submit(src.ptr + i * per * 4, per, rows.ptr + i * rpb * 16, rpb)),
               "c": lambda ch: piped(ch, lambda c, i: c.submit(src.ptr + i * per * 4, per, out.ptr + i * out_cap, out_cap))}
        t = {leg: [] for leg in legs}
        for leg in legs:
            run[leg](chains[leg])                                 # (buffers sized, the ordinary chain past its lock)
        for _ in range(max(5, args.pairs)):
            for leg in legs:
                t0 = time.perf_counter(); run[leg](chains[leg])
                t[leg].append((time.perf_counter() - t0) * 1e3)
        o = {"frames": n, "batches": nb, "ms": {leg: [round(v, 3) for v in t[leg]] for leg in legs},
             "median_ms": {leg: round(float(np.median(t[leg])), 3) for leg in legs},
             "spread_ms": {leg: round(float(max(t[leg]) - min(t[leg])), 3) for leg in legs},
             "median_gsps": {leg: round(n / float(np.median(t[leg])) / 1e6, 3) for leg in legs}}
        for leg in legs:
            if leg != "a":
                chains[leg].set_profiling(True)
                run[leg](chains[leg])
                o["kernels_ms_" + leg] = {k: round(v["ms"], 4) for k, v in chains[leg].profile().items() if v["launches"]}
                chains[leg].set_profiling(False)
        res["host-fed-%d" % nb] = o
        print("host-fed", json.dumps(o), flush=True)
        rows.free()
        if out is not None:
            out.free()
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=28)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--host-fed", action="store_true", help="the host-fed leg: measure loop / measure_submit / submit from pinned memory")
    ap.add_argument("--batches", default="16,64", help="--host-fed: batches per range, comma-separated")
    ap.add_argument("--legs", default="a,b,c", help="--host-fed: which of the three legs run")
    args = ap.parse_args()
    if args.host_fed:
        return host_fed(args)
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
