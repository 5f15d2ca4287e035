#!/usr/bin/env python3
"""Time of the I/Q calibration at its defaults -- 64 blocks, a 9 x 9 grid, 5 levels -- on the device (Chain.calibrate_iq_device: the
block gather and five launches of k_iq_metric) against the same search with the host metric (IqOptimizer.calibrate) on the same
blocks.  A recorded measurement, not a bar:

    python tools/bench_iq_calib.py [--reps 20] [--out profiles/iq_calib.json]

The input is 2^20 cs16 frames of three tones with a 4 % / 0.03 rad imbalance and noise; both sides see the 64 blocks the chain picks.
Wall-clock per call, host timer around the synchronous entry points (each returns with its work done); the first call of each
side (allocations, table upload) is reported apart and not in the median."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import iq_tool_amd
    from iq_tool_amd import synth
    frames = 1 << 20
    n = np.arange(frames)
    rng = np.random.default_rng(3)
    x = sum(amp * np.exp(2j * np.pi * f * n) for f, amp in ((0.11, 0.5), (-0.23, 0.2), (0.31, 0.1)))
    x = x + 1e-3 * (rng.standard_normal(frames) + 1j * rng.standard_normal(frames))
    y = (x.real + 1j * (1.04 * (x.imag * np.cos(0.03) + x.real * np.sin(0.03)))).astype(np.complex64)
    raw = np.ascontiguousarray(synth.quantise(y, "cs16")).view(np.uint8).reshape(-1)
    ch = iq_tool_amd.Chain(in_format="cs16", out_format="cs16", input_rate_hz=2.4e6, target_rate_hz=744187.5)
    d = iq_tool_amd.DeviceBuffer(raw.nbytes)
    d.upload(raw)

    def timed(fn):
        t = time.perf_counter()
        r = fn()
        return (time.perf_counter() - t) * 1e3, r

    first_dev, got = timed(lambda: ch.calibrate_iq_device(d.ptr, frames))
    dev = [timed(lambda: ch.calibrate_iq_device(d.ptr, frames))[0] for _ in range(a.reps)]
    first_stage, _ = timed(lambda: ch.calibrate_iq(raw))
    stage = [timed(lambda: ch.calibrate_iq(raw))[0] for _ in range(a.reps)]
    blocks = ch.calibrate_iq_blocks_device(d.ptr, frames)
    o = iq_tool_amd.IqOptimizer(seed=1)
    first_host, ref = timed(lambda: o.calibrate(blocks))
    host = [timed(lambda: o.calibrate(blocks))[0] for _ in range(max(2, a.reps // 5))]
    res = dict(what="iq calibration at the defaults", blocks=got.blocks_taken, grid=got.grid, levels=len(got.levels), evaluations=got.evaluations,
               device_ms_median=statistics.median(dev), device_ms_min=min(dev), device_ms_first=first_dev,
               device_from_host_input_ms_median=statistics.median(stage), device_from_host_input_ms_first=first_stage,
               host_ms_median=statistics.median(host), host_ms_first=first_host,
               speedup=statistics.median(host) / statistics.median(dev),
               device_factors=got.factors, host_factors=ref.factors, reps=a.reps)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
