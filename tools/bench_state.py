"""Cost of a checkpoint (profiles/r11_state.md): the blob size of the shapes tests/test_gpu_state.py covers, and the wall time of one
iqgpu_chain_save_state and one iqgpu_chain_load_state beside one ordinary 2^28-frame call of the same chain (device-resident:
iqgpu_chain_process_device + synchronise, the path bench.py times).

    python tools/bench_state.py [--log2 28] [--rounds 9]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import iq_tool_amd  # noqa: E402

NRSC5 = dict(in_format="cs16", out_format="cs16", input_rate_hz=2.4e6, target_rate_hz=744187.5, shift_hz=200e3)
CU8_NRSC5 = dict(in_format="cu8", out_format="cu8", input_rate_hz=2.4e6, target_rate_hz=1488375.0)
CONFIG3 = dict(in_format="cs16", out_format="cs16", input_rate_hz=10e6, target_rate_hz=2.4e6, dc_block=True, iq_correct=True,
               iq_mag=0.013, iq_phase=-0.021, filters=(("passband", 158.5e3, 113e3),), filter_taps=1024)
CONFIG4 = dict(in_format="cu8", out_format="cu8", input_rate_hz=61.44e6, target_rate_hz=1488375.0,
               filters=(("lowpass", 300e3, 0.0),), filter_taps=4097, filter_impl="fir")
SIZES = {
    "nrsc5_cs16": NRSC5,
    "cu8_nrsc5": CU8_NRSC5,
    "usb + digital agc": dict(NRSC5, shift_hz=0.0, agc=True, filters=(("passband", 158.5e3, 113e3),)),
    "am (cascade) + digital agc": dict(NRSC5, shift_hz=0.0, target_rate_hz=46511.71875, agc=True),
    "r = 1.2 (k_interp)": dict(NRSC5, input_rate_hz=2.0e6, target_rate_hz=2.4e6, shift_hz=150e3),
    "configs[2]-like": CONFIG3,
    "configs[3]-like": CONFIG4,
    "no_resample + pre filter": dict(in_format="cs16", out_format="cf32", input_rate_hz=2.4e6, no_resample=True, shift_hz=-250e3,
                                     filters=(("passband", -300e3, 100e3),), transition_width_hz=20e3, attenuation_db=70.0,
                                     filter_impl="fft", fft_size=2048),
    "shift_after_resample, cf32": dict(NRSC5, shift_after_resample=True, out_format="cf32"),
    "dc blocker + digital agc": dict(NRSC5, agc=True, dc_block=True),
    "agc local": dict(NRSC5, agc=True, agc_profile="local"),
    "agc dx": dict(NRSC5, agc=True, agc_profile="dx"),
}
TIMED = {"nrsc5_cs16": NRSC5, "configs[2]-like": CONFIG3, "configs[3]-like": CONFIG4}


def median_us(fn, rounds):
    t = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(t)), float(min(t)), float(max(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=28)
    ap.add_argument("--rounds", type=int, default=9)
    a = ap.parse_args()
    out = dict(sizes={k: iq_tool_amd.design_state_size(**kw) for k, kw in SIZES.items()}, timed={})
    n = 1 << a.log2
    rng = np.random.default_rng(11)
    for name, kw in TIMED.items():
        ch = iq_tool_amd.Chain(**kw)
        bpf = ch.in_bytes
        piece = rng.integers(0, 256, min(n, 1 << 24) * bpf, dtype=np.uint8)
        d_in, d_out = iq_tool_amd.DeviceBuffer(n * bpf), iq_tool_amd.DeviceBuffer(ch.max_out_frames(n) * ch.out_bytes)
        lib = ch._lib
        import ctypes as C
        for at in range(0, n * bpf, piece.nbytes):
            iq_tool_amd._lib.check(lib.iqgpu_memcpy_h2d(0, C.c_void_p(d_in.ptr + at), piece.ctypes.data_as(C.c_void_p), min(piece.nbytes, n * bpf - at)))

        def step():
            ch.process_device(d_in.ptr, n, d_out.ptr, d_out.nbytes)
            ch.synchronize()

        step(), step()                                         # warm-up: buffers sized, clocks up
        blob = ch.save_state()
        row = dict(blob_bytes=len(blob), front_kernel=ch.front_kernel())
        # interleaved: call, save, load -- the load puts back the state the save took, so every round starts from the same one
        calls, saves, loads = [], [], []
        for _ in range(a.rounds):
            calls.append(median_us(step, 1)[0])
            saves.append(median_us(ch.save_state, 1)[0])
            b = ch.save_state()
            loads.append(median_us(lambda: ch.load_state(b), 1)[0])
        for what, t in (("call_us", calls), ("save_us", saves), ("load_us", loads)):
            row[what] = dict(median=float(np.median(t)), min=float(min(t)), max=float(max(t)))
        out["timed"][name] = row
        d_in.free(), d_out.free(), ch.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
