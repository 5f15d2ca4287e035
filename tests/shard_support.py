"""What the seamless-sharding GPU tests (test_gpu_seek*.py, test_gpu_state.py, test_gpu_measure_pipe.py, test_gpu_shard_refusals.py)
share: the harness, the routing switches, frame slicing, byte equality, the refusal check and the dx / local input.  A plain module,
imported like np_design; anything that differs in substance between two files stays in those files."""
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "iq_tool_amd", "lib", "iqgpu_run")
OK, EINVAL, ECAPACITY, EHIP, EUNSUPPORTED = 0, -1, -8, -9, -10
LEVELS = (1.0, 0.2, 1.0, 4.0, 0.5)                            # steps of -14, +14, +12, -18 dB


def run(*args):
    """the harness: its report, the last line it prints"""
    r = subprocess.run([EXE, *args], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    return json.loads(r.stdout.strip().splitlines()[-1])


def set_switches(monkeypatch, names, sw):
    """the IQGPU_<NAME> routing switches of one case: every one of `names` cleared, then those of sw set"""
    for k in names:
        monkeypatch.delenv("IQGPU_" + k, raising=False)
    for k, v in sw.items():
        monkeypatch.setenv("IQGPU_" + k, v)


def bpf(kw):
    """bytes per input frame of a description"""
    return {"cu8": 2, "cs8": 2, "cf32": 8}.get(kw["in_format"], 4)


def frames(kw, raw, a, b):
    """frames [a, b) of a raw stream in the description's input format, as bytes"""
    return np.ascontiguousarray(raw).view(np.uint8)[a * bpf(kw):b * bpf(kw)]


def fr(x, a, b):
    """frames [a, b) of an interleaved stream with one element per component"""
    return x[2 * a:2 * b]


def same(a, b):
    """byte equality: the same size and the same bytes"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.nbytes == b.nbytes and a.tobytes() == b.tobytes()


def differing(a, b):
    return int((a.view(np.uint8) != b.view(np.uint8)).sum()) if a.nbytes == b.nbytes else -1


def expect(gpu, code, fn, *args, word=None):
    """fn(*args) is refused with `code`, and with `word` in the message"""
    with pytest.raises(gpu.IqgpuError) as e:
        fn(*args)
    print(e.value)
    assert e.value.code == code, str(e.value)
    if word:
        assert word in str(e.value)


def words(st):
    """the three words of the seam certificate, as bits"""
    return (np.float32(st.current_gain).view(np.uint32).item(), np.float32(st.peak_memory).view(np.uint32).item(), int(st.samples_seen))


def noise(n, fmt, seed, levels=LEVELS):
    """seeded Gaussian noise under level steps, never silent: the input of the dx / local tests"""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((n, 2))
    env = np.repeat(np.asarray(levels, np.float64), -(-n // len(levels)))[:n, None]
    if fmt == "cu8":
        return np.clip(np.rint(127.5 + 6.0 * env * z), 0, 255).astype(np.uint8).reshape(-1)
    return np.clip(np.rint(1500.0 * env * z), -32768, 32767).astype(np.int16).reshape(-1)


def grid(a, b, c):
    """the grid calls of [a, b): the last one of a stream may be shorter"""
    return [(p, min(p + c, b)) for p in range(a, b, c)]
