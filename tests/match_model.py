"""A numpy float64 model of the template-correlation accumulator's contract (include/iqgpu.h "template correlation"): x from the
oracle's unpack at gain 1, c_t[n] = sum x[n + k] conj(h_t[k]) in float64, p = |c|^2, the segment count of the power spectrum's grid at
hop = nfft / 2, rows of B start positions with the largest p, the lowest n that attains it and the sum.  Also the streams with planted
copies that the tests share, and the float32 overlap-save whose error sets the bars of tests/test_gpu_match.py."""
import numpy as np

from env_model import BPF


def nfft_of(nfft, L):
    return nfft or next(n for n in (1024, 2048, 4096) if n // 2 + 1 >= L)


def segments_of(frames, nfft):
    return 0 if frames < nfft else (frames - nfft) // (nfft // 2) + 1


def rows_of(frames, nfft, B):
    return segments_of(frames, nfft) // (B // (nfft // 2))


def templates(nt, L, seed):
    """nt seeded templates of L frames: unit-modulus chips, a waveform with a sharp correlation peak"""
    rng = np.random.default_rng([int(seed), nt, L])
    return np.exp(2j * np.pi * rng.random((nt, L))).astype(np.complex64)


def planted(n, fmt, tmpl, places, seed, noise=0.02, amp=0.25):
    """n frames of complex noise with amp * template t added at frame `at` for every (at, t) or (at, t, amp) of places (cut at the
    stream's end), in the raw format, as bytes"""
    from iq_tool_amd import synth
    rng = np.random.default_rng([int(seed), n])
    z = noise * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for at, t, *a in places:
        h = tmpl[t][:max(0, n - at)]
        z[at:at + h.size] += (a[0] if a else amp) * h
    return np.ascontiguousarray(synth.quantise(z.astype(np.complex64), fmt)).view(np.uint8).reshape(-1)


def powers(x, tmpl):
    """p[t][n] in float64 for every start position n with n + L <= len(x)"""
    x = np.asarray(x, np.complex128)
    L = tmpl.shape[1]
    if x.size < L:
        return np.zeros((tmpl.shape[0], 0))
    m = 1 << int(np.ceil(np.log2(x.size + L)))
    X = np.fft.fft(x, m)
    out = []
    for h in np.asarray(tmpl, np.complex128):
        c = np.fft.ifft(X * np.conj(np.fft.fft(h, m)))[:x.size - L + 1]
        out.append(c.real ** 2 + c.imag ** 2)
    return np.array(out)


def reduce_rows(p, segs, V, B):
    """(peak, at, sum, margin)[rows, nt] and the open row (sum, peak, at)[nt] of p[t][0 .. segs V); margin = (best - runner-up) / best of
    a row, 0 for a row without power"""
    nt, R = p.shape[0], B // V
    rows = segs // R
    q = p[:, :rows * B].reshape(nt, rows, B)
    peak, at, total = q.max(axis=2).T, q.argmax(axis=2).T, q.sum(axis=2).T
    if rows:
        two = np.partition(q, B - 2, axis=2)[:, :, B - 2:]
        with np.errstate(invalid="ignore", divide="ignore"):
            margin = np.where(two[:, :, 1] > 0, (two[:, :, 1] - two[:, :, 0]) / two[:, :, 1], 0.0).T
    else:
        margin = np.zeros((0, nt))
    rest = p[:, rows * B:segs * V]
    if rest.shape[1]:
        open_row = (rest.sum(axis=1), rest.max(axis=1), rest.argmax(axis=1))
    else:
        open_row = (np.zeros(nt), np.zeros(nt), np.zeros(nt, np.int64))
    return (peak, at, total, margin), open_row


def model(raw, fmt, tmpl, B, oracle, nfft=0):
    """((peak, at, sum, margin)[rows, nt] in float64 / int, open row (sum, peak, at), info dict)"""
    raw = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
    tmpl = np.asarray(tmpl, np.complex64).reshape(-1, np.asarray(tmpl).shape[-1])
    x = oracle.to_cf32(raw, fmt, 1.0)
    N = nfft_of(nfft, tmpl.shape[1])
    segs, V = segments_of(x.size, N), N // 2
    rows, open_row = reduce_rows(powers(x, tmpl)[:, :segs * V], segs, V, B)
    info = dict(frames=raw.size // BPF[fmt], segments=segs, rows=segs // (B // V), open_segments=segs % (B // V), nfft=N, block_frames=B,
                n_templates=tmpl.shape[0], template_frames=tmpl.shape[1],
                template_energy=[float((np.abs(h.astype(np.complex128)) ** 2).sum()) for h in tmpl])
    return rows, open_row, info


def f32_overlap_save(raw, fmt, tmpl, B, oracle, nfft=0):
    """the rows of the same overlap-save in float32 on the CPU: scipy.fft on complex64, G rounded to float32, powers re^2 + im^2 in
    float32, sums in double -- (peak, at, sum)[rows, nt]"""
    import scipy.fft
    raw = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
    tmpl = np.asarray(tmpl, np.complex64).reshape(-1, np.asarray(tmpl).shape[-1])
    x = oracle.to_cf32(raw, fmt, 1.0).astype(np.complex64)
    N = nfft_of(nfft, tmpl.shape[1])
    segs, V = segments_of(x.size, N), N // 2
    G = (np.conj(np.fft.fft(tmpl.astype(np.complex128), N, axis=1)) / N).astype(np.complex64)
    seg = x[np.arange(segs)[:, None] * V + np.arange(N)[None, :]] if segs else np.zeros((0, N), np.complex64)
    X = scipy.fft.fft(seg, axis=1)
    assert X.dtype == np.complex64
    p = []
    for g in G:
        c = scipy.fft.ifft(X * g[None, :], axis=1)[:, :V] * np.float32(N)        # (G holds the 1 / N that scipy applies too: exact)
        assert c.dtype == np.complex64
        q = c.real * c.real + c.imag * c.imag
        assert q.dtype == np.float32
        p.append(q.reshape(-1))
    rows, _ = reduce_rows(np.array(p, np.float32).astype(np.float64).reshape(len(G), -1), segs, V, B)
    return rows[:3]
