"""A numpy float64 model of the envelope accumulator's contract (include/iqgpu.h "envelope"): columns, tree, cells, one rounding, the
rails per format from the integer codes; x comes from the oracle's unpack at gain 1.  Every term is exact in double and the order is
fixed, so whatever is compared with this model is compared for EQUALITY.  Also the Python restatement of the burst finder and of the
floor, and the streams the tests share."""
import numpy as np

COLUMNS, CELL = 1024, 65536
FORMATS = ("cu8", "cs8", "cu16", "cs16", "sc16q11", "cs24", "cu32", "cs32", "cf32")
BPF = dict(cu8=2, cs8=2, cu16=4, cs16=4, sc16q11=4, cs24=6, cu32=8, cs32=8, cf32=8)
CODE = dict(cu8=np.uint8, cs8=np.int8, cu16=np.uint16, cs16=np.int16, sc16q11=np.int16, cu32=np.uint32, cs32=np.int32)
# lowest / highest code
RAILS = dict(cu8=(0, 255), cs8=(-128, 127), cu16=(0, 65535), cs16=(-32768, 32767), sc16q11=(-2048, 2047),
             cs24=(-(1 << 23), (1 << 23) - 1), cu32=(0, (1 << 32) - 1), cs32=(-(1 << 31), (1 << 31) - 1))


def codes_of(raw, fmt):
    """[n][2] int64 codes of the raw bytes of an integer format"""
    raw = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
    if fmt == "cs24":
        b = raw.reshape(-1, 3).astype(np.int64)
        c = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        return np.where(c >= 1 << 23, c - (1 << 24), c).reshape(-1, 2)
    return raw.view(CODE[fmt]).astype(np.int64).reshape(-1, 2)


def bytes_of(codes, fmt):
    if fmt == "cs24":
        c = (codes.reshape(-1) & 0xffffff).astype(np.int64)
        return np.stack([c & 0xff, (c >> 8) & 0xff, (c >> 16) & 0xff], axis=1).astype(np.uint8).reshape(-1)
    return codes.reshape(-1).astype(CODE[fmt]).view(np.uint8)


def stream(fmt, n, seed, rate=2.4e6):
    """n frames of the synthetic stream as bytes, rail codes (cf32: values at and beyond +-1.0) written in at known places"""
    from iq_tool_amd import synth
    raw = np.ascontiguousarray(synth.raw_stream(n, rate, seed, fmt)).view(np.uint8).reshape(-1).copy()
    places = sorted({0, n // 3, n // 2, n - 1})
    if fmt == "cf32":
        v = raw.view(np.float32).reshape(-1, 2)
        for k, i in enumerate(places):
            v[i] = [(-1.0, 1.0), (1.0, -1.5), (0.99999994, 1.25), (-1.0, -1.0)][k % 4]
        return raw
    lo, hi = RAILS[fmt]
    c = codes_of(raw, fmt)
    for k, i in enumerate(places):
        c[i] = [(lo, hi), (hi, hi), (lo, lo), (hi, lo)][k % 4]
    if fmt == "sc16q11" and n > 8:
        c[5], c[7] = (-32768, 32767), (-2049, 2048)           # beyond the Q11 rails: counted as on the rail
    return bytes_of(c, fmt)


def frame_terms(raw, fmt, oracle):
    """per frame: p (float64; +0.0 for a non-finite frame, which adds nothing to a sum that is never below +0.0), the components on
    a rail (0 .. 2) and whether the frame is finite"""
    raw = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
    x = oracle.to_cf32(raw, fmt, 1.0)
    re, im = x.real.astype(np.float32), x.imag.astype(np.float32)
    ok = np.isfinite(re) & np.isfinite(im)
    r64, i64 = np.where(ok, re, 0).astype(np.float64), np.where(ok, im, 0).astype(np.float64)
    p = r64 * r64 + i64 * i64                                  # two exact products, one rounded sum
    if fmt == "cf32":
        v = np.stack([re, im], axis=1)
        with np.errstate(invalid="ignore"):
            rail = ((v <= -1.0) | (v >= 1.0)).sum(axis=1) * ok
    else:
        c = codes_of(raw, fmt)
        lo, hi = RAILS[fmt]
        rail = ((c <= lo) | (c >= hi)).sum(axis=1) if fmt == "sc16q11" else ((c == lo) | (c == hi)).sum(axis=1)
    return p, rail.astype(np.int64), ok


def tree(v):
    """the fixed tree of adjacent pairs over a power-of-two number of doubles"""
    v = np.asarray(v, np.float64)
    while v.size > 1:
        v = v[0::2] + v[1::2]
    return float(v[0])


def cell_sum(p):
    """one cell of at most 65536 frames: column i mod 1024 summed in increasing i from 0.0, then the tree"""
    assert 0 < p.size <= CELL
    pad = np.zeros(-(-p.size // COLUMNS) * COLUMNS)
    pad[:p.size] = p
    cols = np.zeros(COLUMNS)
    for step in pad.reshape(-1, COLUMNS):
        cols = cols + step
    return tree(cols)


def row_sum(p):
    """the frames of one row, or of the open row: ((0.0 + cell 0) + cell 1) + ... in double, not rounded"""
    total = 0.0
    for at in range(0, p.size, CELL):
        total = total + cell_sum(p[at:at + CELL])
    return total


def model(raw, fmt, B, oracle):
    """(row_sum float32[rows], row_peak float32[rows], row_rail uint32[rows], open = (sum, peak, rail) in double / int, nonfinite)"""
    p, rail, ok = frame_terms(raw, fmt, oracle)
    rows = p.size // B
    s = np.array([row_sum(p[r * B:(r + 1) * B]) for r in range(rows)], np.float64).astype(np.float32)
    k = p[:rows * B].reshape(rows, B).max(axis=1).astype(np.float32) if rows else np.zeros(0, np.float32)
    n = rail[:rows * B].reshape(rows, B).sum(axis=1).astype(np.uint32) if rows else np.zeros(0, np.uint32)
    rest, rest_rail = p[rows * B:], rail[rows * B:]
    open_row = (row_sum(rest), float(rest.max()), int(rest_rail.sum())) if rest.size else (0.0, 0.0, 0)
    return s, k, n, open_row, int(p.size - ok.sum())


# ---- the burst finder and the floor, restated ----
def bursts(row_sum_f32, B, on, off, min_rows, hang_rows, pad_rows):
    mean = np.asarray(row_sum_f32, np.float32).astype(np.float64) / B
    rows, found, i = mean.size, [], 0
    while i < rows:
        if not mean[i] >= on:
            i += 1
            continue
        e, run = rows, 0
        for j in range(i + 1, rows):
            if mean[j] >= off:
                run = 0
            else:
                run += 1
                if run > hang_rows:
                    e = j + 1 - run
                    break
        if e - i >= min_rows:
            found.append([max(0, i - pad_rows), min(rows, e + pad_rows)])
        i = e
    joined = []
    for a, b in found:
        if joined and a <= joined[-1][1]:
            joined[-1][1] = b
        else:
            joined.append([a, b])
    out = []
    for a, b in joined:
        m = mean[a:b]
        peak = a + int(np.nanargmax(m)) if not np.isnan(m).all() else a
        out.append(dict(first_frame=a * B, frames=(b - a) * B, peak_row=peak, peak_mean=float(mean[peak])))
    return out


def floor(row_sum_f32, B, fraction):
    v = np.sort(np.asarray(row_sum_f32, np.float32))           # (numpy sorts NaN last)
    return float(np.float64(v[int(np.floor(fraction * (v.size - 1)))]) / B)
