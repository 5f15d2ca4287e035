"""A numpy float64 model of the lag-product accumulator's contract (include/iqgpu.h "lag products"): the term of a frame and a lag, the
columns, the tree, the cells, one rounding, the history that is simply "the stream since the last reset"; x comes from the oracle's
unpack at gain 1.  Every product is exact in double and the order is fixed, so whatever is compared with this model is compared for
EQUALITY.  The tree, the power term and the streams are env_model's, imported, not restated.  Also the two host helpers, restated."""
import math

import numpy as np

import env_model
from env_model import CELL, COLUMNS, tree


def lag_terms(re, im, ok, d):
    """(re term, im term, present) per frame n of the stream for lag d: the term exists for n >= d when x[n] and x[n - d] are finite"""
    n = re.size
    tr, ti, present = np.zeros(n), np.zeros(n), np.zeros(n, bool)
    if n > d:
        a_re, a_im, b_re, b_im = re[d:], im[d:], re[:-d], im[:-d]
        present[d:] = ok[d:] & ok[:-d]
        tr[d:] = a_re * b_re + a_im * b_im                       # two exact products, one rounded sum
        ti[d:] = a_im * b_re - a_re * b_im                       # ... one rounded difference
    return tr, ti, present


def cell_sum(t, present):
    """one cell of at most 65536 frames: column i mod 1024 summed in increasing i from 0.0 -- an absent term is an absent addend --
    then the tree (a cell of fewer than 1024 frames: the tree over its columns, a power of two of them)"""
    assert 0 < t.size <= CELL
    width = COLUMNS if t.size >= COLUMNS else 1 << max(0, (t.size - 1).bit_length())
    size = -(-t.size // width) * width
    tt, pp = np.zeros(size), np.zeros(size, bool)
    tt[:t.size], pp[:t.size] = t, present
    cols = np.zeros(width)
    for step, has in zip(tt.reshape(-1, width), pp.reshape(-1, width)):
        cols = np.where(has, cols + step, cols)
    return tree(cols)


def row_value(t, present, B):
    """the frames of one row, or of the open row (fewer than B): ((0.0 + cell 0) + cell 1) + ... in double, not rounded.  The open
    row of a B < 1024 stands in a tree over B columns, the missing ones +0.0"""
    if t.size == 0:
        return 0.0
    if B < COLUMNS and t.size < B:
        t, present = np.concatenate([t, np.zeros(B - t.size)]), np.concatenate([present, np.zeros(B - present.size, bool)])
    total = 0.0
    for at in range(0, t.size, CELL):
        total = total + cell_sum(t[at:at + CELL], present[at:at + CELL])
    return total


def components(raw, fmt, lags, oracle):
    """per component (re, im of every lag, then the power): (term per frame, present per frame); and the finite mask"""
    raw = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
    x = oracle.to_cf32(raw, fmt, 1.0)
    re32, im32 = x.real.astype(np.float32), x.imag.astype(np.float32)
    ok = np.isfinite(re32) & np.isfinite(im32)
    re, im = np.where(ok, re32, 0).astype(np.float64), np.where(ok, im32, 0).astype(np.float64)
    comps = []
    for d in lags:
        tr, ti, present = lag_terms(re, im, ok, d)
        comps += [(tr, present), (ti, present)]
    comps.append((re * re + im * im, ok))
    return comps, ok


def model(raw, fmt, B, lags, oracle):
    """(row_lag complex64[rows, n_lags], row_sum float32[rows], open = (lag complex128[n_lags], sum float), nonfinite)"""
    comps, ok = components(raw, fmt, lags, oracle)
    n, rows = ok.size, ok.size // B
    vals = np.zeros((rows, len(comps)), np.float64)
    opened = np.zeros(len(comps), np.float64)
    for c, (t, present) in enumerate(comps):
        for r in range(rows):
            vals[r, c] = row_value(t[r * B:(r + 1) * B], present[r * B:(r + 1) * B], B)
        opened[c] = row_value(t[rows * B:], present[rows * B:], B)
    f = vals.astype(np.float32)                                  # the ONE rounding
    nl = len(lags)
    row_lag = (f[:, 0:2 * nl:2] + 1j * f[:, 1:2 * nl:2]).astype(np.complex64).reshape(rows, nl)
    open_lag = opened[0:2 * nl:2] + 1j * opened[1:2 * nl:2]
    return row_lag, f[:, 2 * nl].copy(), (open_lag.astype(np.complex128), float(opened[2 * nl])), int(n - ok.sum())


# ---- the host helpers, restated ----
def freq(re, im, lag, sample_rate):
    if re == 0.0 and im == 0.0:
        return 0.0
    return math.atan2(im, re) / (2.0 * math.pi * lag) * sample_rate


def estimate(row_lag, row_sum, lags, lag_index, first_row, n_rows, sample_rate):
    """row_lag: complex64 [rows, n_lags]; row_sum: float32 [rows] or None"""
    v = np.asarray(row_lag, np.complex64).reshape(-1, len(lags))
    re = im = power = 0.0
    for r in range(first_row, first_row + n_rows):
        a, b = float(v[r, lag_index].real), float(v[r, lag_index].imag)
        s = None if row_sum is None else float(np.float32(row_sum[r]))
        if a != a or b != b or (s is not None and s != s):
            continue
        re, im = re + a, im + b
        if s is not None:
            power += s
    return dict(re=re, im=im, power=power, hz=freq(re, im, lags[lag_index], sample_rate),
                coherence=math.hypot(re, im) / power if power > 0 else 0.0, span_hz=sample_rate / lags[lag_index])


stream = env_model.stream
