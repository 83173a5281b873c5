"""A numpy restatement of the two spectrum augmentations (reference data/augmentations.py:12-39) on the plan's op table:
test infrastructure only, the yardstick the kernel is compared with on random rows.  Every step is the reference's fp64
operation in the reference's order (SciPy's correlate1d symmetric branch, np.interp), vectorised over the points."""
import numpy as np

COPY, GAUSS, HSHIFT = 0, 1, 2


def reflect(k, L):
    m = np.mod(k, 2 * L)
    return np.where(m < L, m, 2 * L - 1 - m)


def gauss(row, w):
    """gaussian_filter1d(row, sigma) given the half kernel w_0 .. w_R: x[i] w0, then + (x[i-q] + x[i+q]) w_q, q = R .. 1."""
    x = np.asarray(row, dtype=np.float64)
    L, R = x.size, w.size - 1
    i = np.arange(L)
    acc = x * w[0]
    for q in range(R, 0, -1):
        acc = acc + (x[reflect(i - q, L)] + x[reflect(i + q, L)]) * w[q]
    return acc


def hshift(row, n, i):
    """horizontal_shift_augment output i: row[i::n] (m = L // n points) on np.linspace(0, L, m), at 0..L-1 (np.interp)."""
    x = np.asarray(row, dtype=np.float64)
    L = x.size
    m = L // n
    knots = np.linspace(0, L, m)
    y = x[i::n][:m]
    pts = np.arange(L, dtype=np.float64)
    j = np.clip(np.searchsorted(knots, pts, side="right") - 1, 0, m - 2)
    slope = (y[j + 1] - y[j]) / (knots[j + 1] - knots[j])
    return np.where(knots[j] == pts, y[j], slope * (pts - knots[j]) + y[j])


def apply(table, src, op, op_table, weights):
    """Rows of afm_spectra_augment in fp64: row r = op_table[op[r]] on table[src[r]]."""
    out = np.empty((len(src), table.shape[1]), dtype=np.float64)
    for r, (s, o) in enumerate(zip(src, op)):
        kind, a, b = (int(v) for v in op_table[o])
        row = table[s].astype(np.float64)
        if kind == GAUSS:
            out[r] = gauss(row, weights[b:b + a + 1])
        elif kind == HSHIFT:
            out[r] = hshift(row, a, b)
        else:
            out[r] = row
    return out
