"""The numpy / scipy reference of maria_amd.flagging: plain, slow, and written from the definitions."""

import numpy as np
import scipy.ndimage


def median_residual(x, h):
    """(r, med): med the running median of 2 h + 1 samples with the end sample repeated, r = x - med in float32."""
    x = np.asarray(x, np.float32)
    med = scipy.ndimage.median_filter(x, size=(1, 2 * h + 1), mode="nearest")
    return x - med, med


def median_by_sorting(x, h):
    """The same median rebuilt as clamp, gather and sort."""
    x = np.asarray(x, np.float32)
    T = x.shape[1]
    idx = np.clip(np.arange(T)[:, None] + np.arange(-h, h + 1)[None, :], 0, T - 1)
    return np.sort(x[:, idx], axis=2)[:, :, h]


def robust_sigma(x, h):
    """[D] float64: 1.4826 times the lower median (element (T - 1) // 2 of the sorted row) of |r|."""
    r, _ = median_residual(x, h)
    a = np.sort(np.abs(r), axis=1)[:, (r.shape[1] - 1) // 2]
    return 1.4826 * a.astype(np.float64)


def flags(x, h, thresh, grow_before, grow_after):
    """(flags uint8 [D, T], count [D]): 1 a detection |r| > thresh[d], 2 grown, 0 neither; by loops."""
    r, _ = median_residual(x, h)
    D, T = r.shape
    thresh = np.asarray(thresh, np.float32)
    det = np.abs(r) > thresh[:, None]
    out = np.zeros((D, T), np.uint8)
    for d in range(D):
        for s in np.flatnonzero(det[d]):
            lo, hi = max(0, s - grow_before), min(T, s + grow_after + 1)
            out[d, lo:hi] = np.maximum(out[d, lo:hi], 2)
        out[d, det[d]] = 1
    return out, (out != 0).sum(axis=1)


def runs(f):
    """The maximal runs [a, b) of nonzero entries of a 1-D array."""
    nz = np.concatenate([[0], (np.asarray(f) != 0).astype(np.int8), [0]])
    edge = np.diff(nz)
    return list(zip(np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)))


def gap_fill(x, f, n_fit):
    """(filled x as float32, filled count [D], anchor scale [D, T] = max(|yL|, |yR|) at the flagged samples): float64
    loops, one rounding."""
    x = np.asarray(x, np.float32)
    D, T = x.shape
    out, scale, count = x.copy(), np.zeros((D, T)), np.zeros(D, np.int64)
    for d in range(D):
        for a, b in runs(f[d]):
            if a == 0 and b == T:
                continue
            L = [k for k in range(max(0, a - n_fit), a) if not f[d, k]]
            R = [k for k in range(b, min(T, b + n_fit)) if not f[d, k]]
            yL = np.mean(x[d, L].astype(np.float64)) if L else None
            yR = np.mean(x[d, R].astype(np.float64)) if R else None
            t = np.arange(a, b, dtype=np.float64)
            if a == 0:
                y = np.full(b - a, yR)
            elif b == T:
                y = np.full(b - a, yL)
            else:
                tL, tR = np.mean(np.asarray(L, np.float64)), np.mean(np.asarray(R, np.float64))
                y = yL + (yR - yL) * (t - tL) / (tR - tL)
            out[d, a:b] = y.astype(np.float32)
            scale[d, a:b] = max(abs(v) for v in (yL, yR) if v is not None)
            count[d] += b - a
    return out, count, scale


def downsample_flags(f, q):
    """[D, ceil(T / q)] uint8: output j is 1 if any flag of [j q - q, j q + q] within [0, T) is nonzero; by a loop."""
    f = np.asarray(f)
    D, T = f.shape
    T_out = (T + q - 1) // q
    out = np.zeros((D, T_out), np.uint8)
    for j in range(T_out):
        out[:, j] = (f[:, max(0, j * q - q):min(T, j * q + q + 1)] != 0).any(axis=1)
    return out
