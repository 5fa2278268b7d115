"""The numpy float64 reference of maria_amd.jumps: plain, slow, and written from the definitions; and
``noisy_rows``, the data of the recovery tests."""

import numpy as np


def valid_mask(x, flags):
    x = np.asarray(x)
    return np.ones(x.shape, bool) if flags is None else np.asarray(flags) == 0


def means(x, flags, w, g):
    """(mean_L, mean_R, n_L, n_R), each [D, T]: the float64 means and counts of the valid samples of [t - g - w, t - g) and
    [t + g, t + g + w), from the cumulative sums of the row with its invalid samples zeroed (nan where a count is 0)."""
    x = np.asarray(x, np.float32)
    D, T = x.shape
    ok = valid_mask(x, flags)
    cs = np.concatenate([np.zeros((D, 1)), np.cumsum(np.where(ok, x.astype(np.float64), 0.0), axis=1)], axis=1)
    cn = np.concatenate([np.zeros((D, 1), np.int64), np.cumsum(ok, axis=1)], axis=1)
    t = np.arange(T)
    clip = lambda a: np.clip(a, 0, T)  # noqa: E731
    l0, l1, r0, r1 = clip(t - g - w), clip(t - g), clip(t + g), clip(t + g + w)
    nL, nR = cn[:, l1] - cn[:, l0], cn[:, r1] - cn[:, r0]
    with np.errstate(invalid="ignore", divide="ignore"):
        mL = (cs[:, l1] - cs[:, l0]) / nL
        mR = (cs[:, r1] - cs[:, r0]) / nR
    return mL, mR, nL, nR


def step_statistic(x, w, g=0, flags=None, min_count=None):
    """(s float32 [D, T], scale [D, T] = max(|mean_L|, |mean_R|) where s is formed, 0 elsewhere)."""
    m = w // 2 if min_count is None else min_count
    mL, mR, nL, nR = means(x, flags, w, g)
    good = (nL >= m) & (nR >= m)
    with np.errstate(invalid="ignore"):
        s = np.where(good, mR - mL, 0.0).astype(np.float32)
        scale = np.where(good, np.maximum(np.abs(mL), np.abs(mR)), 0.0)
    return s, scale


def step_statistic_by_loops(x, w, g=0, flags=None, min_count=None):
    """The same statistic by a double loop over samples and window entries."""
    x = np.asarray(x, np.float32)
    D, T = x.shape
    m = w // 2 if min_count is None else min_count
    ok = valid_mask(x, flags)
    s = np.zeros((D, T), np.float32)
    for d in range(D):
        for t in range(T):
            L = [u for u in range(t - g - w, t - g) if 0 <= u < T and ok[d, u]]
            R = [u for u in range(t + g, t + g + w) if 0 <= u < T and ok[d, u]]
            if len(L) >= m and len(R) >= m:
                s[d, t] = np.float32(np.sum(x[d, R].astype(np.float64)) / len(R) - np.sum(x[d, L].astype(np.float64)) / len(L))
    return s


def robust_scale(s):
    """[D] float64: 1.4826 times the lower median (element (T - 1) // 2 of the sorted row) of |s|."""
    s = np.asarray(s, np.float32)
    return 1.4826 * np.sort(np.abs(s), axis=1)[:, (s.shape[1] - 1) // 2].astype(np.float64)


def find(s, thresh, sep, grow_before, grow_after):
    """(flags uint8 [D, T], count [D] of peaks): the peak rule and the growing, by loops."""
    a = np.abs(np.asarray(s, np.float32))
    D, T = a.shape
    thresh = np.asarray(thresh, np.float32)
    out = np.zeros((D, T), np.uint8)
    count = np.zeros(D, np.int64)
    for d in range(D):
        peaks = []
        for t in np.flatnonzero(a[d] > thresh[d]):
            before, after = a[d, max(0, t - sep):t], a[d, t + 1:t + sep + 1]
            if np.all(before < a[d, t]) and np.all(after <= a[d, t]):
                peaks.append(t)
        for p in peaks:
            lo, hi = max(0, p - grow_before), min(T, p + grow_after + 1)
            out[d, lo:hi] = 2
        out[d, peaks] = 1
        count[d] = len(peaks)
    return out, count


def lists(flags):
    """(row_start int32 [D + 1], pos int32 [n]) of the samples whose flag is 1."""
    D = flags.shape[0]
    rows, pos = np.nonzero(np.asarray(flags) == 1)
    row_start = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=D))]).astype(np.int32)
    return row_start, pos.astype(np.int32)


def heights(x, row_start, pos, w, g, flags=None, min_count=None):
    """(height float64 [n], ok bool [n]): the clipped difference of means of every listed jump, by loops."""
    x = np.asarray(x, np.float32)
    D, T = x.shape
    m = w // 2 if min_count is None else min_count
    ok_s = valid_mask(x, flags)
    n = len(pos)
    height, ok = np.zeros(n), np.zeros(n, bool)
    for d in range(D):
        for j in range(row_start[d], row_start[d + 1]):
            p = int(pos[j])
            lo, hi = max(0, p - g - w), min(T, p + g + w)
            if j > row_start[d]:
                lo = max(lo, int(pos[j - 1]) + g)
            if j + 1 < row_start[d + 1]:
                hi = min(hi, int(pos[j + 1]) - g)
            L = [u for u in range(lo, p - g) if ok_s[d, u]]
            R = [u for u in range(p + g, hi) if ok_s[d, u]]
            if len(L) >= m and len(R) >= m:
                ok[j] = True
                height[j] = np.sum(x[d, R].astype(np.float64)) / len(R) - np.sum(x[d, L].astype(np.float64)) / len(L)
    return height, ok


def cumulative(row_start, height):
    """The inclusive cumulative sum of the heights within each row."""
    cum = np.zeros(len(height))
    for d in range(len(row_start) - 1):
        cum[row_start[d]:row_start[d + 1]] = np.cumsum(np.asarray(height, np.float64)[row_start[d]:row_start[d + 1]])
    return cum


def fix(x, row_start, pos, cum):
    """y float32: x less cum[row_start[d] + k - 1], k the number of the row's jumps at or before the sample."""
    x = np.asarray(x, np.float32)
    y = x.copy()
    T = x.shape[1]
    for d in range(x.shape[0]):
        p = np.asarray(pos[row_start[d]:row_start[d + 1]], np.int64)
        k = np.searchsorted(p, np.arange(T), side="right")
        some = k > 0
        y[d, some] = (x[d, some].astype(np.float64) - np.asarray(cum, np.float64)[row_start[d] + k[some] - 1]).astype(np.float32)
    return y


def quantised_statistic(D, T, seed):
    """[D, T] float32 of either sign whose magnitudes are geometric integers (1 with probability 1/2, 2 with 1/4, ..): the
    largest of any window is shared by several samples about as often as not, whatever the window's length."""
    rng = np.random.default_rng(seed)
    return (rng.geometric(0.5, (D, T)) * (2 * rng.integers(0, 2, (D, T)) - 1)).astype(np.float32)


def noisy_rows(D, T, w, seed):
    """(x float32 [D, T], flags uint8 [D, T], pos int64 [D, 4], height float64 [D, 4]): white N(0, 1) plus a 1/f part (the
    rfft of white noise times sqrt(0.01 / f), f in cycles a sample, f[0] := f[1]) plus 5; 2 % of the samples flagged at
    random, carrying +50; four jumps a row of 8 - 16 of either sign, at distinct nodes of a grid of 3 w inside
    [2 w, T - 2 w) plus one random offset in [0, w) common to the row."""
    rng = np.random.default_rng(seed)
    white = rng.standard_normal((D, T))
    f = np.fft.rfftfreq(T)
    f[0] = f[1]
    pink = np.fft.irfft(np.fft.rfft(rng.standard_normal((D, T)), axis=1) * np.sqrt(0.01 / f), n=T, axis=1)
    x = white + pink + 5.0
    flagged = rng.random((D, T)) < 0.02
    x[flagged] += 50.0
    nodes = np.arange(2 * w, T - 2 * w - w, 3 * w)  # node + offset < T - 2 w
    pos = np.zeros((D, 4), np.int64)
    height = np.zeros((D, 4))
    for d in range(D):
        pos[d] = np.sort(rng.choice(nodes, 4, replace=False)) + rng.integers(0, w)
        height[d] = rng.uniform(8.0, 16.0, 4) * (2.0 * rng.integers(0, 2, 4) - 1.0)
        for p, h in zip(pos[d], height[d]):
            x[d, p:] += h
    return x.astype(np.float32), flagged.astype(np.uint8), pos, height


def recover(x, flags, w, n_sigma, sep, gap):
    """The reference's chain on one TOD: (row_start, pos, height, ok, scale [D] of the statistic, jump flags)."""
    s, _ = step_statistic(x, w, 0, flags)
    scale = robust_scale(s)
    jf, _ = find(s, (n_sigma * scale).astype(np.float32), sep, 4, 4)
    row_start, pos = lists(jf)
    height, ok = heights(x, row_start, pos, w, gap, flags)
    return row_start, pos, height, ok, scale, jf
