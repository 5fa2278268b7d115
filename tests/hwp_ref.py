"""The float64 numpy reference of maria_amd.hwp: the lock-in decimator's three formulas, the modulation,
and the tolerances the tests hold the kernels to."""

import numpy as np


def _windows(v, n_taps, q):
    """[D, T_out, n_taps]: the zero-padded rows' windows at every q-th sample."""
    H = (n_taps - 1) // 2
    return np.lib.stride_tricks.sliding_window_view(np.pad(v, ((0, 0), (H, H))), n_taps, axis=1)[:, ::q]


def denominators(h, T, q):
    """[T_out]: the sum of the taps that meet the row at each output (the same correlation of a row of ones)."""
    h = np.asarray(h, np.float64)
    return (_windows(np.ones((1, int(T))), h.size, q) @ h)[0]


def demodulate(x, carrier, q, ht, hp):
    """``(y_t, y_q, y_u, den_t, den_p)`` in float64:
        y_t[d, j] =     sum_i hT[H + i]               x[d, j q + i] / sum_i hT[H + i]
        y_q[d, j] = 2 * sum_i hP[H + i] c[j q + i, 0] x[d, j q + i] / sum_i hP[H + i]
        y_u[d, j] = 2 * sum_i hP[H + i] c[j q + i, 1] x[d, j q + i] / sum_i hP[H + i],   -H <= i <= H, 0 <= j q + i < T."""
    x = np.asarray(x, np.float64)
    c = np.asarray(carrier, np.float64)
    ht, hp = np.asarray(ht, np.float64), np.asarray(hp, np.float64)
    T = x.shape[1]
    assert c.shape == (T, 2) and ht.size == hp.size and ht.size % 2 == 1
    den_t, den_p = denominators(ht, T, q), denominators(hp, T, q)
    y_t = (_windows(x, ht.size, q) @ ht) / den_t
    y_q = 2.0 * (_windows(x * c[None, :, 0], hp.size, q) @ hp) / den_p
    y_u = 2.0 * (_windows(x * c[None, :, 1], hp.size, q) @ hp) / den_p
    return y_t, y_q, y_u, den_t, den_p


def tolerance_t(ref, x, ht, den):
    """2^-23 |ref| + 1e-12 sum|hT| max|x| / min(den): one float32 rounding, and slack for the order of a float64 sum of at
    most 1025 terms (1025 * 2^-53 = 1.1e-13)."""
    return 2.0**-23 * np.abs(ref) + 1e-12 * np.abs(ht).sum() * np.abs(x).max() / den.min()


def tolerance_p(ref, cx, hp, den):
    """2^-23 |ref| + 2e-12 sum|hP| max|c x| / min(den): the same, times the mixing's factor 2."""
    return 2.0**-23 * np.abs(ref) + 2e-12 * np.abs(hp).sum() * np.abs(cx).max() / den.min()


def modulate(s_i, s_c, s_s, carrier):
    """i + c cos 4 chi + s sin 4 chi in float64."""
    c = np.asarray(carrier, np.float64)
    return np.asarray(s_i, np.float64) + np.asarray(s_c, np.float64) * c[None, :, 0] + np.asarray(s_s, np.float64) * c[None, :, 1]
