"""The destriper's prior on the baseline offsets (Madam's C_a): a 1/f noise law turned into a weighted graph Laplacian over
each detector's baselines, evaluated on the host in numpy.

The noise law is the simulator's (oracle/noise.py::one_sided_psd_model): white plus pink, pink equal to white at the knee.
On the sample grid of rate fs the unit 1/f spectrum is two-sided, p(f) = |f|^-alpha on (-fs/2, fs/2] extended with period
fs, in the convention in which white noise of variance sigma^2 a sample is flat at sigma^2; detector d's 1/f part is then
sigma_d^2 knee_d^alpha p(f).

The mean of L consecutive samples, taken once every L samples, has on the baseline-rate grid nu_j = j fs / (L M) the
spectrum

    P_a(nu) = (1 / L) sum_{m=0}^{L-1} p(nu + m fs / L) H_L(nu + m fs / L)^2,   H_L(f) = sin(pi f L / fs) / (L sin(pi f / fs)),

a finite sum (white noise gives sigma^2 / L).  Its inverse, q_j = 1 / P_a(nu_j) with q_0 = 0 (the constant, which the map
absorbs), has the lags c_k = (1 / M) sum_j q_j cos(2 pi j k / M); the prior's weights are w_k = -c_k for k = 1 .. K, signed.
The prior on one detector's nb baselines is the Laplacian

    (T a)_b = sum_{k=1..K} w_k ( [b + k < nb] (a_b - a_{b+k}) + [b - k >= 0] (a_b - a_{b-k}) ),

so T 1 = 0 exactly, also at the ends, and C_a^-1 = s_d T with s_d = W_d / knee_d^alpha (W_d the mapper's per-detector
weight, 1 / sigma_d^2)."""

from __future__ import annotations

import numpy as np

MAX_LAGS = 64        # K: the prior's lags (mrx_baseline_prior_apply)
MAX_BAND = 16        # Kp: the preconditioner's band (mrx_baseline_band_factor)
LAG_CUTOFF = 1e-4    # lags beyond the last |c_k| > LAG_CUTOFF |c_1| are dropped
SYMBOL_TOL = 1e-12   # the symbol may dip below zero by this fraction of its maximum (rounding), no further
MIN_GRID = 4096      # M: at least this many points of the baseline-rate grid, and at least 2 nb


def unit_psd(f, fs, alpha):
    """p(f) = |f|^-alpha, f folded into (-fs/2, fs/2]; inf at multiples of fs."""
    f = np.mod(np.asarray(f, float), fs)
    g = np.minimum(f, fs - f)
    with np.errstate(divide="ignore"):
        return np.where(g > 0, g ** -float(alpha), np.inf)


def mean_response(f, fs, L):
    """H_L(f): the response of the L-sample mean (1 at multiples of fs)."""
    x = np.pi * np.asarray(f, float) / fs
    s = np.sin(x)
    small = np.abs(s) < 1e-300
    return np.where(small, 1.0, np.sin(L * x) / (L * np.where(small, 1.0, s)))


def grid_size(nb):
    """M: a power of two, at least 2 nb and at least MIN_GRID."""
    return 1 << int(np.ceil(np.log2(max(2 * nb, MIN_GRID))))


def baseline_psd(fs, L, alpha, M):
    """P_a(nu_j), j = 0 .. M-1, of the unit spectrum's L-sample means (P_a[0] = inf, the 1/f pole)."""
    nu = np.arange(M) * fs / (L * M)
    out = np.zeros(M)
    for m0 in range(0, L, 256):  # (chunks of aliases: M x 256 values at a time)
        f = nu[:, None] + np.arange(m0, min(L, m0 + 256))[None, :] * (fs / L)
        h = mean_response(f, fs, L)
        with np.errstate(invalid="ignore"):
            term = np.where(h == 0.0, 0.0, unit_psd(f, fs, alpha) * h * h)
        out += term.sum(axis=1)
    out /= L
    out[0] = np.inf
    return out


def inverse_lags(fs, L, alpha, M):
    """c_k, k = 0 .. M/2: the lags of the inverse covariance of the baseline means (q_0 = 0)."""
    q = 1.0 / baseline_psd(fs, L, alpha, M)
    q[0] = 0.0
    return np.fft.rfft(q).real / M  # (q is even: the cosine sum)


def symbol(w, n_theta=8193):
    """sum_k w_k 2 (1 - cos k theta) on theta in [0, pi]."""
    w = np.asarray(w, float)
    theta = np.linspace(0.0, np.pi, n_theta)
    k = np.arange(1, w.size + 1)
    return (2.0 * (1.0 - np.cos(np.outer(theta, k)))) @ w


def symbol_ok(w):
    """Is the Laplacian of these weights positive semi-definite in the interior (its symbol >= 0 to rounding)?"""
    s = symbol(w)
    return bool(s.min() >= -SYMBOL_TOL * max(s.max(), 0.0))


def prior_weights(fs, L, alpha, nb):
    """w_1 .. w_K of the prior for baselines of L samples at sample rate fs, slope alpha, nb baselines a detector.  K is
    the smallest lag beyond which every |c_k| <= LAG_CUTOFF |c_1|, at most MAX_LAGS.  Raises ValueError if the truncated
    prior's symbol goes negative.  One baseline a detector (nb = 1) has no neighbours: w = [0]."""
    alpha = float(alpha)
    if not 0.0 < alpha <= 2.0:
        raise ValueError(f"alpha {alpha}: in (0, 2]")
    if nb <= 1:
        return np.zeros(1)
    c = inverse_lags(float(fs), int(L), alpha, grid_size(nb))
    big = np.nonzero(np.abs(c[1:]) > LAG_CUTOFF * abs(c[1]))[0]
    K = int(min(MAX_LAGS, max(1, big[-1] + 1 if big.size else 1)))
    w = -c[1:K + 1]
    if not symbol_ok(w):
        raise ValueError(f"the prior's symbol goes negative (L {L}, alpha {alpha}, K {K}): not positive semi-definite")
    return w


def band_lags(w, band):
    """Kp: the largest number <= band of leading weights whose Laplacian has a symbol >= 0 (0: the diagonal)."""
    Kp = int(min(band, MAX_BAND, len(w)))
    while Kp > 0 and not symbol_ok(w[:Kp]):
        Kp -= 1
    return Kp


def laplacian(w, nb):
    """The dense [nb, nb] T of weights w (tests, small nb)."""
    T = np.zeros((nb, nb))
    for k, wk in enumerate(np.asarray(w, float), start=1):
        i = np.arange(nb - k)
        T[i, i + k] -= wk
        T[i + k, i] -= wk
        T[i, i] += wk
        T[i + k, i + k] += wk
    return T


def laplacian_diagonal(w, nb):
    """diag T: sum of the weights whose neighbour exists, [nb]."""
    b = np.arange(nb)
    w = np.asarray(w, float)
    k = np.arange(1, w.size + 1)
    return ((b[:, None] + k[None, :] < nb).astype(float) + (b[:, None] - k[None, :] >= 0)) @ w
