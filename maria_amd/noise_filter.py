"""The inverse-noise filter of the correlated-noise GLS map: per detector the lags k[0..K] of a symmetric
kernel whose Toeplitz section approximates N^-1 of the stationary noise law P(f) = white (1 + (knee / |f|)^alpha)
(maria_amd/noise_estimate.py's convention: one-sided, signal units^2 / Hz), and its application to a [D, T] TOD on the
device (``mrx_tod_noise_filter``).

    k[t] = w_B(t) (1 / M) sum_j 2 / (fs P(f_j)) exp(2 pi i j t / M),   f_j = j fs / M,   1 / P(0) = 0 when knee > 0,

M a power of two >= max(65536, 16 (K + 1)), w_B(t) = 1 - |t| / (K + 1) the Bartlett window.  The DTFT of the result is
the Fejer kernel (>= 0) smoothing the non-negative samples 2 / (fs P(f_j)): a non-negative mix, so the Toeplitz section
is positive semi-definite (definite unless every sample is 0), as conjugate gradients need.  White noise (knee 0) gives
exactly delta / sigma^2, sigma^2 = white fs / 2: noise_weights="fit"'s weight.  A law with a non-finite or non-positive
parameter (a failed fit) gives all lags 0: the detector weighs nothing."""

from __future__ import annotations

import numpy as np
import torch

from ._lib import ptr

MAX_LAG = 2048     # mrx_tod_noise_filter's largest K
MIN_GRID = 65536   # the frequency grid M at least
ROW_CHUNK = 256    # detectors a batched inverse transform takes at once (M / 2 + 1 complex values each)


def grid_size(K):
    M = MIN_GRID
    while M < 16 * (K + 1):
        M *= 2
    return M


def lags(white, knee, alpha, fs, K, device=None):
    """[D, K + 1] float64 lags k[0..K] of the inverse-noise kernel of each detector's law (scalars or [D] arrays, numpy or
    torch) at sample rate fs; on ``device`` (default: white's device, else the CPU)."""
    K = int(K)
    if not 0 <= K <= MAX_LAG:
        raise ValueError(f"K {K}: 0 .. {MAX_LAG}")
    if not (np.isfinite(fs) and fs > 0):
        raise ValueError(f"fs {fs}: finite and > 0")
    if device is None:
        device = white.device if isinstance(white, torch.Tensor) else "cpu"
    as64 = lambda v: torch.as_tensor(v, dtype=torch.float64, device=device).reshape(-1)  # noqa: E731
    w, kn, a = as64(white), as64(knee), as64(alpha)
    D = max(w.numel(), kn.numel(), a.numel())
    w, kn, a = (v.expand(D) if v.numel() == 1 else v for v in (w, kn, a))
    if not (w.numel() == kn.numel() == a.numel() == D):
        raise ValueError("white, knee and alpha must be scalars or arrays of one length")
    good = torch.isfinite(w) & torch.isfinite(kn) & (w > 0) & (kn >= 0) & ((kn == 0) | (torch.isfinite(a) & (a > 0)))
    M = grid_size(K)
    f = torch.arange(M // 2 + 1, dtype=torch.float64, device=device) * (fs / M)
    t = torch.arange(K + 1, dtype=torch.float64, device=device)
    bartlett = 1.0 - t / (K + 1)
    out = torch.zeros((D, K + 1), dtype=torch.float64, device=device)
    for lo in range(0, D, ROW_CHUNK):
        hi = min(D, lo + ROW_CHUNK)
        g = good[lo:hi]
        wc = torch.where(g, w[lo:hi], torch.ones_like(w[lo:hi]))[:, None]
        kc = torch.where(g, kn[lo:hi], torch.zeros_like(kn[lo:hi]))[:, None]
        ac = torch.where(g & (kc[:, 0] > 0), a[lo:hi], torch.ones_like(a[lo:hi]))[:, None]
        # 1 / P = f^alpha / (white (f^alpha + knee^alpha)): 0 at f = 0 when knee > 0, 1 / white when knee = 0
        fa = f[None, :] ** ac
        inv_p = torch.where(kc > 0, fa / (wc * (fa + kc**ac)), 1.0 / wc.expand(-1, f.numel()))
        c = (2.0 / fs) * inv_p
        k = torch.fft.irfft(c.to(torch.complex128), n=M, dim=1)[:, : K + 1]
        k = k * bartlett[None, :]
        k[kc[:, 0] == 0] = 0.0  # white: exactly delta / sigma^2
        k[:, 0] = torch.where(kc[:, 0] == 0, (2.0 / fs) / wc[:, 0], k[:, 0])
        out[lo:hi] = torch.where(g[:, None], k, torch.zeros_like(k))
    return out


def default_K(T):
    return max(0, min(MAX_LAG, int(T) - 1))


def apply(ctx, x, lag, sqrt_w=None, out=None):
    """y = s (k * (s x)) per row on the device (``mrx_tod_noise_filter``): x [D, T] float32 (rows may be strided), lag
    [D, K + 1] float64 contiguous, sqrt_w None, a [T] row shared by every detector or [D, T]; out None (a new tensor),
    or a [D, T] float32 tensor (x itself: in place)."""
    D, T = x.shape
    if out is None:
        out = torch.empty((D, T), dtype=torch.float32, device=x.device)
    lag = lag.contiguous()
    ld_w = 0
    if sqrt_w is not None and sqrt_w.dim() == 2:
        ld_w = sqrt_w.stride(0)
    ctx.call("mrx_tod_noise_filter", ptr(x), x.stride(0), ptr(out), out.stride(0), D, T, ptr(lag), lag.shape[1] - 1,
             ptr(sqrt_w), ld_w)
    return out


