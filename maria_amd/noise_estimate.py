"""Detector noise spectra estimated from the data: the Welch spectrum of every row on the device
(``mrx_tod_welch``) and a batched fit of the simulator's noise law to it.

The law is oracle/noise.py::one_sided_psd_model's, the one destripe_prior.py assumes: P(f) = P_w (1 + (f_knee / f)^alpha),
one-sided, P_w = 2 sigma^2 / fs for white noise of variance sigma^2 a sample.  The fit averages the Welch bins into
log-spaced bins over [f_min, f_max] and minimises the count-weighted squares of log P against the log of the model
averaged over the same Welch bins (so an exact model spectrum is recovered exactly), by Levenberg--Marquardt in torch
float64 over all detectors at once."""

from __future__ import annotations

import numpy as np
import torch

from ._lib import Context, ptr

MIN_NPERSEG, MAX_NPERSEG = 256, 8192  # mrx_tod_welch's lengths: the powers of two between
KNEE_FLOOR = 1e-3     # the knee's lower bound, in units of f_min: a white-only row ends there ("knee_at_floor")
ALPHA_MIN, ALPHA_MAX = 1e-3, 2.0
MAX_ITER = 200


def default_nperseg(T):
    """The largest supported power of two <= T / 8 (256 for T < 2048)."""
    if T < MIN_NPERSEG:
        raise ValueError(f"a row of {T} samples is shorter than the shortest segment ({MIN_NPERSEG})")
    return int(min(MAX_NPERSEG, max(MIN_NPERSEG, 1 << int(np.floor(np.log2(max(T // 8, 1)))))))


def check_nperseg(nperseg, T):
    if isinstance(nperseg, bool) or int(nperseg) != nperseg or not MIN_NPERSEG <= nperseg <= MAX_NPERSEG or int(nperseg) & (int(nperseg) - 1):
        raise ValueError(f"nperseg {nperseg!r}: a power of two in {MIN_NPERSEG} .. {MAX_NPERSEG}")
    if T < nperseg:
        raise ValueError(f"nperseg {nperseg} is longer than the row ({T} samples)")
    return int(nperseg)


def welch(x, fs, nperseg=None, ctx=None):
    """scipy.signal.welch(x, fs, nperseg=nperseg) of every row of a [D, T] float32 device tensor, with scipy's defaults
    (periodic Hann window, half overlap, each segment's mean removed, one-sided density).  Returns ``(f, psd)``: f
    [nperseg / 2 + 1] float64 and psd [D, nperseg / 2 + 1] float32, both on x's device."""
    if x.dim() != 2:
        raise ValueError(f"x has shape {tuple(x.shape)}: [D, T]")
    D, T = x.shape
    nperseg = default_nperseg(T) if nperseg is None else check_nperseg(nperseg, T)
    fs = float(fs)
    if not np.isfinite(fs) or fs <= 0:
        raise ValueError(f"fs {fs}: finite and > 0")
    if not x.is_cuda or x.dtype != torch.float32:
        raise ValueError("x: a float32 tensor on the GPU")
    if D < 1:
        raise ValueError("x has no rows")
    if x.stride(1) != 1:
        x = x.contiguous()
    if ctx is None:
        ctx = Context(x.device.index or 0)
        ctx.set_stream(torch.cuda.current_stream(x.device))
    psd = torch.empty((D, nperseg // 2 + 1), dtype=torch.float32, device=x.device)
    ctx.call("mrx_tod_welch", ptr(x), x.stride(0), D, T, nperseg, fs, ptr(psd))
    f = torch.arange(nperseg // 2 + 1, dtype=torch.float64, device=x.device) * (fs / nperseg)
    return f, psd


def log_bins(f, f_min=None, f_max=None, n_bins=32):
    """The Welch bins used and their log bin: (index of each used Welch bin, its log bin, counts of the non-empty log
    bins).  Defaults: from the first non-zero bin to 0.9 x the last (Nyquist)."""
    f = np.asarray(f, np.float64)
    if f.ndim != 1 or f.size < 3:
        raise ValueError("f: the spectrum's frequencies, at least 3")
    f_min = float(f[f > 0][0]) if f_min is None else float(f_min)
    f_max = 0.9 * float(f[-1]) if f_max is None else float(f_max)
    if int(n_bins) != n_bins or n_bins < 3:
        raise ValueError(f"n_bins {n_bins}: an integer >= 3")
    if not (0 < f_min < f_max):
        raise ValueError(f"empty fit range [{f_min}, {f_max}] Hz: need 0 < f_min < f_max")
    used = np.nonzero((f >= f_min) & (f <= f_max))[0]
    edges = np.geomspace(f_min, f_max, int(n_bins) + 1)
    b = np.clip(np.searchsorted(edges, f[used], side="right") - 1, 0, int(n_bins) - 1)
    _, b, counts = np.unique(b, return_inverse=True, return_counts=True)  # the non-empty bins, renumbered
    if counts.size < 3:
        raise ValueError(f"empty fit range [{f_min:.4g}, {f_max:.4g}] Hz: {used.size} Welch bins in {counts.size} log bins, need 3")
    return used, b, counts


def _solve3(A, b):
    """x = A^-1 b for a batch of 3 x 3 systems, by the adjugate (no per-matrix library call)"""
    a = [[A[:, i, j] for j in range(3)] for i in range(3)]
    c00 = a[1][1] * a[2][2] - a[1][2] * a[2][1]
    c01 = a[1][2] * a[2][0] - a[1][0] * a[2][2]
    c02 = a[1][0] * a[2][1] - a[1][1] * a[2][0]
    det = a[0][0] * c00 + a[0][1] * c01 + a[0][2] * c02
    inv = torch.stack([
        torch.stack([c00, a[0][2] * a[2][1] - a[0][1] * a[2][2], a[0][1] * a[1][2] - a[0][2] * a[1][1]], dim=1),
        torch.stack([c01, a[0][0] * a[2][2] - a[0][2] * a[2][0], a[0][2] * a[1][0] - a[0][0] * a[1][2]], dim=1),
        torch.stack([c02, a[0][1] * a[2][0] - a[0][0] * a[2][1], a[0][0] * a[1][1] - a[0][1] * a[1][0]], dim=1),
    ], dim=1) / det[:, None, None]
    return (inv @ b[:, :, None])[:, :, 0]


def fit_noise(f, psd, f_min=None, f_max=None, n_bins=32):
    """Fit P(f) = white (1 + (knee / f)^alpha) to every row of a Welch spectrum ([D, n_f], numpy or torch, any device).

    Returns a dict of float64 tensors on psd's device, one value per row: ``white`` (one-sided, signal units^2 / Hz),
    ``knee`` (Hz), ``alpha`` (in (0, 2]), ``sigma`` = sqrt(white fs / 2) (the white standard deviation of one sample, fs =
    2 f[-1]), and ``knee_at_floor`` (bool: no 1/f part was found, the knee sits at its floor KNEE_FLOOR f_min).  A row
    with a non-finite or non-positive value in the fit range gives NaN."""
    f_np = f.detach().cpu().numpy() if isinstance(f, torch.Tensor) else np.asarray(f)
    used, bins, counts = log_bins(f_np, f_min, f_max, n_bins)
    P = psd if isinstance(psd, torch.Tensor) else torch.as_tensor(np.asarray(psd))
    if P.dim() == 1:
        P = P[None]
    dev = P.device
    P = P.to(torch.float64)[:, torch.as_tensor(used, device=dev)]
    D, nb = P.shape[0], counts.size
    idx = torch.as_tensor(bins, device=dev)
    cnt = torch.as_tensor(counts, dtype=torch.float64, device=dev)
    logf = torch.as_tensor(np.log(f_np[used]), device=dev)
    lo_f, hi_f = float(f_np[used][0]), float(f_np[used][-1])

    avg = torch.zeros((used.size, nb), dtype=torch.float64, device=dev)
    avg[torch.arange(used.size, device=dev), idx] = 1.0
    avg /= cnt

    def bin_mean(v):  # [D, n_used] -> [D, nb]: one matrix product
        return v @ avg

    good = torch.isfinite(P).all(dim=1) & (P > 0).all(dim=1)
    y = torch.log(bin_mean(torch.where(good[:, None], P, torch.ones_like(P))))
    wts = cnt / cnt.sum()
    v_lo, v_hi = float(np.log(KNEE_FLOOR * lo_f)), float(np.log(hi_f))

    def model(th):
        """log of the bin-averaged model and its Jacobian [D, nb, 3] in (log white, log knee, alpha)."""
        u, v, a = th[:, 0:1], th[:, 1:2], th[:, 2:3]
        lr = v - logf[None, :]                      # log(knee / f)
        e = torch.exp(a * lr)
        q, dq_da = bin_mean(e), bin_mean(lr * e)
        m = u + torch.log1p(q)
        J = torch.stack([torch.ones_like(q), a * q / (1 + q), dq_da / (1 + q)], dim=2)
        return m, J

    # start: the white level from the upper quarter of the bins; the knee where the spectrum first falls below twice it
    top = max(1, nb // 4)
    u0 = torch.log(torch.exp(y[:, -top:]).mean(dim=1))
    centres = torch.as_tensor([float(np.exp(np.log(f_np[used][bins == k]).mean())) for k in range(nb)], device=dev)
    above = y > (u0[:, None] + np.log(2.0))
    last = torch.where(above.any(dim=1), nb - 1 - above.flip(1).float().argmax(dim=1), torch.zeros_like(u0, dtype=torch.long))
    v0 = torch.where(above.any(dim=1), torch.log(centres[last]), torch.full_like(u0, np.log(lo_f)))
    th = torch.stack([u0, v0, torch.ones_like(u0)], dim=1)
    lam = torch.full((D,), 1e-3, dtype=torch.float64, device=dev)

    def clamp(t):
        return torch.stack([t[:, 0], t[:, 1].clamp(v_lo, v_hi), t[:, 2].clamp(ALPHA_MIN, ALPHA_MAX)], dim=1)

    m, J = model(th)
    cost = ((y - m) ** 2 * wts).sum(dim=1)
    eye = torch.eye(3, dtype=torch.float64, device=dev)
    for _ in range(MAX_ITER):
        r = y - m
        JW = J * wts[None, :, None]
        A = JW.transpose(1, 2) @ J
        g = (JW * r[:, :, None]).sum(dim=1)
        Ad = A + lam[:, None, None] * (torch.diagonal(A, dim1=1, dim2=2)[:, :, None] * eye + 1e-12 * eye)
        step = _solve3(Ad, g)
        # a parameter on its bound whose step points out of the range is held there: the others are solved without it
        lo = torch.stack([torch.full_like(lam, -np.inf), torch.full_like(lam, v_lo), torch.full_like(lam, ALPHA_MIN)], dim=1)
        hi = torch.stack([torch.full_like(lam, np.inf), torch.full_like(lam, v_hi), torch.full_like(lam, ALPHA_MAX)], dim=1)
        held = ((th <= lo) & (step < 0)) | ((th >= hi) & (step > 0))
        if bool(held.any()):
            free = (~held).double()
            Ad = Ad * free[:, :, None] * free[:, None, :] + torch.diag_embed(1.0 - free)
            step = _solve3(Ad, g * free)
        new = clamp(th + step)
        m_new, J_new = model(new)
        c_new = ((y - m_new) ** 2 * wts).sum(dim=1)
        ok = c_new <= cost
        move = (new - th).abs().amax(dim=1)  # (a step into a bound moves nothing along it)
        th = torch.where(ok[:, None], new, th)
        m = torch.where(ok[:, None], m_new, m)
        J = torch.where(ok[:, None, None], J_new, J)
        cost_old, cost = cost, torch.where(ok, c_new, cost)
        lam = torch.where(ok, lam * 0.3, lam * 10.0).clamp(1e-12, 1e12)
        # every row moved a negligible distance, gained nothing, or cannot improve any further
        small = (move < 1e-9) | (ok & (cost_old - cost <= 1e-12 * cost_old))
        if bool((small | (lam >= 1e8)).all()):
            break
    white, knee, alpha = torch.exp(th[:, 0]), torch.exp(th[:, 1]), th[:, 2]
    nan = torch.full_like(white, float("nan"))
    fs = 2.0 * float(f_np[-1])
    white, knee, alpha = (torch.where(good, v, nan) for v in (white, knee, alpha))
    return {"white": white, "knee": knee, "alpha": alpha, "sigma": torch.sqrt(white * fs / 2.0),
            "knee_at_floor": good & (th[:, 1] <= v_lo + 1e-9)}
