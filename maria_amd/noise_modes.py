"""Noise shared across detectors in the GLS map: per-detector 1/f noise plus m <= 16 stationary 1/f modes
that every detector sees through a constant coupling U [D, m],

    N = (S A S)^-1 + U C U^T,

S = diag(s) the pre-processing's per-sample weight (one row for every detector), A the block-diagonal Toeplitz section
of the per-detector lags k_d (maria_amd/noise_filter.py), C the m independent mode series, each of law
P_j(f) = white_j (1 + (knee_j / f)^alpha_j).  Only N^-1 is applied, by Woodbury on the truncated [0, T) space:

    A' = S A S,   N^-1 x = A' x - A' U b,   (B + U^T A' U) b = U^T A' x,   U^T A' U = S T(G) S,
    G[tau] = sum_d U[d, i] U[d, j] k_d[tau],   B = T(lags of 1 / P_j) (noise_filter.lags on the mode laws).

With Q = A'^(1/2) U, N^-1 = A'^(1/2) (I - Q (B + Q^T Q)^-1 Q^T) A'^(1/2): the middle factor is >= 0 for B >= 0 (the
Bartlett lags' Toeplitz sections are), so N^-1 is positive semi-definite as conjugate gradients need -- provided the inner
system is solved exactly.  It is m x T unknowns in float64, solved here by preconditioned conjugate gradients to a tight
tolerance: the operator by zero-padded FFT linear convolution, the preconditioner the per-frequency m x m inverse of
B(f) + G(f) on the padded grid.  The [D, T] work is two kernels, ``mrx_tod_mode_project`` (U^T z) and
``mrx_tod_noise_filter_modes`` (A' (x - U b)); everything else is torch and runs on the CPU as well."""

from __future__ import annotations

import logging

import numpy as np
import torch

from . import noise_filter
from ._lib import ptr

logger = logging.getLogger("maria")

MAX_MODES = 16           # the kernels' largest m
INNER_TOL_FACTOR = 1e-3  # the inner solve's tolerance against the outer conjugate gradients'
INNER_TOL_FLOOR = 1e-12  # ... and its floor, near float64 rounding of the sums
INNER_MAX_ITER = 1000


def _fast_size(n):
    """the smallest 2^a 3^b 5^c >= n"""
    best = 1 << max(0, int(n - 1).bit_length())
    p5 = 1
    while p5 < best:
        p35 = p5
        while p35 < best:
            p = p35
            while p < n:
                p *= 2
            best = min(best, p)
            p35 *= 3
        p5 *= 5
    return best


def g_lags(U, lag):
    """G[i, j, tau] = sum_d U[d, i] U[d, j] k_d[tau]: [m, m, K + 1] float64 from U [D, m] and the lags [D, K + 1]"""
    U, lag = U.to(torch.float64), lag.to(torch.float64)
    return torch.einsum("di,dj,dk->ijk", U, U, lag)


def mode_lags(law, fs, K, device=None):
    """[m, K + 1] float64 lags of 1 / P_j for the mode laws ``{"white", "knee", "alpha"}`` (noise_filter.lags)"""
    return noise_filter.lags(law["white"], law["knee"], law["alpha"], fs, K, device=device)


def _spectrum(lags, n):
    """real DFT on n points of the symmetric kernels lags[..., 0..K] placed at -K..K: [..., n / 2 + 1] float64"""
    K = lags.shape[-1] - 1
    kern = torch.zeros(lags.shape[:-1] + (n,), dtype=torch.float64, device=lags.device)
    kern[..., : K + 1] = lags
    if K:
        kern[..., n - K:] = lags[..., 1:].flip(-1)
    return torch.fft.rfft(kern, dim=-1).real


class InnerSystem:
    """(B + S T(G) S) b = a on [m, T] float64: the operator by zero-padded FFT linear convolution, the preconditioner the
    per-frequency inverse of B(f) + G(f), and the conjugate-gradient solve.  G [m, m, K + 1], beta (B's lags) [m, K + 1],
    s None or [T]; all on one device."""

    def __init__(self, G, beta, s, T):
        m, K = beta.shape[0], beta.shape[1] - 1
        if G.shape != (m, m, K + 1):
            raise ValueError(f"G has shape {tuple(G.shape)}; need {(m, m, K + 1)}")
        self.m, self.K, self.T = m, K, int(T)
        self.n = _fast_size(self.T + K)  # linear convolution: nothing wraps into [0, T)
        self.s = None if s is None else s.to(torch.float64).reshape(-1)
        self.Gf = _spectrum(G, self.n).permute(2, 0, 1).contiguous()  # [F, m, m]
        self.Gf = 0.5 * (self.Gf + self.Gf.transpose(1, 2))
        self.Bf = _spectrum(beta, self.n).T.contiguous()  # [F, m]
        M = self.Gf + torch.diag_embed(self.Bf)
        # B(f) + G(f) >= 0 (Fejer-smoothed non-negative symbols); a floor keeps the preconditioner definite where a
        # mode's 1/f law leaves almost nothing at the lowest frequencies
        scale = float(torch.diagonal(M, dim1=1, dim2=2).abs().max()) if M.numel() else 1.0
        eye = torch.eye(m, dtype=torch.float64, device=M.device)
        Minv = torch.linalg.inv(M + (1e-12 * (scale or 1.0)) * eye)
        self.Minv = 0.5 * (Minv + Minv.transpose(1, 2))
        self.iterations = []  # per solve

    def _conv(self, spec, v):
        """the symmetric block-circulant product on the padded grid, read back on [0, T): spec [F, m, m], v [m, T]"""
        V = torch.view_as_real(torch.fft.rfft(v, n=self.n, dim=1))  # [m, F, 2]
        Y = torch.einsum("fij,jfc->ifc", spec, V)
        return torch.fft.irfft(torch.view_as_complex(Y.contiguous()), n=self.n, dim=1)[:, : self.T]

    def matvec(self, v):
        """(B + S T(G) S) v for v [m, T] float64"""
        sv = v if self.s is None else v * self.s
        y = self._conv(self.Gf, sv)
        if self.s is not None:
            y = y * self.s
        V = torch.fft.rfft(v, n=self.n, dim=1)
        return y + torch.fft.irfft(V * self.Bf.T, n=self.n, dim=1)[:, : self.T]

    def precond(self, r):
        return self._conv(self.Minv, r)

    def solve(self, a, tol, max_iter=INNER_MAX_ITER):
        """b with |a - (B + S T(G) S) b| <= tol |a| by preconditioned conjugate gradients from 0; the iterations are
        appended to ``self.iterations``"""
        a = a.to(torch.float64)
        a_norm = float(torch.linalg.vector_norm(a))
        b = torch.zeros_like(a)
        if a_norm == 0.0 or not np.isfinite(a_norm):
            self.iterations.append(0)
            return b if a_norm == 0.0 else torch.full_like(a, float("nan"))
        r = a.clone()
        z = self.precond(r)
        p = z.clone()
        rz = float(torch.sum(r * z))
        it, rel = 0, 1.0
        while it < max_iter:
            Ap = self.matvec(p)
            alpha = rz / float(torch.sum(p * Ap))
            b.add_(p, alpha=alpha)
            r.sub_(Ap, alpha=alpha)
            it += 1
            rel = float(torch.linalg.vector_norm(r)) / a_norm
            if rel <= tol:
                break
            z = self.precond(r)
            rz_new = float(torch.sum(r * z))
            p = z + (rz_new / rz) * p
            rz = rz_new
        if rel > tol:
            logger.warning("noise modes: the inner solve stopped at |r|/|a| = %.3e after %d iterations (tol %.1e)", rel, it, tol)
        self.iterations.append(it)
        return b


class ModeModel:
    """What the mode-aware N^-1 of one TOD needs: U [D, m] float64 contiguous on the device, the inner system and its
    tolerance.  ``lag`` [D, K + 1] the detector lags, ``beta`` [m, K + 1] the mode lags, ``sqrt_w`` None or a [T] row."""

    def __init__(self, U, beta, lag, sqrt_w, T, tol):
        if sqrt_w is not None and sqrt_w.dim() != 1:
            raise ValueError("noise modes need one per-sample weight row shared by every detector")
        self.U = U.to(torch.float64).contiguous()
        self.inner = InnerSystem(g_lags(self.U, lag), beta, sqrt_w, T)
        self.tol = float(tol)

    @property
    def m(self):
        return self.U.shape[1]


def inner_tol(outer_tol):
    return max(INNER_TOL_FACTOR * float(outer_tol), INNER_TOL_FLOOR)


def project(ctx, x, U, out=None):
    """a[j, t] = sum_d U[d, j] x[d, t] on the device (``mrx_tod_mode_project``): x [D, T] float32 (rows may be strided), U
    [D, m] float64 contiguous; a new (or ``out``) [m, T] float64 tensor"""
    D, T = x.shape
    m = U.shape[1]
    if out is None:
        out = torch.empty((m, T), dtype=torch.float64, device=x.device)
    ctx.call("mrx_tod_mode_project", ptr(x), x.stride(0), D, T, ptr(U), m, ptr(out))
    return out


def filter_modes(ctx, x, lag, sqrt_w, U, b, out):
    """out = s (k * (s (x - U b))) per row on the device (``mrx_tod_noise_filter_modes``): b [m, T] float32 contiguous"""
    D, T = x.shape
    ld_w = sqrt_w.stride(0) if sqrt_w is not None and sqrt_w.dim() == 2 else 0
    ctx.call("mrx_tod_noise_filter_modes", ptr(x), x.stride(0), ptr(out), out.stride(0), D, T, ptr(lag), lag.shape[1] - 1, ptr(sqrt_w),
             ld_w, ptr(U), U.shape[1], ptr(b))
    return out


def apply(ctx, x, lag, sqrt_w, model, out=None, scratch=None):
    """y = N^-1 x for the mode model: (1) z = A' x into ``scratch``, (2) a = U^T z, (3) b from the inner solve, (4) y = A'
    (x - U b).  x [D, T] float32 (``out`` may be x: in place), lag [D, K + 1] float64 contiguous, sqrt_w None or a [T]
    row, scratch None (a new tensor) or a [D, T] float32 tensor other than x and out."""
    D, T = x.shape
    if out is None:
        out = torch.empty((D, T), dtype=torch.float32, device=x.device)
    z = noise_filter.apply(ctx, x, lag, sqrt_w, out=scratch)
    a = project(ctx, z, model.U)
    b = model.inner.solve(a, model.tol).to(torch.float32).contiguous()
    return filter_modes(ctx, x, lag, sqrt_w, model.U, b, out)


def fit(ctx, x, m, fit_law):
    """The mode model fitted to the pre-processed rows x [D, T] float32 on the device, ``fit_law(rows)`` the noise-law
    fit of float32 rows (a dict of ``white``, ``knee``, ``alpha``, ``sigma`` tensors, NaN where it fails):

    1. each detector's law, and its white sigma_d;
    2. V, the top m eigenvectors of the float64 Gram of the whitened rows diag(1 / sigma) x (rows whose fit failed left
       out), and U = diag(sigma) V;
    3. the mode series a = V^T diag(1 / sigma) x (``mrx_tod_mode_project``);
    4. the detector laws again, on the residual x - U a (the shared power counted once);
    5. the mode laws, fitted to the series' Welch spectra;
    6. modes whose law fails dropped.

    Returns a dict: ``law`` (the detector laws of step 4), ``modes`` [D, m'] float64, ``mode_law`` (dict of [m'] tensors)
    and ``dropped`` (the indices, among the m, of the modes dropped)."""
    D, T = x.shape
    first = fit_law(x)
    sigma = first["sigma"].to(torch.float64)
    good = torch.isfinite(sigma) & (sigma > 0)
    sig = torch.where(good, sigma, torch.zeros_like(sigma))
    w = torch.where(good, 1.0 / torch.where(good, sigma, torch.ones_like(sigma)), torch.zeros_like(sigma))
    gram = torch.zeros((D, D), dtype=torch.float64, device=x.device)
    chunk = max(1, min(T, (1 << 28) // max(D, 1)))  # 2 GiB of float64 rows at a time
    for lo in range(0, T, chunk):
        xc = x[:, lo:lo + chunk].to(torch.float64) * w[:, None]
        gram.addmm_(xc, xc.T)
    _, vecs = torch.linalg.eigh(gram)
    V = vecs[:, -m:].flip(1).contiguous()  # the leading eigenvector first
    V = torch.where(good[:, None], V, torch.zeros_like(V))
    U = (sig[:, None] * V).contiguous()
    a = project(ctx, x, (w[:, None] * V).contiguous())
    resid = torch.addmm(x, U.to(torch.float32), a.to(torch.float32), alpha=-1.0)
    law = fit_law(resid)
    del resid
    mlaw = fit_law(a.to(torch.float32).contiguous())
    ok = torch.isfinite(mlaw["white"]) & torch.isfinite(mlaw["knee"]) & torch.isfinite(mlaw["alpha"]) & (mlaw["white"] > 0)
    keep = torch.nonzero(ok).reshape(-1)
    dropped = torch.nonzero(~ok).reshape(-1).cpu().numpy()
    if dropped.size:
        logger.warning("noise modes: the law fit failed for mode(s) %s; they are dropped", dropped.tolist())
    return {"law": law, "modes": U[:, keep].contiguous(), "mode_law": {k: mlaw[k][keep] for k in ("white", "knee", "alpha")},
            "dropped": dropped}
